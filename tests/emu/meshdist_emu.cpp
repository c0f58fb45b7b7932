// meshdist_emu.cpp -- host instantiation of csrc/meshdist_core.h (test only): (a) the brute force over every face with the
// product's float32 tri_dist2, (b) the grid build (count -> scan -> fill) and the ring walk as host loops.
// Built with -ffp-contract=off, like the kernels.
#include <stdint.h>

#include <vector>

#include "meshdist_core.h"

using namespace r3g_md;

namespace {

// -> number of skipped faces, or -2 for an index outside [0, nv)
int64_t make_records(const float* v, int64_t nv, const int32_t* f, int64_t nf, std::vector<Tri>& tris, float lo[3], float hi[3]) {
    uint32_t elo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, ehi[3] = {0, 0, 0};
    int64_t skipped = 0;
    tris.resize(nf);
    for (int64_t i = 0; i < nf; ++i) {
        Tri t{};
        const int32_t i0 = f[3 * i], i1 = f[3 * i + 1], i2 = f[3 * i + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return -2;
        t.ax = v[3 * i0], t.ay = v[3 * i0 + 1], t.az = v[3 * i0 + 2];
        t.bx = v[3 * i1], t.by = v[3 * i1 + 1], t.bz = v[3 * i1 + 2];
        t.cx = v[3 * i2], t.cy = v[3 * i2 + 1], t.cz = v[3 * i2 + 2];
        if (tri_finite(t)) {
            t.valid = 1;
            const float c[9] = {t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz};
            for (int k = 0; k < 9; ++k) {
                const uint32_t e = enc_float(c[k]);
                if (e < elo[k % 3]) elo[k % 3] = e;
                if (e > ehi[k % 3]) ehi[k % 3] = e;
            }
        } else {
            ++skipped;
        }
        tris[i] = t;
    }
    for (int a = 0; a < 3; ++a) lo[a] = dec_float(elo[a]), hi[a] = dec_float(ehi[a]);
    return skipped;
}

}  // namespace

extern "C" {

float r3g_emu_tri_dist2(const float* p, const float* abc) {
    Tri t{};
    t.ax = abc[0], t.ay = abc[1], t.az = abc[2], t.bx = abc[3], t.by = abc[4], t.bz = abc[5], t.cx = abc[6], t.cy = abc[7], t.cz = abc[8];
    return tri_dist2(p[0], p[1], p[2], t);
}

// (a) every face, no grid
int r3g_emu_meshdist_brute(const float* v, int64_t nv, const int32_t* f, int64_t nf, const float* p, int64_t n, float* dist2,
                           int32_t* face, int64_t* skipped_out) {
    std::vector<Tri> tris;
    float lo[3], hi[3];
    const int64_t skipped = make_records(v, nv, f, nf, tris, lo, hi);
    if (skipped < 0) return (int)skipped;
    if (nf == 0 || skipped >= nf) return -1;
    for (int64_t i = 0; i < n; ++i) {
        const float px = p[3 * i], py = p[3 * i + 1], pz = p[3 * i + 2];
        if (!(finite(px) && finite(py) && finite(pz))) {
            dist2[i] = quiet_nan();
            face[i] = -1;
            continue;
        }
        float best = kInf;
        int32_t bf = kNoFace;
        for (int64_t k = 0; k < nf; ++k)
            if (tris[k].valid) take(tri_dist2(px, py, pz, tris[k]), (int32_t)k, best, bf);
        dist2[i] = best;
        face[i] = bf == kNoFace ? -1 : bf;
    }
    if (skipped_out) *skipped_out = skipped;
    return 0;
}

// (b) the product's build and query in host loops; `reverse_fill` fills the cells in the opposite face order (the order
// inside a cell, which integer atomics decide on the device, must not matter)
int r3g_emu_meshdist_grid(const float* v, int64_t nv, const int32_t* f, int64_t nf, int resolution, int reverse_fill, const float* p,
                          int64_t n, float* dist2, int32_t* face, int* resolution_out, int64_t* pairs_out, int64_t* skipped_out,
                          int64_t* tests_out) {
    std::vector<Tri> tris;
    float lo[3], hi[3];
    const int64_t skipped = make_records(v, nv, f, nf, tris, lo, hi);
    if (skipped < 0) return (int)skipped;
    if (nf == 0 || skipped >= nf) return -1;
    if (resolution < 0 || resolution > kMaxRes) return -1;
    int res = resolution ? resolution : initial_resolution(nf);
    Grid g;
    int64_t pairs = 0;
    for (;;) {
        g = make_grid(lo, hi, res);
        pairs = 0;
        for (int64_t k = 0; k < nf; ++k)
            if (tris[k].valid) pairs += tri_pairs(g, tris[k]);
        if (resolution || res == 1 || pairs <= kPairMult * nf) break;
        res /= 2;
    }
    const int64_t cells = (int64_t)res * res * res;
    std::vector<uint32_t> starts(cells + 1, 0), cursor(cells, 0);
    std::vector<int32_t> list(pairs);
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t kk = 0; kk < nf; ++kk) {
            const int64_t k = (pass == 1 && reverse_fill) ? nf - 1 - kk : kk;
            if (!tris[k].valid) continue;
            int l[3], h[3];
            tri_range(g, tris[k], l, h);
            for (int z = l[2]; z <= h[2]; ++z)
                for (int y = l[1]; y <= h[1]; ++y)
                    for (int x = l[0]; x <= h[0]; ++x) {
                        const int cell = cell_index(g, x, y, z);
                        if (pass == 0) ++starts[cell + 1];
                        else list[starts[cell] + cursor[cell]++] = (int32_t)k;
                    }
        }
        if (pass == 0)
            for (int64_t c = 0; c < cells; ++c) starts[c + 1] += starts[c];
    }
    int64_t tests = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t nt = 0;
        nearest(g, tris.data(), starts.data(), list.data(), p[3 * i], p[3 * i + 1], p[3 * i + 2], &dist2[i], &face[i], &nt);
        tests += nt;
    }
    if (resolution_out) *resolution_out = res;
    if (pairs_out) *pairs_out = pairs;
    if (skipped_out) *skipped_out = skipped;
    if (tests_out) *tests_out = tests;
    return 0;
}

}  // extern "C"
