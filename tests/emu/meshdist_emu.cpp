// meshdist_emu.cpp -- host instantiation of csrc/meshdist_core.h (test only): (a) the brute force over every face with the
// product's float32 tri_dist2, (b) the grid build (csrc/grid_csr.h through host_grid.h) and the ring walk as host loops.
// Built with -ffp-contract=off, like the kernels.
#include "meshdist_host.h"

using namespace r3g_md;

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
    Target T;
    float lo[3], hi[3];
    const int64_t skipped = make_records(v, nv, f, nf, T.recs, lo, hi);
    if (skipped < 0) return (int)skipped;
    if (nf == 0 || skipped >= nf) return -1;
    if (resolution < 0 || resolution > kMaxRes) return -1;
    T.build(lo, hi, resolution, initial_resolution(nf), reverse_fill != 0);
    int64_t tests = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t nt = 0;
        nearest(T.g, T.recs.data(), T.starts.data(), T.list.data(), p[3 * i], p[3 * i + 1], p[3 * i + 2], &dist2[i], &face[i], &nt);
        tests += nt;
    }
    if (resolution_out) *resolution_out = T.g.res;
    if (pairs_out) *pairs_out = T.pairs;
    if (skipped_out) *skipped_out = skipped;
    if (tests_out) *tests_out = tests;
    return 0;
}

}  // extern "C"
