// meshinside_emu.cpp -- host instantiation of csrc/meshinside_core.h (test only): (a) the brute force over every usable face
// with the product's `crossed`, (b) the column build (csrc/grid_csr.h through host_grid.h) and the query as host loops.
// Built with -ffp-contract=off, like the kernels.
#include "host_grid.h"
#include "meshinside_core.h"

using namespace r3g_mi;

namespace {

// -> number of skipped faces, or -2 for an index outside [0, nv); unusable records get ia = -1
int64_t make_records(const float* v, int64_t nv, const int32_t* f, int64_t nf, int axis, std::vector<Rec>& recs, float lo[2],
                     float hi[2]) {
    uint32_t elo[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, ehi[2] = {0, 0};
    int64_t skipped = 0;
    recs.resize(nf);
    for (int64_t i = 0; i < nf; ++i) {
        const int32_t i0 = f[3 * i], i1 = f[3 * i + 1], i2 = f[3 * i + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return -2;
        Rec r = make_rec(v + 3 * (int64_t)i0, i0, v + 3 * (int64_t)i1, i1, v + 3 * (int64_t)i2, i2, axis);
        if (rec_finite(r)) {
            const float c[6] = {r.au, r.av, r.bu, r.bv, r.cu, r.cv};
            for (int k = 0; k < 6; ++k) {
                const uint32_t e = r3g_grid::enc_float(c[k]);
                if (e < elo[k % 2]) elo[k % 2] = e;
                if (e > ehi[k % 2]) ehi[k % 2] = e;
            }
            if (!rec_usable(r)) r.ia = -1;
        } else {
            ++skipped;
            r.ia = -1;
        }
        recs[i] = r;
    }
    for (int a = 0; a < 2; ++a) lo[a] = r3g_grid::dec_float(elo[a]), hi[a] = r3g_grid::dec_float(ehi[a]);
    return skipped;
}

}  // namespace

extern "C" {

// (a) every usable face, no grid
int r3g_emu_meshinside_brute(const float* v, int64_t nv, const int32_t* f, int64_t nf, int axis, const float* p, int64_t n,
                             int32_t* count, int64_t* skipped_out) {
    if (axis < 0 || axis > 2) return -1;
    std::vector<Rec> recs;
    float lo[2], hi[2];
    const int64_t skipped = make_records(v, nv, f, nf, axis, recs, lo, hi);
    if (skipped < 0) return (int)skipped;
    if (nf == 0 || skipped >= nf) return -1;
    for (int64_t i = 0; i < n; ++i) {
        const float* q = p + 3 * i;
        if (!(finite(q[0]) && finite(q[1]) && finite(q[2]))) {
            count[i] = -1;
            continue;
        }
        const float pu = q[(axis + 1) % 3], pv = q[(axis + 2) % 3], pw = q[axis];
        int32_t c = 0;
        for (int64_t k = 0; k < nf; ++k)
            if (recs[k].ia >= 0 && crossed(pu, pv, pw, recs[k])) ++c;
        count[i] = c;
    }
    if (skipped_out) *skipped_out = skipped;
    return 0;
}

// (b) the product's build and query in host loops; `reverse_fill` fills the columns in the opposite face order (the order
// inside a column, which integer atomics decide on the device, must not matter)
int r3g_emu_meshinside_grid(const float* v, int64_t nv, const int32_t* f, int64_t nf, int axis, int resolution, int reverse_fill,
                            const float* p, int64_t n, int32_t* count, int* resolution_out, int64_t* pairs_out,
                            int64_t* skipped_out, int64_t* tests_out) {
    if (axis < 0 || axis > 2) return -1;
    HostGrid<2, Rec> T;
    float lo[2], hi[2];
    const int64_t skipped = make_records(v, nv, f, nf, axis, T.recs, lo, hi);
    if (skipped < 0) return (int)skipped;
    if (nf == 0 || skipped >= nf) return -1;
    if (resolution < 0 || resolution > kMaxRes) return -1;
    T.build(lo, hi, resolution, initial_resolution(nf), reverse_fill != 0);
    int64_t tests = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t nt = 0;
        count[i] = count_crossings(T.g, axis, T.recs.data(), T.starts.data(), T.list.data(), p[3 * i], p[3 * i + 1], p[3 * i + 2], &nt);
        tests += nt;
    }
    if (resolution_out) *resolution_out = T.g.res;
    if (pairs_out) *pairs_out = T.pairs;
    if (skipped_out) *skipped_out = skipped;
    if (tests_out) *tests_out = tests;
    return 0;
}

}  // extern "C"
