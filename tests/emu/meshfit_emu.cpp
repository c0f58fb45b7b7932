// meshfit_emu.cpp -- host twin of the mesh registration (test only): csrc/meshdist_core.h (tri_closest, fit_point, the grid
// walk) and csrc/meshfit_core.h (the solver) in host loops, with the reduction order of DESIGN.md section 4h: lane, wave
// butterfly, the block's four waves in index order, then the blocks' records by the same tree.
// Built with -ffp-contract=off, like the kernels.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "meshdist_host.h"
#include "meshfit_core.h"

using namespace r3g_md;

namespace {

// the grid build of meshdist_emu.cpp; -> 0, -2 for an index outside [0, nv), -1 for a mesh without a usable face
int make_target(const float* v, int64_t nv, const int32_t* f, int64_t nf, int resolution, Target& T) {
    float lo[3], hi[3];
    const int64_t skipped = make_records(v, nv, f, nf, T.recs, lo, hi);
    if (skipped < 0) return (int)skipped;
    if (nf == 0 || skipped >= nf || resolution < 0 || resolution > kMaxRes) return -1;
    T.build(lo, hi, resolution, initial_resolution(nf), false);
    return 0;
}

template <int MODE>
void accumulate(const Target& T, const float* p, int64_t n, const float* w, const Sim& x, float md2, double* sums, int64_t* used_out) {
    constexpr int K = MODE == kFitPlane ? kFitPlaneTerms : kFitPointTerms;
    const int64_t nb = fit_blocks(n);
    std::vector<double> partial((size_t)nb * K), lanes((size_t)kFitBlock * K), col(kFitBlock);
    int64_t used = 0;
    for (int64_t b = 0; b < nb; ++b) {
        for (int t = 0; t < kFitBlock; ++t) {
            double* acc = &lanes[(size_t)t * K];
            for (int k = 0; k < K; ++k) acc[k] = 0.0;
            for (int64_t i = b * kFitBlock + t; i < n; i += nb * kFitBlock) {
                uint32_t u = 0, nt = 0;
                fit_point<MODE>(T.g, T.recs.data(), T.starts.data(), T.list.data(), x, p[3 * i], p[3 * i + 1], p[3 * i + 2],
                                w ? w[i] : 1.0f, md2, acc, &u, &nt);
                used += u;
            }
        }
        for (int k = 0; k < K; ++k) {
            for (int t = 0; t < kFitBlock; ++t) col[t] = lanes[(size_t)t * K + k];
            partial[(size_t)b * K + k] = fit_tree256(col.data());
        }
    }
    for (int k = 0; k < K; ++k) {
        for (int t = 0; t < kFitBlock; ++t) {
            double v = 0.0;
            for (int64_t b = t; b < nb; b += kFitBlock) v = v + partial[(size_t)b * K + k];
            col[t] = v;
        }
        sums[k] = fit_tree256(col.data());
    }
    *used_out = used;
}

void step(const Target& T, const float* p, int64_t n, const float* w, const Sim& x, int mode, double max_dist, double* sums, int64_t* used) {
    for (int k = 0; k < kFitMaxTerms; ++k) sums[k] = 0.0;
    *used = 0;
    if (n == 0) return;
    const float md2 = (float)(max_dist * max_dist);
    if (mode == kFitPlane) accumulate<kFitPlane>(T, p, n, w, x, md2, sums, used);
    else accumulate<kFitPoint>(T, p, n, w, x, md2, sums, used);
}

}  // namespace

extern "C" {

float r3g_emu_mf_tri_dist2(const float* p, const float* abc) {
    Tri t{};
    t.ax = abc[0], t.ay = abc[1], t.az = abc[2], t.bx = abc[3], t.by = abc[4], t.bz = abc[5], t.cx = abc[6], t.cy = abc[7], t.cz = abc[8];
    return tri_dist2(p[0], p[1], p[2], t);
}

// n points against n triangles, one each: dist2 of tri_dist2, dist2 and point of tri_closest
void r3g_emu_mf_tri_closest(const float* p, const float* abc, int64_t n, float* d2_dist, float* d2_closest, float* q) {
    for (int64_t i = 0; i < n; ++i) {
        const float* a = abc + 9 * i;
        Tri t{};
        t.ax = a[0], t.ay = a[1], t.az = a[2], t.bx = a[3], t.by = a[4], t.bz = a[5], t.cx = a[6], t.cy = a[7], t.cz = a[8];
        d2_dist[i] = tri_dist2(p[3 * i], p[3 * i + 1], p[3 * i + 2], t);
        d2_closest[i] = tri_closest(p[3 * i], p[3 * i + 1], p[3 * i + 2], t, &q[3 * i], &q[3 * i + 1], &q[3 * i + 2]);
    }
}

// r3g_meshdist_closest: the walk, then tri_closest on the winning face
int r3g_emu_mf_closest(const float* v, int64_t nv, const int32_t* f, int64_t nf, int resolution, const float* p, int64_t n,
                       float* dist2, int32_t* face, float* closest) {
    Target T;
    const int rc = make_target(v, nv, f, nf, resolution, T);
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i) {
        nearest(T.g, T.recs.data(), T.starts.data(), T.list.data(), p[3 * i], p[3 * i + 1], p[3 * i + 2], &dist2[i], &face[i], nullptr);
        if (face[i] >= 0) {
            dist2[i] = tri_closest(p[3 * i], p[3 * i + 1], p[3 * i + 2], T.recs[face[i]], &closest[3 * i], &closest[3 * i + 1], &closest[3 * i + 2]);
        } else {
            dist2[i] = closest[3 * i] = closest[3 * i + 1] = closest[3 * i + 2] = quiet_nan();
        }
    }
    return 0;
}

// r3g_meshfit_step; centre_out = the centre the sums are taken about
int r3g_emu_mf_step(const float* v, int64_t nv, const int32_t* f, int64_t nf, int resolution, const float* p, int64_t n, const float* w,
                    const double* xform, int mode, double max_dist, double* sums_out, int64_t* used_out, double* centre_out) {
    Target T;
    const int rc = make_target(v, nv, f, nf, resolution, T);
    if (rc) return rc;
    if ((mode != kFitPoint && mode != kFitPlane) || !(max_dist >= 0.0)) return -1;
    Sim x;
    x.s = xform[0];
    memcpy(x.r, xform + 1, sizeof x.r);
    memcpy(x.t, xform + 10, sizeof x.t);
    step(T, p, n, w, x, mode, max_dist, sums_out, used_out);
    if (centre_out) fit_centre(T.g, centre_out);
    return 0;
}

// r3g_meshfit: the same loop as r3g_api.cpp; -3: too few points
int r3g_emu_mf_fit(const float* v, int64_t nv, const int32_t* f, int64_t nf, const float* p, int64_t n, const float* w, const double* init,
                   int mode, int with_scale, int max_iterations, double tolerance, double max_dist, double* matrix_out, double* info_out) {
    Target T;
    const int rc = make_target(v, nv, f, nf, 0, T);
    if (rc) return rc;
    if ((mode != kFitPoint && mode != kFitPlane) || !(max_dist >= 0.0) || max_iterations < 0 || !(tolerance == tolerance)) return -1;
    Sim cur = r3g_mf::identity();
    if (init && !r3g_mf::from_matrix(init, &cur)) return -1;
    double rms = 0.0, rms_prev = 0.0, centre[3], sums[kFitMaxTerms];
    int64_t used = 0;
    int updates = 0, converged = 0;
    fit_centre(T.g, centre);
    const int iw = mode == kFitPlane ? 35 : 0, id = mode == kFitPlane ? 36 : 17;
    for (int it = 0; n > 0; ++it) {
        step(T, p, n, w, cur, mode, max_dist, sums, &used);
        if (used < 3 || !(sums[iw] > 0.0)) return -3;
        rms = sqrt(sums[id] / sums[iw]);
        if (it > 0 && fabs(rms_prev - rms) < tolerance) {
            converged = 1;
            break;
        }
        if (it >= max_iterations) break;
        Sim delta;
        const bool ok = mode == kFitPlane ? r3g_mf::solve_plane(sums, with_scale != 0, centre, &delta)
                                          : r3g_mf::solve_point(sums, with_scale != 0, centre, &delta);
        if (!ok) return -1;
        cur = r3g_mf::compose(delta, cur);
        ++updates;
        rms_prev = rms;
    }
    r3g_mf::to_matrix(cur, matrix_out);
    info_out[0] = updates, info_out[1] = converged, info_out[2] = rms, info_out[3] = (double)used, info_out[4] = cur.s;
    return 0;
}

// the solver alone: sums about `centre` -> xform13 (s, R, t) of the update in world coordinates
int r3g_emu_mf_solve(const double* sums, int mode, int with_scale, const double* centre, double* xform_out, int* dropped_out) {
    Sim d;
    int dropped = 0;
    const bool ok = mode == kFitPlane ? r3g_mf::solve_plane(sums, with_scale != 0, centre, &d, &dropped)
                                      : r3g_mf::solve_point(sums, with_scale != 0, centre, &d);
    if (!ok) return -1;
    xform_out[0] = d.s;
    memcpy(xform_out + 1, d.r, sizeof d.r);
    memcpy(xform_out + 10, d.t, sizeof d.t);
    if (dropped_out) *dropped_out = dropped;
    return 0;
}

// compose(a, b) and the 4 x 4 round trip
void r3g_emu_mf_compose(const double* a16, const double* b16, double* out16) {
    Sim a, b;
    if (!r3g_mf::from_matrix(a16, &a) || !r3g_mf::from_matrix(b16, &b)) {
        for (int i = 0; i < 16; ++i) out16[i] = NAN;
        return;
    }
    r3g_mf::to_matrix(r3g_mf::compose(a, b), out16);
}

}  // extern "C"
