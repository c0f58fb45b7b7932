// facecloud_twin.cpp -- host instantiation of csrc/facecloud_core.h (test only): (a) the brute force over every usable point and every
// face with the product's float32 tri_dist2, (b) the cloud's grid build (csrc/grid_csr.h, host_fill_home) and the ring walk in host
// loops, with either fill order and both enumerations: the narrow one (one lane) and the wide one (64 lanes with a minimum after each
// ring, as fc_wide runs it).  `mutant` selects a deliberate departure from the definition (facecloud_core.h, Mutant), each of which a
// named fixture must expose.  Built with -ffp-contract=off, like the kernels, through tests/emu_facecloud.py.  With -DFACECLOUD_EMU_MAIN it is a stand-alone
// program (for a sanitizer build) that runs (a) and (b) on a lattice cloud against small, large, degenerate and invalid faces.
#include <stdint.h>

#include <vector>

#include "facecloud_core.h"

using namespace r3g_fc;

namespace {

// the cloud's records kernel on the host -> skipped
int64_t make_records(const float* pts, int64_t n, std::vector<Pt>& recs, float lo[3], float hi[3]) {
    int64_t skipped = 0;
    for (int a = 0; a < 3; ++a) lo[a] = kInf, hi[a] = -kInf;
    recs.resize(n);
    for (int64_t i = 0; i < n; ++i) {
        Pt p{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], (int32_t)i};
        if (r3g_cl::pt_finite(p.x, p.y, p.z)) {
            lo[0] = fmin2(lo[0], p.x), lo[1] = fmin2(lo[1], p.y), lo[2] = fmin2(lo[2], p.z);
            hi[0] = fmax2(hi[0], p.x), hi[1] = fmax2(hi[1], p.y), hi[2] = fmax2(hi[2], p.z);
        } else {
            p.x = p.y = p.z = 0.0f;
            p.index = -1;
            ++skipped;
        }
        recs[i] = p;
    }
    return skipped;
}

struct Out {
    float* dist2;
    int32_t* index;
    float* weights;
    float* diff;
};

template <int M>
void brute(const std::vector<Pt>& recs, const float* verts, int64_t V, const int32_t* tri, int64_t F, const Out& o, int64_t* report) {
    int64_t usable = 0, tests = 0;
    for (int64_t f = 0; f < F; ++f) {
        const Tri t = make_record(verts, V, tri[3 * f], tri[3 * f + 1], tri[3 * f + 2]);
        if (!t.valid) {
            finish_unusable(o.dist2 + f, o.index + f, o.weights + 3 * f, o.diff + 3 * f);
            continue;
        }
        ++usable;
        Best b = best_none();
        for (const Pt& q : recs)
            if (r3g_cl::grid_member(q)) offer<M>(b, r3g_md::tri_dist2(q.x, q.y, q.z, t), q), ++tests;
        finish<M>(t, b, o.dist2 + f, o.index + f, o.weights + 3 * f, o.diff + 3 * f);
    }
    if (report) report[0] = usable, report[1] = tests, report[2] = 0, report[3] = 0;
}

// mode 0: as the device classifies (wide above kWideCells), 1: every face narrow, 2: every face wide
template <int M>
void grid_walk(const Grid& g, const Pt* sorted, const uint32_t* starts, int mode, const float* verts, int64_t V, const int32_t* tri, int64_t F,
               const Out& o, int64_t* report) {
    int64_t usable = 0, tests = 0, n_wide = 0, max_ring = 0;
    for (int64_t f = 0; f < F; ++f) {
        const Tri t = make_record(verts, V, tri[3 * f], tri[3 * f + 1], tri[3 * f + 2]);
        if (!t.valid) {
            finish_unusable(o.dist2 + f, o.index + f, o.weights + 3 * f, o.diff + 3 * f);
            continue;
        }
        ++usable;
        const Walk w = walk_setup<M>(g, t);
        const bool wide = mode == 2 || (mode == 0 && box_cells(w) > kWideCells);
        Best b = best_none();
        uint32_t nt = 0;
        int ring = 0;
        if (!wide) {
            ring = walk_narrow<M>(g, sorted, starts, w, t, b, nt);
        } else {
            ++n_wide;
            for (;; ++ring) {
                Best lanes[kWave];
                for (int l = 0; l < kWave; ++l) {
                    lanes[l] = b;
                    wide_ring_lane<M>(g, sorted, starts, w, t, ring, l, lanes[l], nt);
                }
                for (int l = 0; l < kWave; ++l) b = best_min(b, lanes[l]);
                if (walk_ends<M>(g, w, ring, b.d)) break;
            }
        }
        tests += nt;
        max_ring = ring > max_ring ? ring : max_ring;
        finish<M>(t, b, o.dist2 + f, o.index + f, o.weights + 3 * f, o.diff + 3 * f);
    }
    if (report) report[0] = usable, report[1] = tests, report[2] = n_wide, report[3] = max_ring;
}

#define FC_DISPATCH(fn, ...)                                 \
    switch (mutant) {                                        \
        case kNone: fn<kNone>(__VA_ARGS__); break;           \
        case kTieLessEqual: fn<kTieLessEqual>(__VA_ARGS__); break; \
        case kNoBinMargin: fn<kNoBinMargin>(__VA_ARGS__); break;   \
        case kNoSlack: fn<kNoSlack>(__VA_ARGS__); break;     \
        case kStopWithoutOther: fn<kStopWithoutOther>(__VA_ARGS__); break; \
        case kRingWithoutCorners: fn<kRingWithoutCorners>(__VA_ARGS__); break; \
        case kSwapBc: fn<kSwapBc>(__VA_ARGS__); break;       \
        default: return -1;                                  \
    }

}  // namespace

extern "C" {

int r3g_emu_facecloud_wide_cells() { return kWideCells; }

// (a) every usable point against every face, no grid.  dist2 [F], index [F], weights [F][3], diff [F][3], report int64 [4]
int r3g_emu_facecloud_brute(const float* pts, int64_t n, const float* verts, int64_t V, const int32_t* tri, int64_t F, int mutant, float* dist2,
                            int32_t* index, float* weights, float* diff, int64_t* report) {
    if (n <= 0 || V < 0 || F < 0) return -1;
    std::vector<Pt> recs;
    float lo[3], hi[3];
    if (make_records(pts, n, recs, lo, hi) >= n) return -1;
    const Out o{dist2, index, weights, diff};
    FC_DISPATCH(brute, recs, verts, V, tri, F, o, report)
    return 0;
}

// (b) the cloud's build and the product's walk in host loops; `reverse_fill` fills the cells in the opposite point order (the order
// inside a cell, which integer atomics decide on the device, must not matter).  resolution 0: the cloud's automatic rule.
int r3g_emu_facecloud_grid(const float* pts, int64_t n, int resolution, int reverse_fill, int mode, int mutant, const float* verts, int64_t V,
                           const int32_t* tri, int64_t F, float* dist2, int32_t* index, float* weights, float* diff, int64_t* report,
                           int* resolution_out) {
    if (n <= 0 || V < 0 || F < 0 || resolution < 0 || resolution > r3g_cl::kMaxRes || mode < 0 || mode > 2) return -1;
    std::vector<Pt> recs;
    float lo[3], hi[3];
    const int64_t skipped = make_records(pts, n, recs, lo, hi);
    if (skipped >= n) return -1;
    const int res = resolution ? resolution : r3g_cl::auto_resolution(n - skipped, r3g_cl::kPointsPerCell);
    const Grid g = r3g_grid::make_grid(lo, hi, res);
    const int64_t cells = r3g_grid::cells<3>(res);
    std::vector<uint32_t> starts(cells + 1, 0), cursor(cells, 0);
    std::vector<Pt> sorted(n - skipped);
    r3g_grid::host_fill_home(g, recs.data(), n, reverse_fill != 0, starts.data(), cursor.data(), sorted.data());
    const Out o{dist2, index, weights, diff};
    FC_DISPATCH(grid_walk, g, sorted.data(), starts.data(), mode, verts, V, tri, F, o, report)
    if (resolution_out) *resolution_out = res;
    return 0;
}

// the backward: grad_verts [V][3] from the corner lists
int r3g_emu_facecloud_gather(int64_t V, int64_t F, const float* grad_dist2, const int32_t* index, const float* weights, const float* diff,
                             const int32_t* corner_start, const int32_t* corner_ids, float* grad_verts) {
    if (V < 0 || F < 0) return -1;
    for (int64_t v = 0; v < V; ++v)
        gather_vertex(grad_dist2, index, weights, diff, corner_ids, corner_start[v], corner_start[v + 1], 3 * F, grad_verts + 3 * v);
    return 0;
}

// tri_nearest_w beside section 4f's tri_closest, for n (point, triangle) pairs: p [n][3], abc [n][9] -> d2w [n], rw [n][3], w [n][3],
// d2c [n], rc [n][3]
int r3g_emu_facecloud_tri(const float* p, const float* abc, int64_t n, float* d2w, float* rw, float* w, float* d2c, float* rc) {
    for (int64_t i = 0; i < n; ++i) {
        Tri t;
        const float* q = abc + 9 * i;
        t.ax = q[0], t.ay = q[1], t.az = q[2], t.bx = q[3], t.by = q[4], t.bz = q[5], t.cx = q[6], t.cy = q[7], t.cz = q[8];
        t.valid = 1, t.pad1 = t.pad2 = 0;
        d2w[i] = tri_nearest_w(p[3 * i], p[3 * i + 1], p[3 * i + 2], t, rw + 3 * i, w + 3 * i);
        d2c[i] = r3g_md::tri_closest(p[3 * i], p[3 * i + 1], p[3 * i + 2], t, rc + 3 * i, rc + 3 * i + 1, rc + 3 * i + 2);
    }
    return 0;
}

}  // extern "C"

#ifdef FACECLOUD_EMU_MAIN
#include <stdio.h>
#include <string.h>

// a 9^3 lattice (every point on a cell border at resolution 8) with one NaN point, against faces inside one cell, across the box,
// far outside, degenerate, with a NaN vertex and with indices -1 and V; every resolution, fill order and enumeration against (a)
int main() {
    std::vector<float> pts;
    for (int z = 0; z < 9; ++z)
        for (int y = 0; y < 9; ++y)
            for (int x = 0; x < 9; ++x) pts.push_back(0.125f * x), pts.push_back(0.125f * y), pts.push_back(0.125f * z);
    pts[3 * 100] = __builtin_nanf("");
    const int64_t n = (int64_t)pts.size() / 3;
    const float nanv = __builtin_nanf("");
    const float verts[] = {0.30f, 0.31f, 0.32f,  0.33f, 0.30f, 0.34f,  0.31f, 0.35f, 0.30f,      // 0-2: inside one cell
                           -0.2f, -0.1f, 0.5f,   1.3f, 0.2f, 0.45f,    0.4f, 1.4f, 0.55f,       // 3-5: across the box
                           7.0f, 8.0f, -9.0f,    7.5f, 8.0f, -9.0f,    7.0f, 8.5f, -9.5f,       // 6-8: far outside
                           0.5f, 0.5f, 0.5f,     nanv, 0.0f, 0.0f,     0.9f, 0.1f, 0.52f};      // 9, 10 (NaN), 11
    const int64_t V = 12;
    const int32_t tri[] = {0, 1, 2,  3, 4, 5,  6, 7, 8,  9, 9, 9,  9, 11, 11,  0, 10, 2,  -1, 1, 2,  0, 1, 12,  3, 8, 11};
    const int64_t F = 9;
    std::vector<float> da(F), wa(3 * F), fa(3 * F), db(F), wb(3 * F), fb(3 * F);
    std::vector<int32_t> ia(F), ib(F);
    int64_t ra[4], rb[4];
    if (r3g_emu_facecloud_brute(pts.data(), n, verts, V, tri, F, 0, da.data(), ia.data(), wa.data(), fa.data(), ra)) return 2;
    int bad = 0;
    for (int res : {0, 1, 3, 8, 16})
        for (int rev = 0; rev < 2; ++rev)
            for (int mode = 0; mode < 3; ++mode) {
                if (r3g_emu_facecloud_grid(pts.data(), n, res, rev, mode, 0, verts, V, tri, F, db.data(), ib.data(), wb.data(), fb.data(), rb, nullptr))
                    return 2;
                bad += memcmp(da.data(), db.data(), 4 * F) != 0 || memcmp(ia.data(), ib.data(), 4 * F) != 0 ||
                       memcmp(wa.data(), wb.data(), 12 * F) != 0 || memcmp(fa.data(), fb.data(), 12 * F) != 0 || ra[0] != rb[0];
            }
    // the backward over hand-made corner lists: vertex 9 has five corners, vertex 10 one, vertex 6 one
    std::vector<int32_t> cstart(V + 1, 0), cids;
    for (int64_t v = 0; v < V; ++v) {
        for (int64_t c = 0; c < 3 * F; ++c)
            if (tri[c] == v) cids.push_back((int32_t)c);
        cstart[v + 1] = (int32_t)cids.size();
    }
    std::vector<float> grad(F, 1.0f), gv(3 * V);
    grad[1] = nanv;
    if (r3g_emu_facecloud_gather(V, F, grad.data(), ia.data(), wa.data(), fa.data(), cstart.data(), cids.data(), gv.data())) return 2;
    for (int64_t k = 0; k < 3 * V; ++k) bad += !(gv[k] - gv[k] == 0.0f);
    printf("facecloud_emu lattice: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif
