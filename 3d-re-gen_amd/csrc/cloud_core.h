// cloud_core.h -- per-element bodies of the point-cloud neighbour search (exact k nearest neighbours on a uniform grid).
//
// The contract: for a query p and a target point q_i, d2(p, q_i) = ((px-qx)^2 + (py-qy)^2) + (pz-qz)^2
// in float32, one rounding per operation, left to right, without contraction (-ffp-contract=off on both sides).  The answer
// for k is the k smallest pairs (d2, i) in lexicographic order, ascending; equal coordinates under distinct indices are
// distinct neighbours.  The host instantiation (tests/emu/cloud_emu.cpp) and the kernels (cloud_kernels.hip) run this one
// source and give identical bits.  The grid only prunes.  Every usable point is listed in exactly one cell, its home cell
// clamp(coord(x)), and the ring walk visits a cell at most once, so a point enters a k-list at most once; the stop rule
// pulls every bound inward by kBinMargin cells, which absorbs the rounding of coord(), so no point is missed either: the
// result depends neither on the resolution nor on the order of the points inside a cell.
#ifndef R3G_CLOUD_CORE_H
#define R3G_CLOUD_CORE_H
#include <stdint.h>

#include "meshdist_core.h"

#ifndef R3G_CL_HD
#define R3G_CL_HD static inline
#endif
#ifndef R3G_CL_HD_MEMBER                  // the same for member functions, which take no `static`
#define R3G_CL_HD_MEMBER inline
#endif

namespace r3g_cl {

using r3g_grid::clamp;
using r3g_grid::coord;
using r3g_grid::finite;
using r3g_grid::fmax2;
using r3g_grid::fmin2;
using r3g_grid::kBinMargin;
using r3g_md::beyond;
using r3g_md::fabs1;
using r3g_md::kInf;
using r3g_md::kSlackAbs;
using r3g_md::quiet_nan;
using Grid = r3g_grid::GridN<3>;

constexpr int kMaxRes = 256;              // cap: 256^3 = 2^24 cells
constexpr int kMaxK = 32;
constexpr int kPointsPerCell = 1;         // P of the automatic resolution: the fastest of 1, 2, 4, 8, 16 at k = 1 (profiles/cloud.md)
constexpr int32_t kNoIndex = 0x7fffffff;

// one target point, 16 bytes: one aligned load.  index < 0: out of the structure (a non-finite coordinate)
struct alignas(16) Pt {
    float x, y, z;
    int32_t index;
};

R3G_CL_HD bool pt_finite(float x, float y, float z) { return finite(x) && finite(y) && finite(z); }

// THE definition
R3G_CL_HD float dist2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// (d2, index) in lexicographic order
R3G_CL_HD bool before(float d, int32_t i, float e, int32_t j) { return d < e || (d == e && i < j); }

// automatic resolution: min(256, max(1, floor(cbrt(n_usable / P)))), in integers
R3G_CL_HD int auto_resolution(int64_t n_usable, int per_cell) {
    int r = 1;
    while (r < kMaxRes && (int64_t)(r + 1) * (r + 1) * (r + 1) * per_cell <= n_usable) ++r;
    return r;
}

// what the grid builder asks of a record (grid_csr.h): does it take part, and its home cell
R3G_CL_HD bool grid_member(const Pt& p) { return p.index >= 0; }
R3G_CL_HD int grid_home(const Grid& g, const Pt& p) {
    const int c[3] = {clamp(coord(g, 0, p.x), g.res), clamp(coord(g, 1, p.y), g.res), clamp(coord(g, 2, p.z), g.res)};
    return r3g_grid::index(g, c);
}

// A k-list: slots [0, k) sorted ascending by (d2, index); the k-th pair is mirrored in registers (kd, ki) so that a
// candidate that cannot enter costs no access to the list.  Store is where the slots live: get_d / get_i / set by slot
// number (LDS on the device, an array on the host).  K1: k == 1, no store at all.
struct NoStore {        // the store of K1
    R3G_CL_HD_MEMBER float get_d(int) const { return kInf; }
    R3G_CL_HD_MEMBER int32_t get_i(int) const { return kNoIndex; }
    R3G_CL_HD_MEMBER void set(int, float, int32_t) {}
};

template <bool K1, class Store>
struct KList {
    Store& st;
    int k;
    float kd;
    int32_t ki;
    R3G_CL_HD_MEMBER KList(Store& s, int k_) : st(s), k(k_), kd(kInf), ki(kNoIndex) {
        if (!K1)
            for (int j = 0; j < k; ++j) st.set(j, kInf, kNoIndex);
    }
    R3G_CL_HD_MEMBER void offer(float d, int32_t i) {
        if (!before(d, i, kd, ki)) return;
        if (K1) {
            kd = d, ki = i;
            return;
        }
        int j = k - 1;
        while (j > 0) {
            const float e = st.get_d(j - 1);
            const int32_t f = st.get_i(j - 1);
            if (!before(d, i, e, f)) break;
            st.set(j, e, f);
            --j;
        }
        st.set(j, d, i);
        kd = st.get_d(k - 1), ki = st.get_i(k - 1);
    }
    R3G_CL_HD_MEMBER float d_at(int j) const { return K1 ? kd : st.get_d(j); }
    R3G_CL_HD_MEMBER int32_t i_at(int j) const { return K1 ? ki : st.get_i(j); }
};

// distance along axis a from the point (cell coordinate tp) to the home slab of cell c, [c, c + 1) in computed coordinates,
// pulled inward by kBinMargin cells: a lower bound on the axis distance to every point whose home cell is c
R3G_CL_HD float cell_axis_dist(const Grid& g, int a, int c, float tp) {
    const float d = fmax2((float)c - tp, tp - (float)(c + 1)) - kBinMargin;
    return d > 0.0f ? d * g.h[a] : 0.0f;
}

template <class L>
R3G_CL_HD void visit_cell(const Pt* pts, const uint32_t* starts, int cell, float px, float py, float pz, L& list, uint32_t& ntests) {
    const uint32_t e = starts[cell + 1];
    for (uint32_t k = starts[cell]; k < e; ++k) {
        const Pt q = pts[k];
        list.offer(dist2(px, py, pz, q.x, q.y, q.z), q.index);
    }
    ntests += e - starts[cell];
}

// The query of one finite point: Chebyshev rings of cells around the point's (clamped) cell, as meshdist_core.h's nearest()
// walks them, against the k-th best value instead of the best.  pts: the points in cell order (starts[cells + 1]).
// After ring r every point not yet seen has its home cell outside the box [c - r, c + r] on some axis, so its computed
// coordinate on that axis lies beyond a face of that box that is interior to the grid; coord() is monotone and rounds by far
// less than kBinMargin cells where that matters (section 4k), so the point's true axis distance is at least the one to the
// face pulled inward by kBinMargin.  On the other two axes it is at least as far as the query is outside the bounding box.
template <class L>
R3G_CL_HD void knn_walk(const Grid& g, const Pt* pts, const uint32_t* starts, float px, float py, float pz, L& list, uint32_t* ntests_out) {
    const float p[3] = {px, py, pz};
    const int R = g.res;
    float tp[3], out2[3], far2 = 0.0f;
    int c[3], rmax = 0;
    for (int a = 0; a < 3; ++a) {
        tp[a] = coord(g, a, p[a]);
        c[a] = clamp(tp[a], R);
        const int m = c[a] > R - 1 - c[a] ? c[a] : R - 1 - c[a];
        rmax = m > rmax ? m : rmax;
        const float f = fmax2(fabs1(p[a] - g.lo[a]), fabs1(p[a] - g.hi[a]));
        far2 = far2 + f * f;
        const float o = fmax2(0.0f, fmax2(g.lo[a] - p[a], p[a] - g.hi[a]));     // how far outside the box on this axis
        out2[a] = o * o;
    }
    const float other2[3] = {out2[1] + out2[2], out2[0] + out2[2], out2[0] + out2[1]};
    const float slack_abs = kSlackAbs * far2;
    uint32_t ntests = 0;
    for (int r = 0;; ++r) {
        const int z0 = c[2] - r < 0 ? 0 : c[2] - r, z1 = c[2] + r > R - 1 ? R - 1 : c[2] + r;
        const int y0 = c[1] - r < 0 ? 0 : c[1] - r, y1 = c[1] + r > R - 1 ? R - 1 : c[1] + r;
        const int x0 = c[0] - r < 0 ? 0 : c[0] - r, x1 = c[0] + r > R - 1 ? R - 1 : c[0] + r;
        for (int z = z0; z <= z1; ++z) {
            const float dz = cell_axis_dist(g, 2, z, tp[2]);
            for (int y = y0; y <= y1; ++y) {
                const float dy = cell_axis_dist(g, 1, y, tp[1]);
                const float yz2 = dz * dz + dy * dy;
                if (beyond(yz2, slack_abs, list.kd)) continue;
                const bool shell = (z - c[2] == r) || (c[2] - z == r) || (y - c[1] == r) || (c[1] - y == r);
                const int xa = shell ? x0 : c[0] - r, xb = shell ? x1 : c[0] + r;
                const int step = shell ? 1 : 2 * r;             // inside the shell's z and y: only the two x faces (r > 0 there)
                for (int x = xa; x <= xb; x += step) {
                    if (x < 0 || x > R - 1) continue;
                    const float dx = cell_axis_dist(g, 0, x, tp[0]);
                    if (beyond(yz2 + dx * dx, slack_abs, list.kd)) continue;
                    const int cc[3] = {x, y, z};
                    visit_cell(pts, starts, r3g_grid::index(g, cc), px, py, pz, list, ntests);
                }
            }
        }
        if (r >= rmax) break;
        float b2 = kInf;
        for (int a = 0; a < 3; ++a) {
            if (c[a] - r > 0) {
                const float dt = tp[a] - (float)(c[a] - r) - kBinMargin;
                const float d = dt > 0.0f ? dt * g.h[a] : 0.0f;
                b2 = fmin2(b2, d * d + other2[a]);
            }
            if (c[a] + r < R - 1) {
                const float dt = (float)(c[a] + r + 1) - tp[a] - kBinMargin;
                const float d = dt > 0.0f ? dt * g.h[a] : 0.0f;
                b2 = fmin2(b2, d * d + other2[a]);
            }
        }
        if (beyond(b2, slack_abs, list.kd)) break;
    }
    if (ntests_out) *ntests_out = ntests;
}

// one query point -> d2_out [k], index_out [k] (stride 1): the k-list, padded with (+inf, -1); a query with a non-finite
// coordinate gets (quiet_nan(), -1) in every slot
template <bool K1, class Store>
R3G_CL_HD void knn(const Grid& g, const Pt* pts, const uint32_t* starts, float px, float py, float pz, int k, Store& store,
                   float* d2_out, int32_t* index_out, uint32_t* ntests_out) {
    if (!pt_finite(px, py, pz)) {
        for (int j = 0; j < k; ++j) d2_out[j] = quiet_nan(), index_out[j] = -1;
        if (ntests_out) *ntests_out = 0;
        return;
    }
    KList<K1, Store> list(store, k);
    knn_walk(g, pts, starts, px, py, pz, list, ntests_out);
    for (int j = 0; j < k; ++j) {
        const int32_t i = list.i_at(j);
        d2_out[j] = list.d_at(j);
        index_out[j] = i == kNoIndex ? -1 : i;
    }
}

}  // namespace r3g_cl
#endif
