// facecloud_core.h -- per-element bodies of the face-to-cloud distance: for every triangle, its nearest point of the cloud.
//
// The contract: for a triangle t and the usable points p_i of the cloud,
//     d2(t) = min_i tri_dist2(p_i, t)            section 4f's float32 function (meshdist_core.h), no contraction
//     index(t) = the lowest ORIGINAL index i attaining it
// that is the minimum of (d2, i) in lexicographic order: it depends neither on the order of visits nor on the grid.  Beside it
// come the closest point r of t to p_index with its barycentric weights w[3] (tri_nearest_w below), and diff = p_index - r.
// The host instantiation (tests/emu/facecloud_twin.cpp) and the kernels (facecloud_kernels.hip) run this one source and give
// identical bits.
//
// The grid only prunes.  It is the cloud's (cloud_core.h): every usable point is listed in exactly one cell, its home cell.  The
// thing that asks has extent, so the walk starts from a box of cells, not from one: [lo, hi] is the clamped cell box of the
// triangle's axis-aligned box, ring 0 is that box, ring r the cells of [lo - r, hi + r] outside ring r - 1's box.
//
// Why nothing is missed.  A point's distance to the triangle is at least its distance to the triangle's box, and that is at
// least the gap on any one axis, or the root of the gaps' squares over several.  A point whose home cell is c on axis a has its
// computed coordinate in [c, c + 1) up to the rounding of coord(), which is monotone and errs by far less than kBinMargin cells
// (section 4k); so the gap between the triangle's box [tlo, thi] (the same coord()) and the slab, pulled inward by kBinMargin,
// is a lower bound on the true axis gap in cells.  After ring r a point not yet seen has its home cell outside [lo - r, hi + r]
// on some axis, beyond a face of that box that is interior to the grid; on the other two axes it is inside the cloud's box, so
// at least as far from the triangle as the triangle's box lies outside the cloud's.
//
// Why the slack covers the rounding.  The bounds above are on the TRUE distance; the value that competes is tri_dist2's float32
// one.  Every candidate of tri_nearest is |p - x|^2 for a point x OF the triangle (meshdist_core.h), so the computed value
// undershoots the true squared distance by no more than the rounding of that one evaluation: the offsets p - a, the products
// t * ab and the three squares.  Each operand is a difference of two coordinates, one of the triangle's box and one of the
// cloud's box or the triangle's again, so it is at most 2 F in magnitude, where F^2 = far2 is the squared distance between the
// farthest pair of a corner of the triangle's box and a corner of the cloud's box (an edge of the triangle is at most twice the
// larger of its vertices' distances to any fixed point of the cloud's box).  A residual component is rounded three times at
// magnitude <= 3 F, so it errs by <= 9 u F with u = 2^-24, its square and the two additions add <= 3 u d2, and summed over the
// axes the computed value is at least d2 - (2 sqrt(3) * 9 u F * sqrt(d2) + 3 u d2) >= d2 - 35 u far2 for every point that is
// worth a bound (d2 <= far2).  slack_abs = kSlackAbs * far2 = 64 u far2 exceeds that, and beyond()'s relative part covers the
// rounding of the bound's own arithmetic, as in section 4f.  A point the walk never visits therefore has a computed value
// above the best one, and can neither win nor tie.
#ifndef R3G_FACECLOUD_CORE_H
#define R3G_FACECLOUD_CORE_H
#include <stdint.h>

#include "cloud_core.h"

#ifndef R3G_FC_HD
#define R3G_FC_HD static inline
#endif

namespace r3g_fc {

using r3g_cl::before;
using r3g_cl::Grid;
using r3g_cl::kNoIndex;
using r3g_cl::Pt;
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
using r3g_md::seg_nearest;
using r3g_md::Tri;

constexpr int kWideCells = 64;            // a face whose cell box holds more cells is walked by a wave (unmeasured: profiles/facecloud.md)
constexpr int kWave = 64;
constexpr int64_t kMaxFaces = 1ll << 29;
constexpr int kReport = 4;                // usable faces, point-triangle tests, wide faces, the largest ring walked

// deliberate departures from the definition, for the twin's tests alone (the kernels instantiate kNone)
enum Mutant { kNone = 0, kTieLessEqual = 1, kNoBinMargin = 2, kNoSlack = 3, kStopWithoutOther = 4, kRingWithoutCorners = 5, kSwapBc = 6 };

// tri_nearest<true> of meshdist_core.h, text for text, which also returns the barycentric weights of r: the same s, v, w that
// formed r.  Same bits of the value and of r as tri_closest (asserted on the CPU).
template <int M = kNone>
R3G_FC_HD float tri_nearest_w(float px, float py, float pz, const Tri& t, float* r, float* wt) {
    const float abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
    const float acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
    const float bcx = t.cx - t.bx, bcy = t.cy - t.by, bcz = t.cz - t.bz;
    const float apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
    const float bpx = px - t.bx, bpy = py - t.by, bpz = pz - t.bz;
    const float cpx = px - t.cx, cpy = py - t.cy, cpz = pz - t.cz;
    float s = 0.0f;
    float best = seg_nearest<true>(apx, apy, apz, abx, aby, abz, &s);
    r[0] = t.ax + s * abx, r[1] = t.ay + s * aby, r[2] = t.az + s * abz;
    wt[0] = 1.0f - s, wt[1] = s, wt[2] = 0.0f;
    float d = seg_nearest<true>(bpx, bpy, bpz, bcx, bcy, bcz, &s);
    if (d < best) {
        best = d;
        r[0] = t.bx + s * bcx, r[1] = t.by + s * bcy, r[2] = t.bz + s * bcz;
        wt[0] = 0.0f, wt[1] = 1.0f - s, wt[2] = s;
        if (M == kSwapBc) wt[1] = s, wt[2] = 1.0f - s;
    }
    d = seg_nearest<true>(apx, apy, apz, acx, acy, acz, &s);
    if (d < best) {
        best = d;
        r[0] = t.ax + s * acx, r[1] = t.ay + s * acy, r[2] = t.az + s * acz;
        wt[0] = 1.0f - s, wt[1] = 0.0f, wt[2] = s;
    }
    const float d1 = abx * apx + aby * apy + abz * apz, d2 = acx * apx + acy * apy + acz * apz;
    const float d3 = abx * bpx + aby * bpy + abz * bpz, d4 = acx * bpx + acy * bpy + acz * bpz;
    const float d5 = abx * cpx + aby * cpy + abz * cpz, d6 = acx * cpx + acy * cpy + acz * cpz;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (va > 0.0f && vb > 0.0f && vc > 0.0f) {
        const float den = va + vb + vc;
        float v = vb / den, w = vc / den;
        float qx = apx - v * abx - w * acx, qy = apy - v * aby - w * acy, qz = apz - v * abz - w * acz;
        const float g11 = abx * abx + aby * aby + abz * abz, g12 = abx * acx + aby * acy + abz * acz;
        const float g22 = acx * acx + acy * acy + acz * acz, det = g11 * g22 - g12 * g12;
        if (det > 0.0f) {
            const float e1 = abx * qx + aby * qy + abz * qz, e2 = acx * qx + acy * qy + acz * qz;
            const float v2 = v + (g22 * e1 - g12 * e2) / det, w2 = w + (g11 * e2 - g12 * e1) / det;
            if (v2 >= 0.0f && w2 >= 0.0f && v2 + w2 <= 1.0f) {
                qx = apx - v2 * abx - w2 * acx, qy = apy - v2 * aby - w2 * acy, qz = apz - v2 * abz - w2 * acz;
                v = v2, w = w2;
            }
        }
        d = qx * qx + qy * qy + qz * qz;
        if (d < best) {
            best = d;
            r[0] = t.ax + v * abx + w * acx, r[1] = t.ay + v * aby + w * acy, r[2] = t.az + v * abz + w * acz;
            wt[0] = (1.0f - v) - w, wt[1] = v, wt[2] = w;
        }
    }
    return best;
}

// the record of face (i0, i1, i2): valid only when every index lies in [0, V) and every vertex is finite; explicit comparisons
// decide, and nothing is read through an index that fails them
R3G_FC_HD Tri make_record(const float* verts, int64_t n_verts, int32_t i0, int32_t i1, int32_t i2) {
    Tri t;
    t.ax = t.ay = t.az = t.bx = t.by = t.bz = t.cx = t.cy = t.cz = 0.0f;
    t.valid = 0, t.pad1 = 0, t.pad2 = 0;
    if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) return t;
    t.ax = verts[3 * (int64_t)i0], t.ay = verts[3 * (int64_t)i0 + 1], t.az = verts[3 * (int64_t)i0 + 2];
    t.bx = verts[3 * (int64_t)i1], t.by = verts[3 * (int64_t)i1 + 1], t.bz = verts[3 * (int64_t)i1 + 2];
    t.cx = verts[3 * (int64_t)i2], t.cy = verts[3 * (int64_t)i2 + 1], t.cz = verts[3 * (int64_t)i2 + 2];
    t.valid = r3g_md::tri_finite(t) ? 1 : 0;
    return t;
}

// what the walk of one face knows before it starts
struct Walk {
    float tlo[3], thi[3];     // the face's box in cell coordinates (coord(), not clamped)
    int lo[3], hi[3];         // its clamped cell box
    float other2[3];          // per axis: how far the box lies outside the cloud's box on the OTHER two axes, squared and summed
    float slack_abs;
    int rmax;                 // the first ring whose box covers the grid
};

template <int M = kNone>
R3G_FC_HD Walk walk_setup(const Grid& g, const Tri& t) {
    Walk w;
    float mn[3], mx[3], out2[3], far2 = 0.0f;
    r3g_md::grid_box(t, mn, mx);
    w.rmax = 0;
    for (int a = 0; a < 3; ++a) {
        w.tlo[a] = coord(g, a, mn[a]), w.thi[a] = coord(g, a, mx[a]);
        w.lo[a] = clamp(w.tlo[a], g.res), w.hi[a] = clamp(w.thi[a], g.res);
        const int m = w.lo[a] > g.res - 1 - w.hi[a] ? w.lo[a] : g.res - 1 - w.hi[a];
        w.rmax = m > w.rmax ? m : w.rmax;
        const float f = fmax2(fmax2(fabs1(mn[a] - g.lo[a]), fabs1(mn[a] - g.hi[a])), fmax2(fabs1(mx[a] - g.lo[a]), fabs1(mx[a] - g.hi[a])));
        far2 = far2 + f * f;
        const float o = fmax2(0.0f, fmax2(g.lo[a] - mx[a], mn[a] - g.hi[a]));
        out2[a] = o * o;
    }
    w.other2[0] = out2[1] + out2[2], w.other2[1] = out2[0] + out2[2], w.other2[2] = out2[0] + out2[1];
    w.slack_abs = M == kNoSlack ? 0.0f : kSlackAbs * far2;
    return w;
}

// cells in the face's clamped box
R3G_FC_HD int box_cells(const Walk& w) { return (w.hi[0] - w.lo[0] + 1) * (w.hi[1] - w.lo[1] + 1) * (w.hi[2] - w.lo[2] + 1); }

// gap along axis a between the face's box and the home slab [c, c + 1) of cell c, pulled inward by kBinMargin: a lower bound on
// the axis distance between the face and every point whose home cell is c (cloud_core.h::cell_axis_dist, for a box)
template <int M = kNone>
R3G_FC_HD float cell_axis_gap(const Grid& g, const Walk& w, int a, int c) {
    const float d = fmax2((float)c - w.thi[a], w.tlo[a] - (float)(c + 1)) - (M == kNoBinMargin ? 0.0f : kBinMargin);
    return d > 0.0f ? d * g.h[a] : 0.0f;
}

// the running answer: the lexicographic minimum of (d2, index), with the winner's coordinates beside it
struct Best {
    float d;
    int32_t i;
    float x, y, z;
};
R3G_FC_HD Best best_none() { return Best{kInf, kNoIndex, 0.0f, 0.0f, 0.0f}; }

template <int M = kNone>
R3G_FC_HD bool best_before(float d, int32_t i, const Best& b) {
    if (M == kTieLessEqual) return d <= b.d;
    return before(d, i, b.d, b.i);
}

template <int M = kNone>
R3G_FC_HD void offer(Best& b, float d, const Pt& q) {
    if (best_before<M>(d, q.index, b)) b.d = d, b.i = q.index, b.x = q.x, b.y = q.y, b.z = q.z;
}

template <int M = kNone>
R3G_FC_HD void visit_cell(const Pt* pts, const uint32_t* starts, int cell, const Tri& t, Best& b, uint32_t& ntests) {
    const uint32_t e = starts[cell + 1];
    for (uint32_t k = starts[cell]; k < e; ++k) {
        const Pt q = pts[k];
        offer<M>(b, r3g_md::tri_dist2(q.x, q.y, q.z, t), q);
    }
    ntests += e - starts[cell];
}

// the clamped box of ring r
struct RingBox {
    int x0, x1, y0, y1, z0, z1;
};
R3G_FC_HD RingBox ring_box(const Walk& w, int R, int r) {
    RingBox b;
    b.x0 = w.lo[0] - r < 0 ? 0 : w.lo[0] - r, b.x1 = w.hi[0] + r > R - 1 ? R - 1 : w.hi[0] + r;
    b.y0 = w.lo[1] - r < 0 ? 0 : w.lo[1] - r, b.y1 = w.hi[1] + r > R - 1 ? R - 1 : w.hi[1] + r;
    b.z0 = w.lo[2] - r < 0 ? 0 : w.lo[2] - r, b.z1 = w.hi[2] + r > R - 1 ? R - 1 : w.hi[2] + r;
    return b;
}

// is cell (x, y, z) of ring r's box part of ring r, that is, outside ring r - 1's box?
template <int M = kNone>
R3G_FC_HD bool in_ring(const Walk& w, int r, int x, int y, int z) {
    if (r == 0) return true;
    const int q = r - 1;
    const bool ox = x < w.lo[0] - q || x > w.hi[0] + q, oy = y < w.lo[1] - q || y > w.hi[1] + q, oz = z < w.lo[2] - q || z > w.hi[2] + q;
    if (M == kRingWithoutCorners) return (ox ? 1 : 0) + (oy ? 1 : 0) + (oz ? 1 : 0) == 1;
    return ox || oy || oz;
}

// one cell of a ring: its bound against the best value so far, then its points
template <int M = kNone>
R3G_FC_HD void ring_cell(const Grid& g, const Pt* pts, const uint32_t* starts, const Walk& w, const Tri& t, int x, int y, int z, Best& b,
                         uint32_t& ntests) {
    const float dx = cell_axis_gap<M>(g, w, 0, x), dy = cell_axis_gap<M>(g, w, 1, y), dz = cell_axis_gap<M>(g, w, 2, z);
    if (beyond((dz * dz + dy * dy) + dx * dx, w.slack_abs, b.d)) return;
    const int cc[3] = {x, y, z};
    visit_cell<M>(pts, starts, r3g_grid::index(g, cc), t, b, ntests);
}

// does the walk end after ring r?  Either the ring's box covers the grid, or the smallest bound to a face of that box that is
// interior to the grid exceeds the best value.
template <int M = kNone>
R3G_FC_HD bool walk_ends(const Grid& g, const Walk& w, int r, float best) {
    if (r >= w.rmax) return true;
    const int R = g.res;
    const float margin = M == kNoBinMargin ? 0.0f : kBinMargin;
    float b2 = kInf;
    for (int a = 0; a < 3; ++a) {
        const float other = M == kStopWithoutOther ? 0.0f : w.other2[a];
        if (w.lo[a] - r > 0) {
            const float dt = w.tlo[a] - (float)(w.lo[a] - r) - margin;
            const float d = dt > 0.0f ? dt * g.h[a] : 0.0f;
            b2 = fmin2(b2, d * d + other);
        }
        if (w.hi[a] + r < R - 1) {
            const float dt = (float)(w.hi[a] + r + 1) - w.thi[a] - margin;
            const float d = dt > 0.0f ? dt * g.h[a] : 0.0f;
            b2 = fmin2(b2, d * d + other);
        }
    }
    return beyond(b2, w.slack_abs, best);
}

// The narrow walk: one lane, the cells of each ring in z, y, x order.  -> the last ring walked
template <int M = kNone>
R3G_FC_HD int walk_narrow(const Grid& g, const Pt* pts, const uint32_t* starts, const Walk& w, const Tri& t, Best& b, uint32_t& ntests) {
    for (int r = 0;; ++r) {
        const RingBox rb = ring_box(w, g.res, r);
        for (int z = rb.z0; z <= rb.z1; ++z)
            for (int y = rb.y0; y <= rb.y1; ++y)
                for (int x = rb.x0; x <= rb.x1; ++x)
                    if (in_ring<M>(w, r, x, y, z)) ring_cell<M>(g, pts, starts, w, t, x, y, z, b, ntests);
        if (walk_ends<M>(g, w, r, b.d)) return r;
    }
}

// The wide walk as one lane of a wave sees a ring: the cells of the ring's box in x-fastest order, every kWave-th from `lane`,
// against the lane's own running answer (which starts at the wave's answer after the previous ring).
template <int M = kNone>
R3G_FC_HD void wide_ring_lane(const Grid& g, const Pt* pts, const uint32_t* starts, const Walk& w, const Tri& t, int r, int lane, Best& b,
                              uint32_t& ntests) {
    const RingBox rb = ring_box(w, g.res, r);
    const int nx = rb.x1 - rb.x0 + 1, ny = rb.y1 - rb.y0 + 1, nz = rb.z1 - rb.z0 + 1;
    const int n = nx * ny * nz;               // at most 2^24
    for (int i = lane; i < n; i += kWave) {
        const int x = rb.x0 + i % nx, y = rb.y0 + (i / nx) % ny, z = rb.z0 + i / (nx * ny);
        if (in_ring<M>(w, r, x, y, z)) ring_cell<M>(g, pts, starts, w, t, x, y, z, b, ntests);
    }
}

// the lexicographic minimum of two answers (what the wave reduction applies)
R3G_FC_HD Best best_min(const Best& a, const Best& b) { return before(b.d, b.i, a.d, a.i) ? b : a; }

// what a usable face writes once its winner is known
template <int M = kNone>
R3G_FC_HD void finish(const Tri& t, const Best& b, float* dist2, int32_t* index, float* weights, float* diff) {
    float r[3], wt[3];
    tri_nearest_w<M>(b.x, b.y, b.z, t, r, wt);
    *dist2 = b.d;
    *index = b.i == kNoIndex ? -1 : b.i;
    weights[0] = wt[0], weights[1] = wt[1], weights[2] = wt[2];
    diff[0] = b.x - r[0], diff[1] = b.y - r[1], diff[2] = b.z - r[2];
}

// what an unusable face gets
R3G_FC_HD void finish_unusable(float* dist2, int32_t* index, float* weights, float* diff) {
    *dist2 = quiet_nan();
    *index = -1;
    weights[0] = weights[1] = weights[2] = 0.0f;
    diff[0] = diff[1] = diff[2] = 0.0f;
}

// The backward of one vertex: its corners in ascending corner index (corner c = 3 f + a); each adds g_f * (-2 w[f][a]) * diff[f],
// float32, left to right.  A corner whose face is unusable (index < 0) or whose g_f is not finite adds nothing; an id outside
// [0, 3 F) is passed over.
R3G_FC_HD void gather_vertex(const float* grad_dist2, const int32_t* index, const float* weights, const float* diff, const int32_t* corner_ids,
                             int64_t c0, int64_t c1, int64_t n_corners, float* out) {
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    c0 = c0 < 0 ? 0 : c0, c1 = c1 > n_corners ? n_corners : c1;
    for (int64_t c = c0; c < c1; ++c) {
        const int32_t id = corner_ids[c];
        if (id < 0 || id >= n_corners) continue;
        const int64_t f = id / 3;
        const float gf = grad_dist2[f];
        if (index[f] < 0 || !finite(gf)) continue;
        const float k = gf * (-2.0f * weights[id]);
        gx = gx + k * diff[3 * f], gy = gy + k * diff[3 * f + 1], gz = gz + k * diff[3 * f + 2];
    }
    out[0] = gx, out[1] = gy, out[2] = gz;
}

}  // namespace r3g_fc
#endif
