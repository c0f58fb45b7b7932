// meshdist_core.h -- per-element bodies of the mesh-to-mesh distance (exact nearest-triangle query on a uniform grid).
//
// The contract: for a point p and a triangle mesh, dist2 = min over all usable faces t of
// tri_dist2(p, t), face = the lowest face index attaining it.  tri_dist2 below IS the definition: one float32 function,
// evaluated without contraction (-ffp-contract=off on both sides), so the host instantiation (tests/emu/meshdist_emu.cpp)
// and the kernels (meshdist_kernels.hip) give identical bits.  The grid only prunes: the ring walk's stop rule carries a
// slack that covers the rounding of tri_dist2 on faces it never visits, so the result does not depend on the resolution.
#ifndef R3G_MESHDIST_CORE_H
#define R3G_MESHDIST_CORE_H
#include <stdint.h>

#include "grid_csr.h"

#ifndef R3G_MD_HD
#define R3G_MD_HD static inline
#endif

namespace r3g_md {

using r3g_grid::clamp;
using r3g_grid::coord;
using r3g_grid::dec_float;
using r3g_grid::enc_float;
using r3g_grid::finite;
using r3g_grid::fmax2;
using r3g_grid::fmin2;
using r3g_grid::kPairMult;
using r3g_grid::make_grid;
using Grid = r3g_grid::GridN<3>;      // cells (section 4f)

constexpr int kMaxRes = 256;                          // cap: 256^3 = 2^24 cells
constexpr float kSlackRel = 1.0f / 262144.0f;         // 2^-18 of the squared ring bound
constexpr float kSlackAbs = 1.0f / 262144.0f;         // 2^-18 of the squared distance to the farthest corner of the box
constexpr float kInf = __builtin_huge_valf();
constexpr int32_t kNoFace = 0x7fffffff;

// one face, padded to 48 bytes: three 16-byte loads
struct alignas(16) Tri {
    float ax, ay, az;
    int32_t valid;       // 0: out of the structure (non-finite vertex)
    float bx, by, bz;
    int32_t pad1;
    float cx, cy, cz;
    int32_t pad2;
};

R3G_MD_HD float fabs1(float a) { return a < 0.0f ? -a : a; }

// the NaN a non-finite query point gets: one bit pattern on host and device (inf - inf has the sign bit set on x86 only)
R3G_MD_HD float quiet_nan() {
    union { float f; uint32_t u; } c;
    c.u = 0x7fc00000u;
    return c.f;
}

// squared distance from the point with offset (apx, apy, apz) = p - a to the segment a + t * ab, t in [0, 1];
// a == b gives the point distance.  POINT: *t_out = the parameter of the closest point.
template <bool POINT>
R3G_MD_HD float seg_nearest(float apx, float apy, float apz, float abx, float aby, float abz, float* t_out) {
    const float den = abx * abx + aby * aby + abz * abz;
    const float num = apx * abx + apy * aby + apz * abz;
    float t = den > 0.0f ? num / den : 0.0f;
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    const float qx = apx - t * abx, qy = apy - t * aby, qz = apz - t * abz;
    if constexpr (POINT) *t_out = t;
    return qx * qx + qy * qy + qz * qz;
}

// Squared distance from p to the closest point of triangle (a, b, c): the minimum over the three edges (which hold the
// vertex and edge regions, and are all there is of a degenerate triangle) and, where p projects strictly inside, the
// interior point of Ericson's barycentric form (Real-Time Collision Detection 5.1.5).  Every candidate is the distance to
// a point OF the triangle, so the value never undershoots the true distance by more than its own rounding.
// POINT: also the point that attains it, through r[3].  The candidates come in the order edges ab,
// bc, ac, then the refined interior point; a later one replaces the point only when it is strictly nearer.  The point is
// base + t * edge (edges) or a + v * ab + w * ac (interior), one float32 operation each, left to right.  One body: the
// value is the same bits with and without the point, and without it nothing but the distance is computed.
template <bool POINT>
R3G_MD_HD float tri_nearest(float px, float py, float pz, const Tri& t, float* r) {
    const float abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
    const float acx = t.cx - t.ax, acy = t.cy - t.ay, acz = t.cz - t.az;
    const float bcx = t.cx - t.bx, bcy = t.cy - t.by, bcz = t.cz - t.bz;
    const float apx = px - t.ax, apy = py - t.ay, apz = pz - t.az;
    const float bpx = px - t.bx, bpy = py - t.by, bpz = pz - t.bz;
    const float cpx = px - t.cx, cpy = py - t.cy, cpz = pz - t.cz;
    float s = 0.0f;
    float best = seg_nearest<POINT>(apx, apy, apz, abx, aby, abz, &s);
    if constexpr (POINT) r[0] = t.ax + s * abx, r[1] = t.ay + s * aby, r[2] = t.az + s * abz;
    float d = seg_nearest<POINT>(bpx, bpy, bpz, bcx, bcy, bcz, &s);
    if (d < best) {
        best = d;
        if constexpr (POINT) r[0] = t.bx + s * bcx, r[1] = t.by + s * bcy, r[2] = t.bz + s * bcz;
    }
    d = seg_nearest<POINT>(apx, apy, apz, acx, acy, acz, &s);
    if (d < best) {
        best = d;
        if constexpr (POINT) r[0] = t.ax + s * acx, r[1] = t.ay + s * acy, r[2] = t.az + s * acz;
    }
    const float d1 = abx * apx + aby * apy + abz * apz, d2 = acx * apx + acy * apy + acz * apz;
    const float d3 = abx * bpx + aby * bpy + abz * bpz, d4 = acx * bpx + acy * bpy + acz * bpz;
    const float d5 = abx * cpx + aby * cpy + abz * cpz, d6 = acx * cpx + acy * cpy + acz * cpz;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (va > 0.0f && vb > 0.0f && vc > 0.0f) {
        const float den = va + vb + vc;                      // > 0 here
        float v = vb / den, w = vc / den;                    // v, w > 0 and v + w < 1: a point of the triangle
        float qx = apx - v * abx - w * acx, qy = apy - v * aby - w * acy, qz = apz - v * abz - w * acz;
        // One step of iterative refinement.  The barycentrics above come from products of dot products and lose a factor
        // 1 / sin^2 of the smallest angle (marching cubes is full of slivers); the residual q is small, so solving the
        // normal equations once more for it removes that.  Kept only while the point stays one of the triangle.
        const float g11 = abx * abx + aby * aby + abz * abz, g12 = abx * acx + aby * acy + abz * acz;
        const float g22 = acx * acx + acy * acy + acz * acz, det = g11 * g22 - g12 * g12;
        if (det > 0.0f) {
            const float e1 = abx * qx + aby * qy + abz * qz, e2 = acx * qx + acy * qy + acz * qz;
            const float v2 = v + (g22 * e1 - g12 * e2) / det, w2 = w + (g11 * e2 - g12 * e1) / det;
            if (v2 >= 0.0f && w2 >= 0.0f && v2 + w2 <= 1.0f) {
                qx = apx - v2 * abx - w2 * acx, qy = apy - v2 * aby - w2 * acy, qz = apz - v2 * abz - w2 * acz;
                if constexpr (POINT) v = v2, w = w2;
            }
        }
        d = qx * qx + qy * qy + qz * qz;
        if (d < best) {
            best = d;
            if constexpr (POINT) r[0] = t.ax + v * abx + w * acx, r[1] = t.ay + v * aby + w * acy, r[2] = t.az + v * abz + w * acz;
        }
    }
    return best;
}

R3G_MD_HD float tri_dist2(float px, float py, float pz, const Tri& t) { return tri_nearest<false>(px, py, pz, t, nullptr); }

R3G_MD_HD float tri_closest(float px, float py, float pz, const Tri& t, float* cx, float* cy, float* cz) {
    float r[3];
    const float d = tri_nearest<true>(px, py, pz, t, r);
    *cx = r[0], *cy = r[1], *cz = r[2];
    return d;
}

// (dist2, face) in lexicographic order: the order in which candidates arrive does not matter
R3G_MD_HD void take(float d, int32_t f, float& best, int32_t& bface) {
    if (d < best || (d == best && f < bface)) {
        best = d;
        bface = f;
    }
}

R3G_MD_HD bool tri_finite(const Tri& t) {
    return finite(t.ax) && finite(t.ay) && finite(t.az) && finite(t.bx) && finite(t.by) && finite(t.bz) && finite(t.cx) &&
           finite(t.cy) && finite(t.cz);
}

// first resolution tried for F faces: a closed surface of F faces crosses ~3 R^2 cells, so R = sqrt(F / 2) leaves one to a
// few triangles in an occupied cell
R3G_MD_HD int initial_resolution(int64_t nf) {
    int r = 1;
    while (r < kMaxRes && (int64_t)(r + 1) * (r + 1) * 2 <= nf) ++r;
    return r;
}

// what the grid builder asks of a record (grid_csr.h): does it take part, and its axis-aligned box
R3G_MD_HD bool grid_member(const Tri& t) { return t.valid != 0; }
R3G_MD_HD void grid_box(const Tri& t, float mn[3], float mx[3]) {
    mn[0] = fmin2(t.ax, fmin2(t.bx, t.cx)), mn[1] = fmin2(t.ay, fmin2(t.by, t.cy)), mn[2] = fmin2(t.az, fmin2(t.bz, t.cz));
    mx[0] = fmax2(t.ax, fmax2(t.bx, t.cx)), mx[1] = fmax2(t.ay, fmax2(t.by, t.cy)), mx[2] = fmax2(t.az, fmax2(t.bz, t.cz));
}

// the grid helpers under the names of this header's interface: a triangle's cell range, its pair count, a cell's index
R3G_MD_HD void tri_range(const Grid& g, const Tri& t, int lo[3], int hi[3]) { r3g_grid::range(g, t, lo, hi); }
R3G_MD_HD int64_t tri_pairs(const Grid& g, const Tri& t) { return r3g_grid::pairs(g, t); }
R3G_MD_HD int cell_index(const Grid& g, int x, int y, int z) {
    const int c[3] = {x, y, z};
    return r3g_grid::index(g, c);
}

R3G_MD_HD void visit_cell(const Tri* tris, const uint32_t* starts, const int32_t* pairs, int cell, float px, float py,
                          float pz, float& best, int32_t& bface, uint32_t& ntests) {
    const uint32_t e = starts[cell + 1];
    for (uint32_t k = starts[cell]; k < e; ++k) {
        const int32_t f = pairs[k];
        take(tri_dist2(px, py, pz, tris[f]), f, best, bface);
        ++ntests;
    }
}

// distance along axis a from the point (cell coordinate tp) to cell k's slab [k, k + 1]
R3G_MD_HD float cell_axis_dist(const Grid& g, int a, int k, float tp) {
    const float d = fmax2((float)k - tp, tp - (float)(k + 1));
    return d > 0.0f ? d * g.h[a] : 0.0f;
}

// true when a squared lower bound v, less the slack, still exceeds the best value: nothing behind it can win or tie
R3G_MD_HD bool beyond(float v, float slack_abs, float best) { return v - (v * kSlackRel + slack_abs) > best; }

// A cell is skipped when its own box is beyond the best value: a face's closest point lies in a cell that lists the face,
// and that cell is no farther than the face, so the winner is always met in a cell that is not skipped.
// The query of one point: Chebyshev rings of cells around the point's (clamped) cell.  After ring r every face not yet seen
// has no cell inside the box [c - r, c + r], so on some axis its whole cell range lies beyond that box, past a face of the
// box that is interior to the grid.  Its distance is at least the point's axis distance to that face; and since every face
// lies inside the bounding box, on the other two axes it is at least as far as the point is outside the box (this keeps
// points far outside from walking the whole grid).  The walk stops once the best value is below the smallest such bound
// squared, less the slack.  Once the box of cells covers the grid nothing is left.
R3G_MD_HD void nearest(const Grid& g, const Tri* tris, const uint32_t* starts, const int32_t* pairs, float px, float py,
                       float pz, float* dist2_out, int32_t* face_out, uint32_t* ntests_out) {
    if (!(finite(px) && finite(py) && finite(pz))) {
        *dist2_out = quiet_nan();
        *face_out = -1;
        return;
    }
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
    float best = kInf;
    int32_t bface = kNoFace;
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
                if (beyond(yz2, slack_abs, best)) continue;
                const bool shell = (z - c[2] == r) || (c[2] - z == r) || (y - c[1] == r) || (c[1] - y == r);
                const int xa = shell ? x0 : c[0] - r, xb = shell ? x1 : c[0] + r;
                const int step = shell ? 1 : 2 * r;             // inside the shell's z and y: only the two x faces (r > 0 there)
                for (int x = xa; x <= xb; x += step) {
                    if (x < 0 || x > R - 1) continue;
                    const float dx = cell_axis_dist(g, 0, x, tp[0]);
                    if (beyond(yz2 + dx * dx, slack_abs, best)) continue;
                    visit_cell(tris, starts, pairs, cell_index(g, x, y, z), px, py, pz, best, bface, ntests);
                }
            }
        }
        if (r >= rmax) break;
        float b2 = kInf;
        for (int a = 0; a < 3; ++a) {
            if (c[a] - r > 0) {
                const float dt = tp[a] - (float)(c[a] - r);
                const float d = dt > 0.0f ? dt * g.h[a] : 0.0f;
                b2 = fmin2(b2, d * d + other2[a]);
            }
            if (c[a] + r < R - 1) {
                const float dt = (float)(c[a] + r + 1) - tp[a];
                const float d = dt > 0.0f ? dt * g.h[a] : 0.0f;
                b2 = fmin2(b2, d * d + other2[a]);
            }
        }
        if (beyond(b2, slack_abs, best)) break;
    }
    *dist2_out = best;
    *face_out = bface == kNoFace ? -1 : bface;
    if (ntests_out) *ntests_out = ntests;
}

// ---- registration: what one point adds to the sums of a fit step --------------------------------
// All of it float64 on float32 inputs, one operation per product and sum, left to right, no contraction: the host twin
// (tests/emu/meshfit_emu.cpp) and the kernels (meshfit_kernels.hip) add the same bits in the same order.
constexpr int kFitPoint = 0, kFitPlane = 1;
constexpr int kFitPointTerms = 18;      // W, sum w p [3], sum w q [3], sum w p q^T [9, row = p], sum w |p|^2, sum w d^2
constexpr int kFitPlaneTerms = 37;      // upper triangle of sum g j j^T [28, row-major], sum g j r [7], W, sum w d^2
constexpr int kFitMaxTerms = 37;
constexpr int kFitRecord = 40;          // 8-byte slots of a partial record: the terms, then [38] = used, [39] = tests (uint64)
constexpr int kFitBlock = 256;          // lanes per block: four waves
constexpr int kFitMaxBlocks = 4096;     // blocks of a step; beyond 2^20 points a lane takes several, in index order

R3G_MD_HD int fit_terms(int mode) { return mode == kFitPlane ? kFitPlaneTerms : kFitPointTerms; }
R3G_MD_HD int64_t fit_blocks(int64_t n) {
    const int64_t b = (n + kFitBlock - 1) / kFitBlock;
    return b < 1 ? 1 : (b > kFitMaxBlocks ? kFitMaxBlocks : b);
}

// similarity p -> s R p + t (R row-major)
struct Sim {
    double s;
    double r[9];
    double t[3];
};

// the moved point, rounded to float32: the grid walk and every sum see this value
R3G_MD_HD void sim_apply(const Sim& x, float px, float py, float pz, float* ox, float* oy, float* oz) {
    const double X = (double)px, Y = (double)py, Z = (double)pz;
    const double rx = x.r[0] * X + x.r[1] * Y + x.r[2] * Z;
    const double ry = x.r[3] * X + x.r[4] * Y + x.r[5] * Z;
    const double rz = x.r[6] * X + x.r[7] * Y + x.r[8] * Z;
    *ox = (float)(x.s * rx + x.t[0]);
    *oy = (float)(x.s * ry + x.t[1]);
    *oz = (float)(x.s * rz + x.t[2]);
}

// centre of the grid's box: the sums are taken about it, so that their products stay small
R3G_MD_HD void fit_centre(const Grid& g, double c[3]) {
    for (int a = 0; a < 3; ++a) c[a] = 0.5 * ((double)g.lo[a] + (double)g.hi[a]);
}

// One source point (px, py, pz) with weight w under the similarity x against the grid: acc[0 .. fit_terms(MODE)) += its
// terms, *used += 1, when the moved point is finite and dist2 <= md2 (float32; +inf: every finite point).
// MODE plane works with the UNNORMALISED float64 normal N = (b - a) x (c - a) of the winning face and the factor
// g = w / (N . N): g (J J^T) and g (J R) with J = [p x N, N, p . N], R = N . (q - p) are what the unit normal gives, without
// a square root.  N . N == 0 (a face without area): N = p - q; still 0 (the point lies on it): the point adds W and d^2 only.
template <int MODE>
R3G_MD_HD void fit_point(const Grid& g, const Tri* tris, const uint32_t* starts, const int32_t* pairs, const Sim& x, float px,
                         float py, float pz, float w32, float md2, double* acc, uint32_t* used, uint32_t* ntests) {
    float mx, my, mz, d2;
    int32_t face;
    uint32_t nt = 0;
    sim_apply(x, px, py, pz, &mx, &my, &mz);
    nearest(g, tris, starts, pairs, mx, my, mz, &d2, &face, &nt);
    *ntests += nt;
    if (face < 0 || !(d2 <= md2)) return;
    const Tri t = tris[face];
    float qx, qy, qz;
    tri_closest(mx, my, mz, t, &qx, &qy, &qz);
    double c[3];
    fit_centre(g, c);
    const double w = (double)w32;
    const double p[3] = {(double)mx - c[0], (double)my - c[1], (double)mz - c[2]};
    const double q[3] = {(double)qx - c[0], (double)qy - c[1], (double)qz - c[2]};
    *used += 1u;
    if (MODE == kFitPoint) {
        const double wp[3] = {w * p[0], w * p[1], w * p[2]};
        acc[0] += w;
_Pragma("unroll")
        for (int a = 0; a < 3; ++a) acc[1 + a] += wp[a];
_Pragma("unroll")
        for (int a = 0; a < 3; ++a) acc[4 + a] += w * q[a];
_Pragma("unroll")
        for (int a = 0; a < 3; ++a)
_Pragma("unroll")
            for (int b = 0; b < 3; ++b) acc[7 + 3 * a + b] += wp[a] * q[b];
        acc[16] += wp[0] * p[0] + wp[1] * p[1] + wp[2] * p[2];
        acc[17] += w * (double)d2;
    } else {
        const double e1[3] = {(double)t.bx - (double)t.ax, (double)t.by - (double)t.ay, (double)t.bz - (double)t.az};
        const double e2[3] = {(double)t.cx - (double)t.ax, (double)t.cy - (double)t.ay, (double)t.cz - (double)t.az};
        double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        double nn = N[0] * N[0] + N[1] * N[1] + N[2] * N[2];
        if (!(nn > 0.0)) {
_Pragma("unroll")
            for (int a = 0; a < 3; ++a) N[a] = p[a] - q[a];
            nn = N[0] * N[0] + N[1] * N[1] + N[2] * N[2];
        }
        if (nn > 0.0) {
            const double gw = w / nn;
            const double J[7] = {p[1] * N[2] - p[2] * N[1], p[2] * N[0] - p[0] * N[2], p[0] * N[1] - p[1] * N[0], N[0], N[1], N[2],
                                 p[0] * N[0] + p[1] * N[1] + p[2] * N[2]};
            const double R = N[0] * (q[0] - p[0]) + N[1] * (q[1] - p[1]) + N[2] * (q[2] - p[2]);
            int k = 0;
_Pragma("unroll")
            for (int a = 0; a < 7; ++a) {
                const double gj = gw * J[a];
_Pragma("unroll")
                for (int b = a; b < 7; ++b) acc[k++] += gj * J[b];
                acc[28 + a] += gj * R;
            }
        }
        acc[35] += w;
        acc[36] += w * (double)d2;
    }
}

// The reduction order, stated on the host (the kernels do the same with shuffles and LDS): lane l of a wave holds v[l];
// the butterfly v[l] += v[l ^ d] for d = 32, 16, 8, 4, 2, 1 leaves the wave's sum in every lane (a + b is commutative, so
// all lanes hold the same bits); the four waves of a block are then added in index order, ((s0 + s1) + s2) + s3.
R3G_MD_HD double fit_tree256(const double* v) {
    double s[4];
    for (int wv = 0; wv < 4; ++wv) {
        double a[64], b[64];
        for (int l = 0; l < 64; ++l) a[l] = v[64 * wv + l];
        for (int d = 32; d >= 1; d >>= 1) {
            for (int l = 0; l < 64; ++l) b[l] = a[l] + a[l ^ d];
            for (int l = 0; l < 64; ++l) a[l] = b[l];
        }
        s[wv] = a[0];
    }
    return ((s[0] + s[1]) + s[2]) + s[3];
}

}  // namespace r3g_md
#endif
