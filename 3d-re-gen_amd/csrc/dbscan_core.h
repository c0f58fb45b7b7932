// dbscan_core.h -- per-element bodies of DBSCAN on a point cloud: the neighbour predicate, the radius
// walk over the uniform grid of section 4k, and the visitors of the count, link and border passes.
//
// The contract: q is a neighbour of p iff d2 = ((dx*dx) + dy*dy) + dz*dz <= eps*eps, every coordinate widened to float64
// first, one rounding per operation, left to right, without contraction (-ffp-contract=off on both sides); eps*eps is computed
// once in float64.  A point is its own neighbour; equal coordinates under distinct indices are distinct neighbours.  The host
// instantiation (tests/emu/dbscan_emu.cpp) and the kernels (dbscan_kernels.hip) run this one source.  Every output is an
// integer, so both give identical bits.  The grid only prunes: the walk visits the box of cells that can hold a neighbour,
// every cell at most once, and every usable point is listed in exactly one cell, so a neighbour is met exactly once and the
// result depends neither on the resolution nor on the order of the points inside a cell.
#ifndef R3G_DBSCAN_CORE_H
#define R3G_DBSCAN_CORE_H
#include <stdint.h>

#include "cloud_core.h"

#ifndef R3G_DB_HD
#define R3G_DB_HD static inline
#endif
#ifndef R3G_DB_HD_MEMBER
#define R3G_DB_HD_MEMBER inline
#endif

namespace r3g_db {

using r3g_cl::Grid;
using r3g_cl::Pt;
using r3g_grid::clamp;
using r3g_grid::coord;
using r3g_grid::kBinMargin;

constexpr int kReport = 8;                // n_usable, n_core, n_border, n_noise, n_clusters, largest, largest_size, resolution
constexpr int kCellsPerPoint = 8;         // the automatic resolution never makes more cells than this per usable point
constexpr double kReach = 1.0 + 1.0 / 1099511627776.0;      // 1 + 2^-40: the walk's radius over eps (absorbs the rounding of d2)

// THE definition
R3G_DB_HD bool neighbour(const Pt& p, const Pt& q, double eps2) {
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
    const double d2 = ((dx * dx) + dy * dy) + dz * dz;
    return d2 <= eps2;
}

// the float32 next to x on the side named: float_up(x) >= x >= float_down(x), by one step from the nearest float32
R3G_DB_HD float float_step(float f, bool up) {
    union { float f; uint32_t u; } c;
    c.f = f;
    if (f == 0.0f) c.u = up ? 0x00000001u : 0x80000001u;
    else if ((f > 0.0f) == up) c.u += 1;
    else c.u -= 1;
    return c.f;
}
R3G_DB_HD float float_up(double x) {
    const float f = (float)x;
    return (double)f < x ? float_step(f, true) : f;
}
R3G_DB_HD float float_down(double x) {
    const float f = (float)x;
    return (double)f > x ? float_step(f, false) : f;
}

// automatic resolution for a radius search: cells of side about eps along the longest axis of the box of the usable points,
// res = floor(extent / eps), at least 1, at most kMaxRes, and at most the largest res with res^3 <= kCellsPerPoint * n_usable
// (a sparse cloud in a large box would otherwise pay for 2^24 mostly empty cells)
R3G_DB_HD int auto_resolution(const float* lo, const float* hi, double eps, int64_t n_usable) {
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double e = (double)hi[a] - (double)lo[a];
        ext = e > ext ? e : ext;
    }
    const int cap = r3g_cl::auto_resolution(n_usable * kCellsPerPoint, 1);
    const double r = ext / eps;
    if (!(r >= 1.0)) return 1;
    return r >= (double)cap ? cap : (int)r;
}
// the most cells per axis that the automatic rule can choose for n points, whatever their box
R3G_DB_HD int auto_resolution_most(int64_t n) { return r3g_cl::auto_resolution(n * kCellsPerPoint, 1); }

// The radius walk of one usable point p: visit(q) for every neighbour q of p, itself included, until visit returns false.
// pts: the points in cell order (starts[cells + 1]).  -> the number of predicate evaluations.
// A neighbour q has |p.x - q.x| <= eps * kReach in real numbers (kReach covers the roundings of d2), so q.x <= up :=
// float_up(p.x + eps * kReach): q.x is a float32 and both roundings are monotone.  coord() and clamp() are monotone too, so
// q's home cell clamp(coord(q.x)) is at most clamp(coord(up)); the same from below.  The bounds are pulled outward by
// kBinMargin cells on top of that, as section 4k does.  Axis 0 is the fastest in a cell's index, so a row of the box is
// one run of records.
template <class V>
R3G_DB_HD uint32_t radius_walk(const Grid& g, const Pt* pts, const uint32_t* starts, const Pt& p, double eps, double eps2, V& visit) {
    const float pc[3] = {p.x, p.y, p.z};
    const double reach = eps * kReach;
    int lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = clamp(coord(g, a, float_down((double)pc[a] - reach)) - kBinMargin, g.res);
        hi[a] = clamp(coord(g, a, float_up((double)pc[a] + reach)) + kBinMargin, g.res);
    }
    uint32_t tests = 0;
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y) {
            const int c0[3] = {lo[0], y, z};
            const int row = r3g_grid::index(g, c0);
            const uint32_t e = starts[row + (hi[0] - lo[0]) + 1];
            for (uint32_t k = starts[row]; k < e; ++k) {
                const Pt q = pts[k];
                ++tests;
                if (neighbour(p, q, eps2) && !visit(q)) return tests;
            }
        }
    return tests;
}

// count pass: the neighbours of p, itself included; stops at `limit` (0xffffffff: never)
struct CountVisitor {
    uint32_t count, limit;
    R3G_DB_HD_MEMBER bool operator()(const Pt&) { return ++count < limit; }
};

// link pass of a core point `self`: unite(self, j) for every core neighbour j of smaller index
template <class Unite>
struct LinkVisitor {
    const uint8_t* core;
    int32_t self;
    Unite& unite;
    R3G_DB_HD_MEMBER bool operator()(const Pt& q) {
        if (q.index < self && core[q.index]) unite(self, q.index);
        return true;
    }
};

// border pass of a non-core point: the smallest root over its core neighbours (root[]: flattened), kNoIndex without one
struct BorderVisitor {
    const uint8_t* core;
    const int32_t* root;
    int32_t best;
    R3G_DB_HD_MEMBER bool operator()(const Pt& q) {
        if (core[q.index]) {
            const int32_t r = root[q.index];
            best = r < best ? r : best;
        }
        return true;
    }
};

// a cluster's root is the core point that is its own parent
R3G_DB_HD uint32_t root_flag(const int32_t* root, int64_t i) { return root[i] == (int32_t)i ? 1u : 0u; }
// root[i] < 0: noise or unusable; number[]: the exclusive scan of root_flag
R3G_DB_HD int32_t label_of(const int32_t* root, const uint32_t* number, int64_t i) {
    const int32_t r = root[i];
    return r < 0 ? -1 : (int32_t)number[r];
}

// the arg-max over clusters by one integer max: most points first, then the lowest number
R3G_DB_HD uint64_t pack_best(uint32_t size, int32_t label) { return ((uint64_t)size << 32) | (uint32_t)~(uint32_t)label; }
R3G_DB_HD int32_t best_label(uint64_t packed) { return (packed >> 32) ? (int32_t)~(uint32_t)packed : -1; }
R3G_DB_HD int64_t best_size(uint64_t packed) { return (int64_t)(packed >> 32); }

}  // namespace r3g_db
#endif
