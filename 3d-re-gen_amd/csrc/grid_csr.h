// grid_csr.h -- the uniform grid in CSR form that the mesh distance (D = 3) and the point-in-mesh
// columns (D = 2, section 4g) share: starts[cells + 1] plus a pair list, every record listed in each cell its box overlaps.
//
// Host and device instantiate this one source (R3G_GRID_HD, as the *_core.h files do), so a host twin and the kernels list
// the same records in the same cells.  What the exactness of both users rests on lives here: a record's cell range is
// computed from monotone float32 operations and widened by kBinMargin, so rounding can only add cells; starts[] carries
// one element more than there are cells, which receives the total; and the order of the records inside a cell is left open
// (integer atomics decide it on the device), so a user must not depend on it.
//
// A record type R takes part through two functions found by argument-dependent lookup:
//   bool grid_member(const R&)                        does the record take part at all?
//   void grid_box(const R&, float mn[D], float mx[D])  its box on the grid axes
#ifndef R3G_GRID_CSR_H
#define R3G_GRID_CSR_H
#include <stdint.h>

#ifndef R3G_GRID_HD
#define R3G_GRID_HD static inline
#endif

namespace r3g_grid {

constexpr int kPairMult = 8;                          // automatic resolution: halve while pairs > kPairMult * F
constexpr float kBinMargin = 1.0f / 256.0f;           // cells; widens a record's cell range (rounding can only add cells)

template <int D>
struct GridN {
    float lo[D];
    float hi[D];
    float h[D];          // cell size per axis
    float inv[D];        // 1 / h: defines the cell coordinate t = (x - lo) * inv
    int res;             // cells per axis
};

R3G_GRID_HD bool finite(float x) { return (x - x) == 0.0f; }
R3G_GRID_HD float fmin2(float a, float b) { return b < a ? b : a; }
R3G_GRID_HD float fmax2(float a, float b) { return b > a ? b : a; }

// order-preserving float -> uint32 (bounding box by integer atomicMin / atomicMax) and back
R3G_GRID_HD uint32_t enc_float(float x) {
    union { float f; uint32_t u; } c;
    c.f = x;
    return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
R3G_GRID_HD float dec_float(uint32_t u) {
    union { float f; uint32_t u; } c;
    c.u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return c.f;
}

template <int D>
R3G_GRID_HD GridN<D> make_grid(const float (&lo)[D], const float (&hi)[D], int res) {
    GridN<D> g;
    g.res = res;
    float ext[D], maxext = 0.0f;
    for (int a = 0; a < D; ++a) {
        g.lo[a] = lo[a];
        g.hi[a] = hi[a];
        ext[a] = hi[a] - lo[a];
        maxext = fmax2(maxext, ext[a]);
    }
    for (int a = 0; a < D; ++a) {
        float h = ext[a] / (float)res;
        if (!(h >= 1e-30f && h <= 1e30f)) h = maxext / (float)res;     // a flat axis: every record lands in its cell 0
        if (!(h >= 1e-30f && h <= 1e30f)) h = 1.0f;
        g.h[a] = h;
        g.inv[a] = 1.0f / h;
    }
    return g;
}

// res^D
template <int D>
constexpr R3G_GRID_HD int64_t cells(int res) {
    int64_t n = 1;
    for (int a = 0; a < D; ++a) n *= res;
    return n;
}

// monotone in x: subtraction of a constant and multiplication by a positive constant round monotonically
template <int D>
R3G_GRID_HD float coord(const GridN<D>& g, int a, float x) { return (x - g.lo[a]) * g.inv[a]; }

// floor(t) clamped to [0, res - 1]; NaN -> 0
R3G_GRID_HD int clamp(float t, int res) {
    if (!(t > 0.0f)) return 0;
    if (t >= (float)res) return res - 1;
    return (int)t;
}

// the cells a record's box overlaps, widened by kBinMargin on both sides
template <int D, class R>
R3G_GRID_HD void range(const GridN<D>& g, const R& r, int* lo, int* hi) {
    float mn[D], mx[D];
    grid_box(r, mn, mx);
    for (int a = 0; a < D; ++a) {
        lo[a] = clamp(coord(g, a, mn[a]) - kBinMargin, g.res);
        hi[a] = clamp(coord(g, a, mx[a]) + kBinMargin, g.res);
    }
}

template <int D, class R>
R3G_GRID_HD int64_t pairs(const GridN<D>& g, const R& r) {
    int lo[D], hi[D];
    range(g, r, lo, hi);
    int64_t n = hi[0] - lo[0] + 1;
    for (int a = 1; a < D; ++a) n *= hi[a] - lo[a] + 1;
    return n;
}

// the cell with coordinates c[0 .. D), axis 0 fastest
template <int D>
R3G_GRID_HD int index(const GridN<D>& g, const int* c) {
    int i = c[D - 1];
    for (int a = D - 2; a >= 0; --a) i = i * g.res + c[a];
    return i;
}

// fn(cell) for every cell of a record's range, axis 0 fastest (D = 2: the z loop runs once)
template <int D, class R, class Fn>
R3G_GRID_HD void for_each_cell(const GridN<D>& g, const R& r, Fn fn) {
    static_assert(D == 2 || D == 3, "columns or cells");
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    range(g, r, lo, hi);
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
                const int c[3] = {x, y, z};
                fn(index(g, c));
            }
}

// The resolution rule: `forced`, or halve from `initial` while the structure would list more than kPairMult pairs a record
// (e.g. one triangle that spans the box has res^D pairs of its own).  count(g, &pairs) -> 0 or an error, which ends the search.
template <int D, class Count>
static inline int choose_resolution(const float (&lo)[D], const float (&hi)[D], int forced, int initial, int64_t nf, Count count, GridN<D>* g,
                                    int64_t* npairs) {
    int res = forced ? forced : initial;
    for (;;) {
        *g = make_grid(lo, hi, res);
        const int rc = count(*g, npairs);
        if (rc) return rc;
        if (forced || res == 1 || *npairs <= kPairMult * nf) return 0;
        res /= 2;
    }
}

// ---- the build as host loops (the twins under tests/emu) ------------------------------------------------------------------
template <int D, class R>
static inline int64_t host_pairs(const GridN<D>& g, const R* recs, int64_t nf) {
    int64_t n = 0;
    for (int64_t k = 0; k < nf; ++k)
        if (grid_member(recs[k])) n += pairs(g, recs[k]);
    return n;
}

// count pass, prefix sum, fill pass.  starts [cells + 1] and cursor [cells] arrive zeroed; list holds host_pairs() entries.
// `reverse_fill` fills in the opposite record order: the order inside a cell must not matter.
template <int D, class R>
static inline void host_fill(const GridN<D>& g, const R* recs, int64_t nf, bool reverse_fill, uint32_t* starts, uint32_t* cursor,
                             int32_t* list) {
    for (int64_t k = 0; k < nf; ++k)
        if (grid_member(recs[k])) for_each_cell(g, recs[k], [&](int cell) { ++starts[cell + 1]; });
    for (int64_t c = 0, n = cells<D>(g.res); c < n; ++c) starts[c + 1] += starts[c];
    for (int64_t kk = 0; kk < nf; ++kk) {
        const int64_t k = reverse_fill ? nf - 1 - kk : kk;
        if (grid_member(recs[k])) for_each_cell(g, recs[k], [&](int cell) { list[starts[cell] + cursor[cell]++] = (int32_t)k; });
    }
}

// ---- records with one home cell each (the point clouds of section 4k) -------------------------------------------------------
// A record type R with a third function
//   int grid_home(const GridN<D>&, const R&)          the one cell that lists the record
// is listed exactly once, without the kBinMargin widening, and the build moves the records themselves into cell order:
// sorted[starts[cell] .. starts[cell + 1]) are cell's records.  Same arrays and the same open order inside a cell as above.
template <int D, class R>
static inline void host_fill_home(const GridN<D>& g, const R* recs, int64_t n, bool reverse_fill, uint32_t* starts, uint32_t* cursor,
                                  R* sorted) {
    for (int64_t k = 0; k < n; ++k)
        if (grid_member(recs[k])) ++starts[grid_home(g, recs[k]) + 1];
    for (int64_t c = 0, nc = cells<D>(g.res); c < nc; ++c) starts[c + 1] += starts[c];
    for (int64_t kk = 0; kk < n; ++kk) {
        const int64_t k = reverse_fill ? n - 1 - kk : kk;
        if (!grid_member(recs[k])) continue;
        const int cell = grid_home(g, recs[k]);
        sorted[starts[cell] + cursor[cell]++] = recs[k];
    }
}

}  // namespace r3g_grid
#endif
