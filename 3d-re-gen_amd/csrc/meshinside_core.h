// meshinside_core.h -- per-element bodies of the point-in-mesh query (ray-crossing count with a watertight tie rule).
//
// The contract: crossings(p, mesh, axis) = the number of usable faces the ray from p in the +axis
// direction crosses; a point is inside when the count is odd.  `crossed` below IS the definition: float64 arithmetic on the
// float32 inputs, every difference and product one operation, evaluated without contraction (-ffp-contract=off on both
// sides), so the host instantiation (tests/emu/meshinside_emu.cpp), the kernels (meshinside_kernels.hip) and the numpy
// restatement (tests/meshinside_ref.py) give identical counts.  The grid of columns only prunes: a face is listed in every
// column its projected box overlaps, and a face can only be crossed by a point inside that box.
#ifndef R3G_MESHINSIDE_CORE_H
#define R3G_MESHINSIDE_CORE_H
#include <stdint.h>

#include "grid_csr.h"

#ifndef R3G_MI_HD
#define R3G_MI_HD static inline
#endif

namespace r3g_mi {

using r3g_grid::clamp;
using r3g_grid::coord;
using r3g_grid::dec_float;
using r3g_grid::enc_float;
using r3g_grid::finite;
using r3g_grid::fmax2;
using r3g_grid::fmin2;
using r3g_grid::kPairMult;
using r3g_grid::make_grid;
using Grid2 = r3g_grid::GridN<2>;      // columns (section 4g): the grid of grid_csr.h over the two projected axes

constexpr int kMaxRes = 1024;                         // cap: 1024^2 = 2^20 columns
constexpr float kInf = __builtin_huge_valf();

// one face in projected coordinates (u, v) = (x[(axis+1)%3], x[(axis+2)%3]), depth w = x[axis], with its vertex indices
// (the last tie-break of the canonical edge direction); 48 bytes: three 16-byte loads.  ia < 0: not usable.
struct alignas(16) Rec {
    float au, av, aw;
    int32_t ia;
    float bu, bv, bw;
    int32_t ib;
    float cu, cv, cw;
    int32_t ic;
};

R3G_MI_HD Rec make_rec(const float a[3], int32_t ia, const float b[3], int32_t ib, const float c[3], int32_t ic, int axis) {
    const int iu = (axis + 1) % 3, iv = (axis + 2) % 3;
    Rec r;
    r.au = a[iu], r.av = a[iv], r.aw = a[axis], r.ia = ia;
    r.bu = b[iu], r.bv = b[iv], r.bw = b[axis], r.ib = ib;
    r.cu = c[iu], r.cv = c[iv], r.cw = c[axis], r.ic = ic;
    return r;
}

R3G_MI_HD bool rec_finite(const Rec& r) {
    return finite(r.au) && finite(r.av) && finite(r.aw) && finite(r.bu) && finite(r.bv) && finite(r.bw) && finite(r.cu) &&
           finite(r.cv) && finite(r.cw);
}

// true when P comes before Q in the lexicographic order on (u, v, w), the vertex index last: P -> Q is the canonical direction
R3G_MI_HD bool before(float pu, float pv, float pw, int32_t pi, float qu, float qv, float qw, int32_t qi) {
    if (pu != qu) return pu < qu;
    if (pv != qv) return pv < qv;
    if (pw != qw) return pw < qw;
    return pi < qi;
}

// E(x) of the canonical edge U -> V: each difference and product one float64 operation
R3G_MI_HD double edge_fn(double Uu, double Uv, double Vu, double Vv, double xu, double xv) {
    const double du = Vu - Uu, dv = Vv - Uv;
    const double xdv = xv - Uv, xdu = xu - Uu;
    const double t1 = du * xdv, t2 = dv * xdu;
    return t1 - t2;
}

// the edge P -> Q of a face (its own vertex order), the opposite vertex O and a point x
struct EdgeEval {
    double ex;        // E(x) along the canonical direction
    double eo;        // E(O) along the canonical direction
    bool flip;        // the face traverses the edge against its canonical direction
};

R3G_MI_HD EdgeEval eval_edge(float pu, float pv, float pw, int32_t pi, float qu, float qv, float qw, int32_t qi, float ou, float ov,
                             float xu, float xv) {
    EdgeEval e;
    e.flip = !before(pu, pv, pw, pi, qu, qv, qw, qi);
    const double Uu = e.flip ? qu : pu, Uv = e.flip ? qv : pv, Vu = e.flip ? pu : qu, Vv = e.flip ? pv : qv;
    e.ex = edge_fn(Uu, Uv, Vu, Vv, xu, xv);
    e.eo = edge_fn(Uu, Uv, Vu, Vv, ou, ov);
    return e;
}

// a face is usable when, for each of its edges, E of the opposite vertex is nonzero (the vertices are finite here)
R3G_MI_HD bool rec_usable(const Rec& r) {
    const EdgeEval ab = eval_edge(r.au, r.av, r.aw, r.ia, r.bu, r.bv, r.bw, r.ib, r.cu, r.cv, r.cu, r.cv);
    const EdgeEval bc = eval_edge(r.bu, r.bv, r.bw, r.ib, r.cu, r.cv, r.cw, r.ic, r.au, r.av, r.au, r.av);
    const EdgeEval ca = eval_edge(r.cu, r.cv, r.cw, r.ic, r.au, r.av, r.aw, r.ia, r.bu, r.bv, r.bu, r.bv);
    return ab.eo != 0.0 && bc.eo != 0.0 && ca.eo != 0.0;
}

// does the ray from (pu, pv, pw) in the +w direction cross the usable face r?
R3G_MI_HD bool crossed(float pu, float pv, float pw, const Rec& r) {
    // covered, part 1: the closed float32 bounding box of the projected vertices
    if (pu < fmin2(r.au, fmin2(r.bu, r.cu)) || pu > fmax2(r.au, fmax2(r.bu, r.cu))) return false;
    if (pv < fmin2(r.av, fmin2(r.bv, r.cv)) || pv > fmax2(r.av, fmax2(r.bv, r.cv))) return false;
    // covered, part 2: on every edge p lies on the side of the opposite vertex; E == 0 counts as +1
    const EdgeEval ab = eval_edge(r.au, r.av, r.aw, r.ia, r.bu, r.bv, r.bw, r.ib, r.cu, r.cv, pu, pv);
    if ((ab.ex >= 0.0) != (ab.eo > 0.0)) return false;
    const EdgeEval bc = eval_edge(r.bu, r.bv, r.bw, r.ib, r.cu, r.cv, r.cw, r.ic, r.au, r.av, pu, pv);
    if ((bc.ex >= 0.0) != (bc.eo > 0.0)) return false;
    const EdgeEval ca = eval_edge(r.cu, r.cv, r.cw, r.ic, r.au, r.av, r.aw, r.ia, r.bu, r.bv, pu, pv);
    if ((ca.ex >= 0.0) != (ca.eo > 0.0)) return false;
    // above: the edge values along the face's own vertex order; no division, strict comparisons
    const double D = ab.flip ? -ab.eo : ab.eo;
    const double eab = ab.flip ? -ab.ex : ab.ex, ebc = bc.flip ? -bc.ex : bc.ex, eca = ca.flip ? -ca.ex : ca.ex;
    const double n1 = ebc * (double)r.aw, n2 = eca * (double)r.bw, n3 = eab * (double)r.cw;
    const double n12 = n1 + n2;
    const double N = n12 + n3;
    const double pd = (double)pw * D;
    return D > 0.0 ? N > pd : N < pd;
}

// first resolution tried for F faces: R = floor(sqrt(F)) columns per axis leaves a few faces in an occupied column
R3G_MI_HD int initial_resolution(int64_t nf) {
    int r = 1;
    while (r < kMaxRes && (int64_t)(r + 1) * (r + 1) <= nf) ++r;
    return r;
}

// what the grid builder asks of a record (grid_csr.h): does it take part, and its projected box
R3G_MI_HD bool grid_member(const Rec& r) { return r.ia >= 0; }
R3G_MI_HD void grid_box(const Rec& r, float mn[2], float mx[2]) {
    mn[0] = fmin2(r.au, fmin2(r.bu, r.cu)), mn[1] = fmin2(r.av, fmin2(r.bv, r.cv));
    mx[0] = fmax2(r.au, fmax2(r.bu, r.cu)), mx[1] = fmax2(r.av, fmax2(r.bv, r.cv));
}

// the grid helpers under the names of this header's interface: a face's column range, its pair count, a column's index
R3G_MI_HD void rec_range(const Grid2& g, const Rec& r, int lo[2], int hi[2]) { r3g_grid::range(g, r, lo, hi); }
R3G_MI_HD int64_t rec_pairs(const Grid2& g, const Rec& r) { return r3g_grid::pairs(g, r); }
R3G_MI_HD int col_index(const Grid2& g, int x, int y) {
    const int c[2] = {x, y};
    return r3g_grid::index(g, c);
}

// The query of one point given in mesh coordinates: project, find the column, sum the crossings of the faces listed there.
// A face that p is covered by holds p inside its projected box, so (the grid's coord is monotone) p's column lies inside the
// face's column range: every face that can be crossed is listed in p's column.
R3G_MI_HD int32_t count_crossings(const Grid2& g, int axis, const Rec* recs, const uint32_t* starts, const int32_t* pairs, float px,
                                  float py, float pz, uint32_t* ntests_out) {
    if (!(finite(px) && finite(py) && finite(pz))) return -1;
    const float p[3] = {px, py, pz};
    const float pu = p[(axis + 1) % 3], pv = p[(axis + 2) % 3], pw = p[axis];
    if (pu < g.lo[0] || pu > g.hi[0] || pv < g.lo[1] || pv > g.hi[1]) return 0;     // outside the projected box: no lookup
    const int col = col_index(g, clamp(coord(g, 0, pu), g.res), clamp(coord(g, 1, pv), g.res));
    const uint32_t e = starts[col + 1];
    int32_t n = 0;
    uint32_t ntests = 0;
    for (uint32_t k = starts[col]; k < e; ++k) {
        n += crossed(pu, pv, pw, recs[pairs[k]]) ? 1 : 0;
        ++ntests;
    }
    if (ntests_out) *ntests_out = ntests;
    return n;
}

}  // namespace r3g_mi
#endif
