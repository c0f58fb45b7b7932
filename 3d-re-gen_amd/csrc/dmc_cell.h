// dmc_cell.h -- per-cell logic of the dual-marching-cubes extractor (product code; definition: DESIGN.md section 4c).
//
// One vertex per surface patch of a cell, one quad (two triangles) per crossed grid edge with four cells around it.
// Parallel formulation: everything a quad needs hangs on the cell whose corner 0 is the edge's low end p (the edges
// 0, 4, 8 of that cell), and ascending (p, axis) is ascending (cell, axis); so vertices AND quads are numbered by one
// exclusive scan over the cells of {patch count, quad count}.
//
// Corner c = 4*d0 + 2*d1 + d2 (d = offsets on array axes 0, 1, 2), case = sum of (value > level) << c.
// Edge e = 4*a + 2*u + v: along axis a, low corner at offset u on axis (a+1)%3 and v on axis (a+2)%3.
//
// Shared by dmc_kernels.hip (device) and tests/emu (host emulation of the launch structure, test-only).
// Compile with -ffp-contract=off: positions and the diagonal test are fixed to the bit.
#ifndef R3G_DMC_CELL_H
#define R3G_DMC_CELL_H

#include <stdint.h>

#include "surf_common.h"   // R3G_DEV default, range flags, Xform, store_vertex
#include "dmc_luts.h"

#if defined(__clang__)
#define R3G_DMC_UNROLL _Pragma("unroll")
#else
#define R3G_DMC_UNROLL
#endif

#define R3G_DMC_FLAG_LE R3G_SURF_FLAG_LE    // some sample <= level
#define R3G_DMC_FLAG_GE R3G_SURF_FLAG_GE    // some sample >= level
#define R3G_DMC_FLAG_NAN R3G_SURF_FLAG_NAN  // some sample is NaN

namespace r3g_dmc {

struct Dims {
    int n0, n1, n2;  // nodes per axis
};

// what the vertex pass leaves for the quad pass; only active cells are ever written or read
struct CellRef {
    uint32_t vbase;  // id of the cell's first vertex
    uint32_t ecase;  // effective case (the complemented one where the manifold rule applies)
};

// output transform, as r3g_mc_emit (surf_common.h); positions are already in output-column order
using r3g_surf::Xform;
using r3g_surf::store_vertex;

R3G_DEV int lut_patch(uint64_t w, int e) { return (int)((w >> (4 * e)) & 0xFu); }
R3G_DEV int lut_count(uint64_t w) { return (int)((w >> 48) & 0x7u); }
R3G_DEV int lut_tunnel(uint64_t w) { return (int)((w >> 52) & 0x7u); }

R3G_DEV void load_cell(const float* g, const Dims& d, int i, int j, int k, float* f) {
    const int64_t s1 = d.n2, s0 = (int64_t)d.n1 * d.n2;
    const float* p = g + (int64_t)i * s0 + (int64_t)j * s1 + k;
    f[0] = p[0]; f[1] = p[1]; f[2] = p[s1]; f[3] = p[s1 + 1];
    f[4] = p[s0]; f[5] = p[s0 + 1]; f[6] = p[s0 + s1]; f[7] = p[s0 + s1 + 1];
}

// case of cell (i,j,k); *flags gathers the range flags of its 8 samples
R3G_DEV int cell_case(const float* g, const Dims& d, int i, int j, int k, double level, unsigned* flags) {
    float f[8];
    load_cell(g, d, i, j, k, f);
    int cs = 0;
    unsigned fl = 0;
    R3G_DMC_UNROLL
    for (int c = 0; c < 8; ++c) {
        const double v = (double)f[c];
        if (v > level) cs |= 1 << c;
        if (v <= level) fl |= R3G_DMC_FLAG_LE;
        if (v >= level) fl |= R3G_DMC_FLAG_GE;
        if (v != v) fl |= R3G_DMC_FLAG_NAN;
    }
    *flags |= fl;
    return cs;
}

// Manifold rule: a case that tunnels through face f takes its complement's patches when the cell across f tunnels
// through the same face.  The neighbour's case is recomputed from the grid (tunnelling cells are rare).
R3G_DEV int effective_case(const float* g, const Dims& d, int i, int j, int k, double level, int cs, bool manifold) {
    const int tf = lut_tunnel(R3G_DMC_CASE[cs]);
    if (!manifold || tf == 7) return cs;
    const int ax = tf >> 1, step = (tf & 1) ? 1 : -1;
    int ni = i, nj = j, nk = k;
    if (ax == 0) ni += step; else if (ax == 1) nj += step; else nk += step;
    if (ni < 0 || nj < 0 || nk < 0 || ni > d.n0 - 2 || nj > d.n1 - 2 || nk > d.n2 - 2) return cs;
    unsigned ignored = 0;
    const int ncs = cell_case(g, d, ni, nj, nk, level, &ignored);
    return lut_tunnel(R3G_DMC_CASE[ncs]) == (tf ^ 1) ? (cs ^ 255) : cs;
}

// Pass 1 record of an active cell, 0 for an inactive one:
//   bits 0..7 effective case, 8..10 which of the edges 0/4/8 (axis 0/1/2 from corner 0) carry a quad,
//   11 corner 0 inside, 12..14 patch count, 16..17 quad count, 31 set.
R3G_DEV unsigned classify_cell(const float* g, const Dims& d, int i, int j, int k, double level, int cs, bool manifold) {
    if (cs == 0 || cs == 255) return 0u;
    const int ec = effective_case(g, d, i, j, k, level, cs, manifold);
    unsigned qmask = 0;
    // crossed: corner 0 against corner 4 / 2 / 1; four cells around the edge: both other coordinates >= 1
    if (((cs ^ (cs >> 4)) & 1) && j >= 1 && k >= 1) qmask |= 1u;
    if (((cs ^ (cs >> 2)) & 1) && k >= 1 && i >= 1) qmask |= 2u;
    if (((cs ^ (cs >> 1)) & 1) && i >= 1 && j >= 1) qmask |= 4u;
    const unsigned nq = (qmask & 1u) + ((qmask >> 1) & 1u) + (qmask >> 2);
    return (unsigned)ec | (qmask << 8) | ((unsigned)(cs & 1) << 11) | ((unsigned)lut_count(R3G_DMC_CASE[ec]) << 12) |
           (nq << 16) | 0x80000000u;
}
R3G_DEV unsigned rec_patches(unsigned rec) { return (rec >> 12) & 0x7u; }
R3G_DEV unsigned rec_quads(unsigned rec) { return (rec >> 16) & 0x3u; }

// Pass 3: the vertices of one active cell, and its entry in the cell table.  Per patch: the crossing points of its
// edges in ascending edge number, summed in double, divided by their number, rounded once.  Loops over the edges are
// unrolled so that corner values and crossing parameters are indexed statically (registers, no scratch).
R3G_DEV void emit_cell_vertices(unsigned rec, uint32_t vbase, const float* g, const Dims& d, int i, int j, int k,
                                double level, int64_t cell, CellRef* ctab, float* verts, const Xform& xf, bool use_xf) {
    const int ec = (int)(rec & 0xFFu);
    const uint64_t w = R3G_DMC_CASE[ec];
    const int np = lut_count(w);
    CellRef ref;
    ref.vbase = vbase;
    ref.ecase = (uint32_t)ec;
    ctab[cell] = ref;
    float f[8];
    load_cell(g, d, i, j, k, f);
    double t[12];
    R3G_DMC_UNROLL
    for (int e = 0; e < 12; ++e) {
        const int a = e >> 2, u = (e >> 1) & 1, v = e & 1;
        const int lo = (a == 0 ? 2 * u + v : a == 1 ? u + 4 * v : 4 * u + 2 * v), hi = lo + (4 >> a);
        const double va = (double)f[lo], vb = (double)f[hi];
        t[e] = (level - va) / (vb - va);
    }
    for (int p = 0; p < np; ++p) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        int n = 0;
        R3G_DMC_UNROLL
        for (int e = 0; e < 12; ++e) {
            if (lut_patch(w, e) != p) continue;
            const int a = e >> 2, u = (e >> 1) & 1, v = e & 1;
            // offsets of the low corner on array axes 0, 1, 2
            const int d0 = a == 1 ? v : a == 2 ? u : 0, d1 = a == 0 ? u : a == 2 ? v : 0, d2 = a == 0 ? v : a == 1 ? u : 0;
            double p0 = (double)(i + d0), p1 = (double)(j + d1), p2 = (double)(k + d2);
            if (a == 0) p0 = p0 + t[e]; else if (a == 1) p1 = p1 + t[e]; else p2 = p2 + t[e];
            s0 = s0 + p0; s1 = s1 + p1; s2 = s2 + p2;
            ++n;
        }
        const double dn = (double)n;
        store_vertex(verts + 3 * ((int64_t)vbase + p), s0 / dn, s1 / dn, s2 / dn, xf, use_xf);
    }
}

R3G_DEV float dist2(const float* a, const float* b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}

// Pass 4: the quads of one active cell (grid edges from its corner 0), each as two triangles at faces[6*(qbase+rank)].
// The diagonal test reads the float32 positions pass 3 stored.
R3G_DEV void emit_cell_quads(unsigned rec, uint32_t qbase, const Dims& d, int i, int j, int k, const CellRef* ctab,
                             const float* verts, int32_t* faces, bool reversed) {
    const unsigned qmask = (rec >> 8) & 0x7u;
    const bool inside = (rec >> 11) & 1u;
    const int64_t c1 = d.n1 - 1, c2 = d.n2 - 1;
    uint32_t rank = 0;
    R3G_DMC_UNROLL
    for (int a = 0; a < 3; ++a) {
        if (!((qmask >> a) & 1u)) continue;
        const int u = (a + 1) % 3, v = (a + 2) % 3;
        const int DU[4] = {-1, 0, 0, -1}, DV[4] = {-1, -1, 0, 0};
        int32_t q[4];
        R3G_DMC_UNROLL
        for (int m = 0; m < 4; ++m) {
            const int o0 = (u == 0 ? DU[m] : 0) + (v == 0 ? DV[m] : 0), o1 = (u == 1 ? DU[m] : 0) + (v == 1 ? DV[m] : 0),
                      o2 = (u == 2 ? DU[m] : 0) + (v == 2 ? DV[m] : 0);
            const CellRef r = ctab[((int64_t)(i + o0) * c1 + (j + o1)) * c2 + (k + o2)];
            q[m] = (int32_t)(r.vbase + (uint32_t)lut_patch(R3G_DMC_CASE[r.ecase & 0xFFu], 4 * a - 2 * DU[m] - DV[m]));
        }
        if (!inside) {
            int32_t x = q[0]; q[0] = q[3]; q[3] = x;
            x = q[1]; q[1] = q[2]; q[2] = x;
        }
        float P[4][3];
        R3G_DMC_UNROLL
        for (int m = 0; m < 4; ++m) {
            const float* s = verts + 3 * (int64_t)q[m];
            P[m][0] = s[0]; P[m][1] = s[1]; P[m][2] = s[2];
        }
        int32_t tri[6];
        if (dist2(P[1], P[3]) < dist2(P[0], P[2])) {
            tri[0] = q[1]; tri[1] = q[2]; tri[2] = q[3]; tri[3] = q[1]; tri[4] = q[3]; tri[5] = q[0];
        } else {
            tri[0] = q[0]; tri[1] = q[1]; tri[2] = q[2]; tri[3] = q[0]; tri[4] = q[2]; tri[5] = q[3];
        }
        int32_t* dst = faces + 6 * ((int64_t)qbase + rank);
        if (reversed) {
            dst[0] = tri[2]; dst[1] = tri[1]; dst[2] = tri[0]; dst[3] = tri[5]; dst[4] = tri[4]; dst[5] = tri[3];
        } else {
            R3G_DMC_UNROLL
            for (int m = 0; m < 6; ++m) dst[m] = tri[m];
        }
        ++rank;
    }
}

}  // namespace r3g_dmc
#endif
