// recon_core.h -- per-element bodies of the Poisson surface on a uniform lattice: the splat of oriented
// points into int64 fixed-point channels, the divergence, the stencil passes of the geometric multigrid and the trilinear
// sample.  Compiled for the device (recon_kernels.hip) and for the host (tests/emu/recon_emu.cpp), both without contraction:
// every float32 operation below is written out, one rounding each, in the order it stands.  Every value is a pure function
// of its inputs or an integer sum, so the two sides agree bit for bit whatever the order in which lanes run.
//
// Lattice: n = 2^depth + 1 nodes per axis, node (i0, i1, i2) at lo + h * i, stored [i0][i1][i2] (i2 fastest).
#ifndef R3G_RECON_CORE_H
#define R3G_RECON_CORE_H
#include <math.h>
#include <stdint.h>

#ifndef R3G_RC_HD
#define R3G_RC_HD static inline
#endif

namespace r3g_rc {

constexpr int kMinDepth = 2, kMaxDepth = 8;
constexpr double kFixed = 1073741824.0;           // 2^30: the unit of the int64 sums
constexpr double kFixedInv = 1.0 / 1073741824.0;
constexpr float kOmegaOver6 = 1.0f / 7.0f;        // damped Jacobi, omega = 6/7, over the diagonal's 6
constexpr float kSixth = 1.0f / 6.0f;
constexpr int kChannels = 4;                      // density, V0, V1, V2

struct Lattice {
    int depth, n;
    float lo[3];        // (float)(centre - side / 2)
    float inv_h;        // (float)(1 / h)
    float inv_2h;       // (float)(1 / (2 h))
};

// centre, side: float64, decided once on the host and handed to both sides
R3G_RC_HD Lattice make_lattice(int depth, const double centre[3], double side) {
    Lattice L;
    L.depth = depth;
    L.n = (1 << depth) + 1;
    const double h = side / (double)(L.n - 1);
    for (int a = 0; a < 3; ++a) L.lo[a] = (float)(centre[a] - 0.5 * side);
    L.inv_h = (float)(1.0 / h);
    L.inv_2h = (float)(1.0 / (2.0 * h));
    return L;
}

// level d of the hierarchy (n_d = 2^d + 1, spacing h * 2^(depth - d)): h_d^2 and its inverse as float32
R3G_RC_HD void level_h2(int depth, double side, int d, float* h2, float* inv_h2) {
    const double hd = side / (double)(1 << depth) * (double)(1 << (depth - d));
    *h2 = (float)(hd * hd);
    *inv_h2 = (float)(1.0 / (hd * hd));
}

R3G_RC_HD bool finite1(float x) { return x - x == 0.0f; }
R3G_RC_HD bool finite3(const float* p) { return finite1(p[0]) && finite1(p[1]) && finite1(p[2]); }
// a usable point: finite coordinates, finite non-zero normal
R3G_RC_HD bool usable(const float* p, const float* nrm) {
    return finite3(p) && finite3(nrm) && (nrm[0] != 0.0f || nrm[1] != 0.0f || nrm[2] != 0.0f);
}

R3G_RC_HD int64_t node(int n, int i0, int i1, int i2) { return ((int64_t)i0 * n + i1) * n + i2; }

// the cell of a finite point and its fractions: t = (p - lo) * inv_h, c = clamp(floor(t), 0, n - 2), f = clamp(t - c, 0, 1)
struct Cell {
    int c[3];
    float f[3];
};
R3G_RC_HD Cell locate(const Lattice& L, const float* p) {
    Cell k;
    for (int a = 0; a < 3; ++a) {
        const float d = p[a] - L.lo[a];
        const float t = d * L.inv_h;
        float fl = floorf(t);
        fl = fl > 0.0f ? fl : 0.0f;                                     // (written so that a NaN ends at 0, inside the lattice)
        fl = fl < (float)(L.n - 2) ? fl : (float)(L.n - 2);
        k.c[a] = (int)fl;
        float f = t - fl;
        f = f > 0.0f ? f : 0.0f;
        f = f < 1.0f ? f : 1.0f;
        k.f[a] = f;
    }
    return k;
}

// trilinear weight of corner (d0, d1, d2) in {0, 1}^3: (w0 * w1) * w2 with w_a = d_a ? f_a : 1 - f_a
R3G_RC_HD float corner_weight(const Cell& k, int d0, int d1, int d2) {
    const float w0 = d0 ? k.f[0] : 1.0f - k.f[0];
    const float w1 = d1 ? k.f[1] : 1.0f - k.f[1];
    const float w2 = d2 ? k.f[2] : 1.0f - k.f[2];
    return (w0 * w1) * w2;
}

R3G_RC_HD int64_t to_fixed(float v) { return (int64_t)llrint((double)v * kFixed); }
R3G_RC_HD float from_fixed(int64_t s) { return (float)((double)s * kFixedInv); }

// the unit normal in float32: each component divided in float64 by sqrt of the float64 sum of squares, rounded once
R3G_RC_HD void unit_normal(const float* nrm, float out[3]) {
    const double x = nrm[0], y = nrm[1], z = nrm[2];
    const double len = sqrt((x * x + y * y) + z * z);
    out[0] = (float)(x / len), out[1] = (float)(y / len), out[2] = (float)(z / len);
}

// Splat of one usable point: add(channel, node, fixed) is an integer addition (an atomic on the device).
// channels: int64 [4][n^3]
template <class Add>
R3G_RC_HD void splat_point(const Lattice& L, const float* p, const float* nrm, Add& add) {
    const Cell k = locate(L, p);
    float u[3];
    unit_normal(nrm, u);
    for (int d0 = 0; d0 < 2; ++d0)
        for (int d1 = 0; d1 < 2; ++d1)
            for (int d2 = 0; d2 < 2; ++d2) {
                const float w = corner_weight(k, d0, d1, d2);
                if (w == 0.0f) continue;
                const int64_t at = node(L.n, k.c[0] + d0, k.c[1] + d1, k.c[2] + d2);
                add(0, at, to_fixed(w));
                add(1, at, to_fixed(w * u[0]));
                add(2, at, to_fixed(w * u[1]));
                add(3, at, to_fixed(w * u[2]));
            }
}

// Trilinear sample at a finite point: acc = 0, then acc += w * value over the 8 corners in the order of splat_point
// (corners of weight 0 are skipped).  load(node) gives the float32 value of a node.
template <class Load>
R3G_RC_HD float sample_point(const Lattice& L, const float* p, const Load& load) {
    const Cell k = locate(L, p);
    float acc = 0.0f;
    for (int d0 = 0; d0 < 2; ++d0)
        for (int d1 = 0; d1 < 2; ++d1)
            for (int d2 = 0; d2 < 2; ++d2) {
                const float w = corner_weight(k, d0, d1, d2);
                if (w == 0.0f) continue;
                acc = acc + w * load(node(L.n, k.c[0] + d0, k.c[1] + d1, k.c[2] + d2));
            }
    return acc;
}

R3G_RC_HD bool interior(int n, int i0, int i1, int i2) {
    return i0 > 0 && i0 < n - 1 && i1 > 0 && i1 < n - 1 && i2 > 0 && i2 < n - 1;
}

// b = div V at an interior node by central differences: ((d0 + d1) + d2) * inv_2h, d_a = V_a[+1] - V_a[-1]; 0 on the boundary
R3G_RC_HD float rhs_node(const int64_t* ch, const Lattice& L, int i0, int i1, int i2) {
    const int n = L.n;
    if (!interior(n, i0, i1, i2)) return 0.0f;
    const int64_t n3 = (int64_t)n * n * n;
    const float d0 = from_fixed(ch[n3 + node(n, i0 + 1, i1, i2)]) - from_fixed(ch[n3 + node(n, i0 - 1, i1, i2)]);
    const float d1 = from_fixed(ch[2 * n3 + node(n, i0, i1 + 1, i2)]) - from_fixed(ch[2 * n3 + node(n, i0, i1 - 1, i2)]);
    const float d2 = from_fixed(ch[3 * n3 + node(n, i0, i1, i2 + 1)]) - from_fixed(ch[3 * n3 + node(n, i0, i1, i2 - 1)]);
    return ((d0 + d1) + d2) * L.inv_2h;
}

// sum of the six neighbours of an interior node: ((x0- + x0+) + (x1- + x1+)) + (x2- + x2+)
R3G_RC_HD float nbr_sum(const float* x, int n, int i0, int i1, int i2) {
    const int64_t at = node(n, i0, i1, i2), s0 = (int64_t)n * n, s1 = n;
    return ((x[at - s0] + x[at + s0]) + (x[at - s1] + x[at + s1])) + (x[at - 1] + x[at + 1]);
}

// one damped Jacobi sweep of (sum - 6 x) / h^2 = b at a node: x + (1/7) * ((sum - 6 x) - h^2 b); 0 on the boundary
R3G_RC_HD float smooth_node(const float* x, const float* b, int n, float h2, int i0, int i1, int i2) {
    if (!interior(n, i0, i1, i2)) return 0.0f;
    const int64_t at = node(n, i0, i1, i2);
    const float c = x[at];
    const float r = (nbr_sum(x, n, i0, i1, i2) - 6.0f * c) - h2 * b[at];
    return c + kOmegaOver6 * r;
}

// residual b - (sum - 6 x) * inv_h2 at an interior node
R3G_RC_HD float residual_node(const float* x, const float* b, int n, float inv_h2, int i0, int i1, int i2) {
    const int64_t at = node(n, i0, i1, i2);
    return b[at] - (nbr_sum(x, n, i0, i1, i2) - 6.0f * x[at]) * inv_h2;
}

// full weighting, by the number of axes on which the fine node is off the coarse one: 1/8, 1/16, 1/32, 1/64
#define R3G_RC_FULL_WEIGHTS {0.125f, 0.0625f, 0.03125f, 0.015625f}

// Coarse right-hand side at coarse node (I0, I1, I2) of a level of nc = (nf + 1) / 2 nodes: the full weighting of the fine
// residual over the 27 fine nodes 2 I + e, e in {-1, 0, 1}^3 in lexicographic order, acc += w * r; 0 on the coarse boundary.
// (Every fine node touched is interior: 1 <= 2 I + e <= nf - 2.)
R3G_RC_HD float restrict_node(const float* xf, const float* bf, int nf, float inv_h2f, const float* w4, int I0, int I1, int I2) {
    const int nc = (nf + 1) / 2;
    if (!interior(nc, I0, I1, I2)) return 0.0f;
    float acc = 0.0f;
    for (int e0 = -1; e0 <= 1; ++e0)
        for (int e1 = -1; e1 <= 1; ++e1)
            for (int e2 = -1; e2 <= 1; ++e2) {
                const float w = w4[(e0 != 0) + (e1 != 0) + (e2 != 0)];
                acc = acc + w * residual_node(xf, bf, nf, inv_h2f, 2 * I0 + e0, 2 * I1 + e1, 2 * I2 + e2);
            }
    return acc;
}

// Trilinear prolongation of the coarse correction to fine node (i0, i1, i2), interior: on an even axis the coarse node i/2
// with weight 1, on an odd one (i - 1)/2 and (i + 1)/2 with weight 1/2 each; acc += (w0 * w1 * w2) * xc in lexicographic
// order of the (up to 8) coarse nodes.  Returns x + acc; the boundary keeps 0.
R3G_RC_HD float prolong_node(const float* xf, const float* xc, int nf, int i0, int i1, int i2) {
    if (!interior(nf, i0, i1, i2)) return 0.0f;
    const int nc = (nf + 1) / 2;
    const int o0 = i0 & 1, o1 = i1 & 1, o2 = i2 & 1;
    const float w = (o0 ? 0.5f : 1.0f) * (o1 ? 0.5f : 1.0f) * (o2 ? 0.5f : 1.0f);      // a power of two: exact
    float acc = 0.0f;
    for (int a0 = 0; a0 <= o0; ++a0)
        for (int a1 = 0; a1 <= o1; ++a1)
            for (int a2 = 0; a2 <= o2; ++a2) acc = acc + w * xc[node(nc, (i0 >> 1) + a0, (i1 >> 1) + a1, (i2 >> 1) + a2)];
    return xf[node(nf, i0, i1, i2)] + acc;
}

// the coarsest level (3^3 nodes, one interior node): -6 x / h^2 = b  ->  x = -((h^2 b) * (1/6))
R3G_RC_HD float coarsest_value(float b, float h2) { return -((h2 * b) * kSixth); }

}  // namespace r3g_rc
#endif
