// softras_core.h -- the definition of the soft silhouette: which faces are drawn, the fragment of a face at
// a pixel (clipped barycentrics, depth, signed squared distance to the nearest edge), the K smallest keys (depth, face) of a
// pixel, the sigmoid blend, and the gradient of the blend to the xy of the vertices.  Plain C++, float32 throughout, one
// rounding per operation; compiled for the device by softras_kernels.hip and for the host by the test twin
// (tests/emu/softras_emu.cpp), both with contraction off, so the two agree bit for bit.  Nothing here calls expf: sr_exp is
// range reduction, a fixed polynomial and an exponent assembled as integer bits; division and sqrtf are the correctly rounded
// IEEE operations on both sides.
//
// Summation order of the backward (it depends on the face's pixel box alone, never on a schedule):
//   * the box of a face (face_box: the vertices' bounds widened by sqrt(blur_radius) + 1 pixel, cut to the image) is walked in
//     raster order, pixel i = (row y0 + i / bw, column x0 + i % bw);
//   * slot t (0..255) adds the terms of pixels t, t + 256, t + 512, ... in that order to +0.0 (the vertex off the winning edge
//     gets +0.0; a pixel without a stored fragment of the face adds nothing);
//   * the 256 slots are four groups of 64; a group is summed by the butterfly  for d in 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l ^ d]
//     and the four group sums are added as ((g0 + g1) + g2) + g3.  A box of more than 64 pixels is thereby split over up to
//     four waves.
//   * a vertex sums the entries of its corners sequentially, in ascending corner index 3 f + a, from +0.0.
#ifndef R3G_SOFTRAS_CORE_H
#define R3G_SOFTRAS_CORE_H
#include <math.h>
#include <stdint.h>

#ifndef R3G_SR_HD
#define R3G_SR_HD static inline
#endif

namespace r3g_sr {

constexpr int kMaxK = 32;
constexpr int kTile = 8;               // a tile is 8 x 8 pixels: one wave, one lane per pixel
constexpr int kMaxSide = 16384;        // height and width
constexpr float kMinArea = 1e-8f;      // |edge function| of a face that is drawn, and |v1 - v0|^2 of an edge that has a direction
constexpr float kMaxCoord = 1e15f;     // a face with a larger |coordinate| is skipped: its squared distances would overflow
constexpr float kSigmoidClamp = 80.0f;
constexpr int kBackThreads = 256;      // slots of the backward's summation order
constexpr int kFwdReport = 8, kBwdReport = 4, kPasses = 4;

// deliberate departures from the definition, for the test twin alone (the device passes 0)
enum Mutant { kNone = 0, kBlurLessEqual = 1, kNoFaceKey = 2, kUnclippedDepth = 3, kNarrowBox = 4, kIgnoreEndpoint = 5, kDivideOut = 6 };

struct Tri {
    float x[3], y[3], z[3];
};

struct Box {
    int x0, x1, y0, y1;      // inclusive; empty when x0 > x1 or y0 > y1
};

struct Frag {
    bool kept;        // inside, or closer than the blur radius; and pz >= 0
    bool inside;
    float pz, dist;
    int edge;         // the edge that gave d2: (edge, (edge + 1) % 3)
    float t, t_raw;   // position of the closest point on it, clamped to [0, 1] / as computed (1 for an edge without length)
    float dx, dy;     // p - closest point
};

R3G_SR_HD float bits_to_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// e^x for x in [-80, 80]: x = k ln2 + r, |r| <= ln2 / 2; Taylor's polynomial of degree 7 in r; 2^k from the exponent bits
R3G_SR_HD float sr_exp(float x) {
    const float t = x * 1.44269502f;
    const float kf = (t + 12582912.0f) - 12582912.0f;      // the nearest integer (1.5 * 2^23: the sum has no fraction bits)
    float r = x - kf * 0.693145752f;                       // ln2's upper bits: the product is exact
    r = r - kf * 1.42860677e-06f;
    float p = 1.0f / 5040.0f;
    p = p * r + 1.0f / 720.0f;
    p = p * r + 1.0f / 120.0f;
    p = p * r + 1.0f / 24.0f;
    p = p * r + 1.0f / 6.0f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const int k = (int)kf;                                 // in [-116, 116]
    return p * bits_to_float((uint32_t)(k + 127) << 23);
}

// 1 / (1 + e^-x), the argument clamped to [-80, 80] (so the smallest value is 1.8e-35, not 0, and no operand is subnormal)
R3G_SR_HD float sr_sigmoid(float x) {
    x = x > kSigmoidClamp ? kSigmoidClamp : x;
    x = x < -kSigmoidClamp ? -kSigmoidClamp : x;
    return 1.0f / (1.0f + sr_exp(-x));
}

R3G_SR_HD bool coord_ok(float v) { return v >= -kMaxCoord && v <= kMaxCoord; }      // false for NaN and +-inf

R3G_SR_HD float edge_fn(float px, float py, float ax, float ay, float bx, float by) { return (px - ax) * (by - ay) - (py - ay) * (bx - ax); }

// the face's vertices; false when an index lies outside [0, n_verts)
R3G_SR_HD bool load_tri(const float* pos, int64_t n_verts, const int32_t* tri, int64_t f, Tri* T) {
    for (int a = 0; a < 3; ++a) {
        const int32_t v = tri[3 * f + a];
        if (v < 0 || v >= n_verts) return false;
        T->x[a] = pos[3 * (int64_t)v], T->y[a] = pos[3 * (int64_t)v + 1], T->z[a] = pos[3 * (int64_t)v + 2];
    }
    return true;
}

// is the face drawn at all; *area = its edge function
R3G_SR_HD bool face_drawn(const Tri& T, float* area) {
    for (int a = 0; a < 3; ++a)
        if (!coord_ok(T.x[a]) || !coord_ok(T.y[a]) || !coord_ok(T.z[a])) return false;
    const float ar = edge_fn(T.x[2], T.y[2], T.x[0], T.y[0], T.x[1], T.y[1]);
    *area = ar;
    if (ar <= kMinArea && ar >= -kMinArea) return false;
    if (T.z[0] < 0.0f && T.z[1] < 0.0f && T.z[2] < 0.0f) return false;
    return true;
}

// the pixels whose centre can hold a fragment of the face: the bounds of the vertices widened by r = sqrtf(blur_radius) and one
// pixel more (the margin of half a pixel covers every rounding below), clamped in float before the conversion
R3G_SR_HD Box face_box(const Tri& T, float r, int width, int height, int mutant = 0) {
    if (mutant == kNarrowBox) r = 0.0f;
    float xl = T.x[0], xh = T.x[0], yl = T.y[0], yh = T.y[0];
    for (int a = 1; a < 3; ++a) {
        xl = T.x[a] < xl ? T.x[a] : xl, xh = T.x[a] > xh ? T.x[a] : xh;
        yl = T.y[a] < yl ? T.y[a] : yl, yh = T.y[a] > yh ? T.y[a] : yh;
    }
    float lo = (xl - r) - 1.0f, hi = (xh + r) + 1.0f;
    lo = lo < 0.0f ? 0.0f : lo, lo = lo > (float)width ? (float)width : lo;
    hi = hi < -1.0f ? -1.0f : hi, hi = hi > (float)(width - 1) ? (float)(width - 1) : hi;
    Box b;
    b.x0 = (int)lo, b.x1 = (int)(hi + 1.0f) - 1;
    lo = (yl - r) - 1.0f, hi = (yh + r) + 1.0f;
    lo = lo < 0.0f ? 0.0f : lo, lo = lo > (float)height ? (float)height : lo;
    hi = hi < -1.0f ? -1.0f : hi, hi = hi > (float)(height - 1) ? (float)(height - 1) : hi;
    b.y0 = (int)lo, b.y1 = (int)(hi + 1.0f) - 1;
    return b;
}

R3G_SR_HD bool box_empty(const Box& b) { return b.x0 > b.x1 || b.y0 > b.y1; }

// the fragment of a drawn face at the point (px, py)
R3G_SR_HD Frag fragment(const Tri& T, float area, float px, float py, float blur_radius, int mutant = 0) {
    Frag g;
    const float b0 = edge_fn(px, py, T.x[1], T.y[1], T.x[2], T.y[2]) / area;
    const float b1 = edge_fn(px, py, T.x[2], T.y[2], T.x[0], T.y[0]) / area;
    const float b2 = edge_fn(px, py, T.x[0], T.y[0], T.x[1], T.y[1]) / area;
    float c0 = b0 > 0.0f ? b0 : 0.0f, c1 = b1 > 0.0f ? b1 : 0.0f, c2 = b2 > 0.0f ? b2 : 0.0f;
    float sum = (c0 + c1) + c2;
    sum = sum > 1e-5f ? sum : 1e-5f;
    c0 = c0 / sum, c1 = c1 / sum, c2 = c2 / sum;
    if (mutant == kUnclippedDepth) c0 = b0, c1 = b1, c2 = b2;
    g.pz = (c0 * T.z[0] + c1 * T.z[1]) + c2 * T.z[2];
    g.inside = b0 > 0.0f && b1 > 0.0f && b2 > 0.0f;
    float best = 0.0f;
    g.edge = 0, g.t = 0.0f, g.t_raw = 0.0f, g.dx = 0.0f, g.dy = 0.0f;
    for (int e = 0; e < 3; ++e) {
        const int a = e, b = e == 2 ? 0 : e + 1;
        const float ex = T.x[b] - T.x[a], ey = T.y[b] - T.y[a];
        const float l2 = ex * ex + ey * ey;
        float t = 1.0f, tr = 1.0f;
        if (l2 > kMinArea) {
            tr = ((px - T.x[a]) * ex + (py - T.y[a]) * ey) / l2;
            t = tr < 0.0f ? 0.0f : tr;
            t = t > 1.0f ? 1.0f : t;
        }
        const float dx = px - (T.x[a] + t * ex), dy = py - (T.y[a] + t * ey);
        const float d2 = dx * dx + dy * dy;
        if (e == 0 || d2 < best) best = d2, g.edge = e, g.t = t, g.t_raw = tr, g.dx = dx, g.dy = dy;
    }
    g.dist = g.inside ? -best : best;
    const bool near = mutant == kBlurLessEqual ? best <= blur_radius : best < blur_radius;
    g.kept = (g.inside || near) && !(g.pz < 0.0f);
    return g;
}

// the order of the fragments of a pixel: (pz, face) lexicographically
R3G_SR_HD bool key_less(float pa, int fa, float pb, int fb, int mutant = 0) {
    if (mutant == kNoFaceKey) return pa <= pb;
    return pa < pb || (pa == pb && fa < fb);
}

// keep the K smallest keys in ascending order; element j of a list lies at [j * stride]
R3G_SR_HD void list_insert(float* lpz, int32_t* lface, float* ldist, int stride, int* n, int K, float pz, int32_t face, float dist, int mutant = 0) {
    int j = *n;
    if (j == K) {
        if (!key_less(pz, face, lpz[(K - 1) * stride], lface[(K - 1) * stride], mutant)) return;
        j = K - 1;
    } else {
        *n = j + 1;
    }
    while (j > 0 && key_less(pz, face, lpz[(j - 1) * stride], lface[(j - 1) * stride], mutant)) {
        lpz[j * stride] = lpz[(j - 1) * stride], lface[j * stride] = lface[(j - 1) * stride], ldist[j * stride] = ldist[(j - 1) * stride];
        --j;
    }
    lpz[j * stride] = pz, lface[j * stride] = face, ldist[j * stride] = dist;
}

R3G_SR_HD float frag_sigmoid(float dist, float sigma) { return sr_sigmoid((-dist) / sigma); }

// alpha = 1 - prod (1 - s_k), the product in list order
R3G_SR_HD float blend(const float* ldist, int stride, int n, float sigma) {
    float prod = 1.0f;
    for (int k = 0; k < n; ++k) prod = prod * (1.0f - frag_sigmoid(ldist[k * stride], sigma));
    return 1.0f - prod;
}

// d alpha / d dist_k of a pixel's stored list (n entries, k among them)
R3G_SR_HD float dalpha_ddist(const float* ldist, int n, int k, float sigma, int mutant = 0) {
    const float sk = frag_sigmoid(ldist[k], sigma);
    float excl = 1.0f;
    if (mutant == kDivideOut) {
        for (int j = 0; j < n; ++j) excl = excl * (1.0f - frag_sigmoid(ldist[j], sigma));
        excl = excl / (1.0f - sk);
    } else {
        for (int j = 0; j < n; ++j)
            if (j != k) excl = excl * (1.0f - frag_sigmoid(ldist[j], sigma));
    }
    return -(((sk * (1.0f - sk)) * excl) / sigma);
}

// the terms face f adds to its six sums (acc[2 a + c]: vertex a of the face, c = x, y) at the pixel whose centre is (px, py),
// whose stored list is lface / ldist [K] and whose incoming gradient is ga; returns whether it added any
R3G_SR_HD bool back_pixel(const Tri& T, float area, float px, float py, float blur_radius, float sigma, float ga, const int32_t* lface,
                          const float* ldist, int K, int32_t f, float* acc, int mutant = 0) {
    if (!(ga - ga == 0.0f)) return false;      // NaN or +-inf: the pixel contributes nothing
    const Frag g = fragment(T, area, px, py, blur_radius, mutant);
    if (!g.kept) return false;
    int n = 0, k = -1;
    for (; n < K && lface[n] >= 0; ++n)
        if (lface[n] == f) k = n;
    if (k < 0) return false;
    const float gd = ga * dalpha_ddist(ldist, n, k, sigma, mutant);
    const float gd2 = g.inside ? -gd : gd;
    const float t = mutant == kIgnoreEndpoint ? g.t_raw : g.t;
    const int a = g.edge, b = g.edge == 2 ? 0 : g.edge + 1;
    const float wa = -2.0f * (1.0f - t), wb = -2.0f * t;
    // (no indexing by a or b: the sums stay in registers.  A sum that starts at +0.0 is never -0.0, so the +0.0 that the vertex
    // off the edge adds changes no bit)
    for (int v = 0; v < 3; ++v) {
        const float w = v == a ? wa : wb;
        const bool on = v == a || v == b;
        acc[2 * v] = acc[2 * v] + (on ? gd2 * (w * g.dx) : 0.0f);
        acc[2 * v + 1] = acc[2 * v + 1] + (on ? gd2 * (w * g.dy) : 0.0f);
    }
    return true;
}

}  // namespace r3g_sr
#endif
