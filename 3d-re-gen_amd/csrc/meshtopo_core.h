// meshtopo_core.h -- the definitions of the mesh topology primitive, shared by the kernels
// (meshtopo_kernels.hip) and the host twin (tests/emu/meshtopo_emu.cpp).  Everything here is a pure function of its
// arguments; the includer defines R3G_MT_HD (`static __host__ __device__ __forceinline__` under hipcc, `static inline`
// on the host) and compiles with -ffp-contract=off.
//
// Half-edge h = 3 f + k of usable face f = (v0, v1, v2) runs from v_k to v_(k+1)%3.  Its undirected key is (min, max); it is
// FORWARD when it runs min -> max.  An edge's slot in the open-addressing table counts its forward and backward half-edges
// and keeps the lowest and highest half-edge id; with exactly two half-edges the mate of h is lo + hi - h.
#ifndef R3G_MESHTOPO_CORE_H
#define R3G_MESHTOPO_CORE_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef R3G_MT_HD
#define R3G_MT_HD static inline
#endif

namespace r3g_mt {

constexpr int64_t kMaxFaces = 1ll << 29;        // 3 F half-edge ids and 2 F + 1 labels stay inside int32
constexpr int32_t kMateBoundary = -1;
constexpr int32_t kMateNonManifold = -2;
constexpr int32_t kMateSkipped = -3;
constexpr unsigned long long kEdgeEmpty = ~0ull;
constexpr int kMaxRounds = 1024;                // label rounds of one build; reaching it fails the build

// the counts a build leaves (one read-back); the kernels add into it with integer atomics only
struct Small {
    uint32_t bad_index;      // != 0: a face index outside [0, V)
    uint32_t max_bits;       // bits of the largest finite |coordinate| of a referenced vertex (0: none, or no vertices given)
    uint32_t changed;        // a label moved in the last round
    uint32_t pad;
    unsigned long long usable, skipped, vref, nonfinite;
    unsigned long long edges, boundary, clash, nonmanifold;
    unsigned long long bodies, unorientable;
    long long six_volume_q, two_area_q;     // over the faces as they are wound
    long long six_volume_fixed_q;           // over the faces of the ORIENTABLE bodies as `flip` would wind them: what outward = 2
                                            // looks at (the bodies it may reverse, so a reversal negates it exactly)
    unsigned long long faces_reversed, bodies_reversed;     // of the last apply
};

R3G_MT_HD unsigned long long edge_key(int32_t a, int32_t b) {
    const uint32_t lo = (uint32_t)(a < b ? a : b), hi = (uint32_t)(a < b ? b : a);
    return ((unsigned long long)lo << 32) | hi;
}

R3G_MT_HD uint64_t edge_hash(unsigned long long k) {      // splitmix64 finaliser
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}

// slots of the edge table: the power of two >= 6 F (3 F keys at most: the load stays under one half)
R3G_MT_HD uint64_t table_slots(int64_t nf) {
    uint64_t n = 64;
    while (n < 6ull * (uint64_t)nf) n <<= 1;
    return n;
}

R3G_MT_HD bool face_usable(int32_t a, int32_t b, int32_t c) { return a != b && b != c && a != c; }

// one 64-bit add per half-edge: forward count in the low word, backward count in the high word
R3G_MT_HD unsigned long long count_unit(int32_t from, int32_t to) { return from < to ? 1ull : (1ull << 32); }
R3G_MT_HD uint32_t count_fwd(unsigned long long c) { return (uint32_t)c; }
R3G_MT_HD uint32_t count_bwd(unsigned long long c) { return (uint32_t)(c >> 32); }

// ---- labels.  label[f] = (L << 1) | s says "f lies in the body of face L <= f and is wound like L when s == 0, against it
// when s == 1"; -1 marks a skipped face.  A smaller label is a better one; in an orientable body every label that can arise is a
// true statement, so an atomic min of labels loses nothing.
R3G_MT_HD int32_t label_make(int32_t root, int s) { return (int32_t)(((uint32_t)root << 1) | (uint32_t)(s & 1)); }
R3G_MT_HD int32_t label_root(int32_t l) { return l >> 1; }
R3G_MT_HD int label_par(int32_t l) { return l & 1; }

// follow the labels from l to a face that names itself; the roots strictly decrease on the way, so this ends
template <class Load>
R3G_MT_HD int32_t label_chase(Load load, int32_t l) {
    for (;;) {
        const int32_t up = load(label_root(l));
        if (label_root(up) == label_root(l)) return l;
        l = label_make(label_root(up), label_par(l) ^ label_par(up));
    }
}

// One round for face f (usable): take the best of its own chased label and what its neighbours across deg = 2 edges say, give
// it to f and to f's former root.  load(i) reads label[i]; lower(i, v) is label[i] = min(label[i], v) and returns true if that
// lowered it.  clash3[k] != 0: the mate of half-edge k runs in the same direction.  -> did anything move
template <class Load, class Lower>
R3G_MT_HD bool label_round(Load load, Lower lower, int32_t f, const int32_t mate3[3], const uint8_t clash3[3]) {
    const int32_t own = load(f);
    const int32_t mine = label_chase(load, own);
    int32_t best = mine;
    for (int k = 0; k < 3; ++k) {
        if (mate3[k] < 0) continue;
        const int32_t g = mate3[k] / 3;
        const int32_t lg = label_chase(load, load(g));
        const int32_t cand = label_make(label_root(lg), label_par(lg) ^ (clash3[k] ? 1 : 0));
        if (cand < best) best = cand;
    }
    bool moved = false;
    if (best < own) moved = lower(f, best) || moved;
    if (label_root(best) < label_root(mine))        // f's former root learns the lower one, with the parity through f
        moved = lower(label_root(mine), label_make(label_root(best), label_par(best) ^ label_par(mine))) || moved;
    return moved;
}

// ---- volume and area: float64 arithmetic on the float32 inputs, one rounding per product and difference as written.
// six_vol is det[a, b, c] expanded along b, the vertex a reversal [c, b, a] leaves in place: every minor changes its sign
// exactly when a and c swap, so six_vol(c, b, a) == -six_vol(a, b, c) to the bit.
R3G_MT_HD double six_vol(const float a[3], const float b[3], const float c[3]) {
    const double a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2], c0 = c[0], c1 = c[1], c2 = c[2];
    const double m0 = a1 * c2 - a2 * c1;
    const double m1 = a0 * c2 - a2 * c0;
    const double m2 = a0 * c1 - a1 * c0;
    const double t0 = b0 * m0, t1 = b1 * m1, t2 = b2 * m2;
    return (t1 - t0) - t2;
}

R3G_MT_HD double two_area(const float a[3], const float b[3], const float c[3]) {
    const double u0 = (double)b[0] - (double)a[0], u1 = (double)b[1] - (double)a[1], u2 = (double)b[2] - (double)a[2];
    const double v0 = (double)c[0] - (double)a[0], v1 = (double)c[1] - (double)a[1], v2 = (double)c[2] - (double)a[2];
    const double n0 = u1 * v2 - u2 * v1;
    const double n1 = u2 * v0 - u0 * v2;
    const double n2 = u0 * v1 - u1 * v0;
    return sqrt((n0 * n0 + n1 * n1) + n2 * n2);
}

R3G_MT_HD uint32_t float_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
R3G_MT_HD bool finite_f(float x) { return (float_bits(x) & 0x7f800000u) != 0x7f800000u; }

// The scale exponents.  max_bits = the bits of M, the largest finite |coordinate|; M < 2^e with e = (max_bits >> 23) - 126.
// |six_vol| <= (sqrt(3) M)^3 < 8 M^3 < 2^(3 e + 3) and two_area <= (2 sqrt(3) M)^2 < 16 M^2 < 2^(2 e + 4) (the roundings of
// the float64 evaluation are far inside that slack), so with
//     s_vol = 30 - 3 e        s_area = 29 - 2 e
// every |x 2^s| < 2^33, every |q| <= 2^33, and 2^29 faces sum to at most 2^62: no int64 overflow.
R3G_MT_HD int scale_e(uint32_t max_bits) { return (int)(max_bits >> 23) - 126; }
R3G_MT_HD int vol_scale(uint32_t max_bits) { return 30 - 3 * scale_e(max_bits); }
R3G_MT_HD int area_scale(uint32_t max_bits) { return 29 - 2 * scale_e(max_bits); }

// q = llrint(x * 2^s): the product is exact (a power of two; s in [-354, 408] is a normal double), so the only rounding is
// llrint's, at most 1/2 per face:  |sum q / 2^s - sum x| <= faces * 2^-(s + 1)
R3G_MT_HD long long quantise(double x, int s) {
    const uint64_t bits = (uint64_t)(s + 1023) << 52;
    double p;
    memcpy(&p, &bits, 8);
    return llrint(x * p);
}

}  // namespace r3g_mt
#endif
