// orient_core.h -- per-element bodies of the normal orientation (part A): the weight of a graph edge, the
// neighbour list of a point, the hook of a Boruvka round and the keys of the per-tree reductions.  Compiled for the device
// (orient_kernels.hip) and for the host (tests/emu/orient_emu.cpp), both without contraction.
//
// The graph: {i, j} is an edge when j is among the k nearest usable neighbours of i other than i, or the other way round; a
// row of the (k + 1)-list of the cloud against itself (ascending by (d2, index)) gives the neighbours of i by dropping the entry
// i, or the last entry when i is absent (more than k duplicates of the point with lower indices).  Edges are totally ordered by
// (w, min(i, j), max(i, j)), w = 1 - |u_i . u_j| >= 0 in float32 on the unit normals, so the minimum spanning forest is unique
// and nothing depends on the order in which integer atomics land.
#ifndef R3G_ORIENT_CORE_H
#define R3G_ORIENT_CORE_H
#include <stdint.h>

#include "recon_core.h"

#ifndef R3G_OR_HD
#define R3G_OR_HD static inline
#endif

namespace r3g_or {

constexpr int kMinK = 1, kMaxK = 31;            // k + 1 <= 32, the longest list of r3g_cloud_knn
constexpr uint32_t kNoWeight = 0xffffffffu;
constexpr uint64_t kNoPair = ~0ull;
constexpr int kReport = 8;                      // usable, trees, flipped, rounds, frustrated, 0, 0, 0

// u_i . u_j = (ax bx + ay by) + az bz, float32, one rounding per operation
R3G_OR_HD float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the weight's bits: w = 1 - |d|, raised to 0 where rounding left |d| above 1; non-negative floats order as their bits do
R3G_OR_HD uint32_t weight_bits(float d) {
    float w = 1.0f - (d < 0.0f ? -d : d);
    w = w > 0.0f ? w : 0.0f;
    union {
        float f;
        uint32_t u;
    } c;
    c.f = w;
    return c.u;
}
// 1 when the two signs must differ along the edge: u_i . u_j < 0
R3G_OR_HD int flip_bit(float d) { return d < 0.0f ? 1 : 0; }

R3G_OR_HD uint64_t pack_pair(int32_t i, int32_t j) {
    const uint32_t lo = (uint32_t)(i < j ? i : j), hi = (uint32_t)(i < j ? j : i);
    return ((uint64_t)lo << 32) | hi;
}
R3G_OR_HD int32_t pair_lo(uint64_t p) { return (int32_t)(p >> 32); }
R3G_OR_HD int32_t pair_hi(uint64_t p) { return (int32_t)(p & 0xffffffffu); }

// Walk the neighbours of point i in its row of k + 1 entries: f(j) for every neighbour j, in the row's order
template <class F>
R3G_OR_HD void each_neighbour(const int32_t* row, int k, int32_t i, F&& f) {
    bool met = false;
    for (int s = 0; s <= k; ++s) {
        const int32_t j = row[s];
        if (j == i) {
            met = true;
            continue;
        }
        if (s == k && !met) break;      // i is absent: the last entry is the one dropped
        if (j >= 0) f(j);
    }
}

R3G_OR_HD bool has_neighbour(const int32_t* row, int k, int32_t i, int32_t j) {
    bool yes = false;
    each_neighbour(row, k, i, [&](int32_t x) { yes = yes || x == j; });
    return yes;
}

// The hook of root r whose cheapest leaving edge is `pair` (comp and par as they stood before the round; best_* after the two
// minimum passes): r hangs itself under the root at the other end, unless that root chose the same edge and has the higher
// index (a mutual pair keeps the lower root).  -> true when r hooks; then *to is its new parent and *par_to its parity to it.
R3G_OR_HD bool hook(int32_t r, uint64_t pair, const int32_t* comp, const uint8_t* par, const uint64_t* best_pair, const float* unit,
                    int32_t* to, uint8_t* par_to) {
    if (pair == kNoPair) return false;
    const int32_t a = pair_lo(pair), b = pair_hi(pair);
    const int32_t x = comp[a] == r ? a : b, y = comp[a] == r ? b : a;      // x in r, y in the other component
    const int32_t other = comp[y];
    if (best_pair[other] == pair && r < other) return false;
    *to = other;
    *par_to = (uint8_t)(par[x] ^ par[y] ^ flip_bit(dot3(unit + 3 * a, unit + 3 * b)));
    return true;
}

// the key of the per-tree maximum that finds the member with the largest z, the lowest index on a tie: z's bits made to
// order as unsigned, then the complement of the index
R3G_OR_HD uint64_t top_key(float z, int32_t i) {
    union {
        float f;
        uint32_t u;
    } c;
    c.f = z + 0.0f;                                         // -0 -> +0
    const uint32_t o = (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
    return ((uint64_t)o << 32) | (uint32_t)(~(uint32_t)i);
}
R3G_OR_HD int32_t top_index(uint64_t key) { return (int32_t)(~(uint32_t)(key & 0xffffffffu)); }

// is edge {i, j} (seen from i's row) frustrated: both in one tree and the signs disagree with the edge's flip bit
R3G_OR_HD bool frustrated(const int8_t* sign, const float* unit, int32_t i, int32_t j) {
    const int want = flip_bit(dot3(unit + 3 * i, unit + 3 * j));
    return (sign[i] != sign[j]) != (want != 0);
}

}  // namespace r3g_or
#endif
