// meshfill_core.h -- the definitions of the hole-filling primitive, shared by the kernels
// (meshfill_kernels.hip) and the host twin (tests/emu/meshfill_emu.cpp).  Everything here is a pure function of its arguments;
// the includer defines R3G_MF_HD (`static __host__ __device__ __forceinline__` under hipcc, `static inline` on the host) and
// compiles with -ffp-contract=off.
//
// The boundary half-edges (mate = -1 in the table of section 4i) are compacted by ascending id into B slots; from here on a
// boundary half-edge is its slot c.  succ[c] is the slot that leaves head(c) when that vertex is simple, else -1, so succ is
// injective where it is defined and the slots fall into cycles (the loops) and chains that end in -1 (the tangled ones).
#ifndef R3G_MESHFILL_CORE_H
#define R3G_MESHFILL_CORE_H
#include <stdint.h>

#ifndef R3G_MF_HD
#define R3G_MF_HD static inline
#endif

namespace r3g_mf {

constexpr int kModeFan = 0, kModeCentroid = 1;
constexpr int64_t kMinLoop = 3;

// the int64 [16] report of r3g_meshfill_plan
enum {
    kRepBoundary = 0, kRepLoops, kRepTangled, kRepFilled, kRepOversize, kRepLongest, kRepLoopEdges, kRepFacesAdded, kRepVertsAdded,
    kRepRounds, kRepMaxLoop, kRepMode, kRepFaces, kRepVerts
};

// what the allocation pass leaves (one read-back); integer atomics only
struct Small {
    unsigned long long loops, filled, loop_edges, faces_added;
    uint32_t longest, pad;
};

// tail and head of half-edge h = 3 f + k
R3G_MF_HD int32_t he_tail(const int32_t* faces, int64_t h) { return faces[h]; }
R3G_MF_HD int32_t he_head(const int32_t* faces, int64_t h) { return faces[h - h % 3 + (h % 3 + 1) % 3]; }

// one 64-bit add per endpoint: nout in the low word, nin in the high word
constexpr unsigned long long kDegOut = 1ull, kDegIn = 1ull << 32;
R3G_MF_HD uint32_t deg_out(unsigned long long d) { return (uint32_t)d; }
R3G_MF_HD bool vertex_simple(unsigned long long d) { return d == (kDegOut | kDegIn); }

// rounds of each doubling: a window of 2^rounds >= B slots covers every cycle and every chain
R3G_MF_HD int rounds_for(int64_t boundary) {
    if (boundary <= 0) return 0;
    int r = 1;
    while ((1ll << r) < boundary) ++r;
    return r;
}

// One round of the minimum / open doubling for one slot.  m: the lowest slot within the window, p: the slot one window ahead,
// -1 once the window has run off the end of a chain (it stays -1: that is the open flag).  load_m / load_p read the PREVIOUS
// round's arrays only.
template <class LoadM, class LoadP>
R3G_MF_HD void min_step(LoadM load_m, LoadP load_p, int32_t m, int32_t p, int32_t* m_out, int32_t* p_out) {
    if (p < 0) {
        *m_out = m, *p_out = -1;
        return;
    }
    const int32_t mp = load_m(p);
    *m_out = mp < m ? mp : m;
    *p_out = load_p(p);
}

// One round of the rank doubling (Wyllie): d counts the succ steps from the slot to q; the leader is terminal (q = itself,
// d = 0), so after the last round d is the number of steps to the leader.
template <class LoadQ, class LoadD>
R3G_MF_HD void rank_step(LoadQ load_q, LoadD load_d, int32_t q, int32_t d, int32_t* q_out, int32_t* d_out) {
    *d_out = d + load_d(q);
    *q_out = load_q(q);
}

// the loop's length from the steps its leader's successor needs, and a slot's rank from its own
R3G_MF_HD int32_t loop_length(int32_t d_of_succ_of_leader) { return d_of_succ_of_leader + 1; }
R3G_MF_HD int32_t loop_rank(int32_t length, int32_t d) { return (length - d) % length; }

R3G_MF_HD bool loop_kept(int32_t length, int64_t max_loop) { return (int64_t)length <= max_loop; }
R3G_MF_HD uint32_t loop_faces(int32_t length, int mode) { return (uint32_t)(mode == kModeFan ? length - 2 : length); }

// The face that the slot of rank i emits into the loop's block of faces, if any.  a(i) reads loop vertex i (0 <= i < length).
// fan: ranks 1 .. L - 2 emit (a_0, a_(i+1), a_i) at i - 1; centroid: every rank emits (c, a_(i+1)%L, a_i) at i.
// -> the face's place inside the block, or -1
template <class LoopVert>
R3G_MF_HD int32_t loop_face(LoopVert a, int32_t length, int32_t i, int mode, int32_t centre, int32_t out[3]) {
    if (mode == kModeFan) {
        if (i < 1 || i > length - 2) return -1;
        out[0] = a(0), out[1] = a(i + 1), out[2] = a(i);
        return i - 1;
    }
    out[0] = centre, out[1] = a(i + 1 == length ? 0 : i + 1), out[2] = a(i);
    return i;
}

// The centroid: per coordinate the float64 sum of the float32 values in rank order, one rounding per addition, the float64
// quotient by the length, converted once to float32.  coord(i, k) reads coordinate k of loop vertex i.
template <class Coord>
R3G_MF_HD void loop_centroid(Coord coord, int32_t length, float out[3]) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int32_t i = 0; i < length; ++i)
        for (int k = 0; k < 3; ++k) s[k] = s[k] + (double)coord(i, k);
    for (int k = 0; k < 3; ++k) out[k] = (float)(s[k] / (double)length);
}

}  // namespace r3g_mf
#endif
