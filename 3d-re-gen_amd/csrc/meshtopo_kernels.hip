// meshtopo_kernels.hip -- half-edge mates, edge classes, bodies with winding parity, quantised volume / area and the in-place
// reversal.
//
// check (index range, usable faces, referenced vertices, |coordinate| maximum) -> edge insert (open addressing, 64-bit CAS on
// the key; per slot a 64-bit add of the forward / backward counts and min / max of the half-edge id) -> classify (mate, clash
// bit, class counts) -> label rounds until one moves nothing (meshtopo_core.h: label_round) -> verify (unorientable bodies)
// -> sums -> apply.  Integer atomics only, and their order decides nothing: counts and sums are integer sums, lo / hi are a
// min and a max, the labels only ever decrease towards a fixed point that the definition fixes.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_MT_HD static __host__ __device__ __forceinline__
#include "mesh_launch.h"
#include "meshtopo_kernels.h"
#include "wave_sum.h"

namespace r3g {
namespace {

using r3g_mt::Small;

// A lane's count in the kernels below is at most ceil(3 * 2^29 / (4096 * 256)) = 1536, a wave's at most 98304: exact in float.
__device__ __forceinline__ unsigned long long wave_count(unsigned n) { return (unsigned long long)wave_sum((float)n); }

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ void add_count(unsigned long long* dst, unsigned n) {
    const unsigned long long t = wave_count(n);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(dst, t);
}

__global__ __launch_bounds__(kT) void mt_check(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ faces,
                                               int64_t nf, int32_t* __restrict__ label, unsigned* __restrict__ vmark,
                                               Small* __restrict__ sm) {
    unsigned usable = 0, skipped = 0, vref = 0, nonfinite = 0, maxbits = 0;
    bool bad = false;
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const int32_t i[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        int32_t l = -1;
        if (i[0] < 0 || i[1] < 0 || i[2] < 0 || i[0] >= nv || i[1] >= nv || i[2] >= nv) {
            bad = true;                                   // nothing is read or marked through a bad index
        } else if (!r3g_mt::face_usable(i[0], i[1], i[2])) {
            ++skipped;
        } else {
            ++usable;
            l = r3g_mt::label_make((int32_t)f, 0);
            bool fin = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned bit = 1u << (i[k] & 31);
                if (!(atomicOr(&vmark[i[k] >> 5], bit) & bit)) ++vref;      // exactly one lane sees the bit clear
                if (verts) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float x = verts[3 * (int64_t)i[k] + a];
                        if (r3g_mt::finite_f(x)) {
                            const unsigned b = r3g_mt::float_bits(x) & 0x7fffffffu;
                            maxbits = b > maxbits ? b : maxbits;
                        } else {
                            fin = false;
                        }
                    }
                }
            }
            if (!fin) ++nonfinite;
        }
        label[f] = l;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = __shfl_xor(maxbits, d, 64);
        maxbits = o > maxbits ? o : maxbits;
    }
    add_count(&sm->usable, usable);
    add_count(&sm->skipped, skipped);
    add_count(&sm->vref, vref);
    add_count(&sm->nonfinite, nonfinite);
    const unsigned long long anybad = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        if (maxbits) atomicMax(&sm->max_bits, maxbits);
        if (anybad) atomicOr(&sm->bad_index, 1u);
    }
}

__global__ __launch_bounds__(kT) void mt_insert(const int32_t* __restrict__ faces, int64_t nf, const int32_t* __restrict__ label,
                                                unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts,
                                                int32_t* __restrict__ lo, int32_t* __restrict__ hi, uint32_t* __restrict__ hslot,
                                                uint64_t mask) {
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        if (label[f] < 0) continue;
        const int32_t v[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int32_t a = v[k], b = v[(k + 1) % 3];
            const unsigned long long key = r3g_mt::edge_key(a, b);
            uint64_t slot = r3g_mt::edge_hash(key) & mask;
            for (;;) {          // the table is at most half full: an empty slot or the key itself comes up
                const unsigned long long prev = atomicCAS(&keys[slot], r3g_mt::kEdgeEmpty, key);
                if (prev == r3g_mt::kEdgeEmpty || prev == key) break;
                slot = (slot + 1) & mask;
            }
            const int32_t h = (int32_t)(3 * f + k);
            atomicAdd(&counts[slot], r3g_mt::count_unit(a, b));
            atomicMin(&lo[slot], h);
            atomicMax(&hi[slot], h);
            hslot[h] = (uint32_t)slot;
        }
    }
}

__global__ __launch_bounds__(kT) void mt_classify(int64_t nf, const int32_t* __restrict__ label, const uint32_t* __restrict__ hslot,
                                                  const unsigned long long* __restrict__ counts, const int32_t* __restrict__ lo,
                                                  const int32_t* __restrict__ hi, int32_t* __restrict__ mate,
                                                  uint8_t* __restrict__ hclash, Small* __restrict__ sm) {
    unsigned edges = 0, boundary = 0, clash = 0, nonmanifold = 0;
    for (int64_t h = (int64_t)blockIdx.x * kT + threadIdx.x; h < 3 * nf; h += (int64_t)gridDim.x * kT) {
        int32_t m = r3g_mt::kMateSkipped;
        uint8_t cl = 0;
        if (label[h / 3] >= 0) {
            const uint32_t slot = hslot[h];
            const unsigned long long c = counts[slot];
            const uint32_t fwd = r3g_mt::count_fwd(c), bwd = r3g_mt::count_bwd(c);
            const uint64_t deg = (uint64_t)fwd + bwd;
            const int32_t l = lo[slot];
            const bool first = l == (int32_t)h;             // the edge is counted at its lowest half-edge
            if (deg == 1) {
                m = r3g_mt::kMateBoundary;
                boundary += first;
            } else if (deg == 2) {
                m = (int32_t)((int64_t)l + hi[slot] - h);
                cl = fwd != 1;
                clash += first && cl;
            } else {
                m = r3g_mt::kMateNonManifold;
                nonmanifold += first;
            }
            edges += first;
        }
        mate[h] = m;
        hclash[h] = cl;
    }
    add_count(&sm->edges, edges);
    add_count(&sm->boundary, boundary);
    add_count(&sm->clash, clash);
    add_count(&sm->nonmanifold, nonmanifold);
}

struct LabelLoad {
    int32_t* label;
    __device__ int32_t operator()(int32_t i) const {
        return __hip_atomic_load(&label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct LabelLower {
    int32_t* label;
    __device__ bool operator()(int32_t i, int32_t v) const { return atomicMin(&label[i], v) > v; }
};

__global__ __launch_bounds__(kT) void mt_round(int64_t nf, const int32_t* __restrict__ mate, const uint8_t* __restrict__ hclash,
                                               int32_t* label, Small* __restrict__ sm) {
    bool moved = false;
    const LabelLoad load{label};
    const LabelLower lower{label};
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        if (load((int32_t)f) < 0) continue;
        const int32_t m3[3] = {mate[3 * f], mate[3 * f + 1], mate[3 * f + 2]};
        const uint8_t c3[3] = {hclash[3 * f], hclash[3 * f + 1], hclash[3 * f + 2]};
        moved = r3g_mt::label_round(load, lower, (int32_t)f, m3, c3) || moved;
    }
    const unsigned long long any = __ballot(moved);
    if ((threadIdx.x & 63) == 0 && any) atomicOr(&sm->changed, 1u);
}

// after the fixed point: every label names its body's lowest face directly.  A deg = 2 edge whose two parities do not differ by
// its clash bit exists exactly in the bodies that are not orientable.
__global__ __launch_bounds__(kT) void mt_verify(int64_t nf, const int32_t* __restrict__ mate, const uint8_t* __restrict__ hclash,
                                                const int32_t* __restrict__ label, unsigned* __restrict__ unori) {
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const int32_t l = label[f];
        if (l < 0) continue;
        bool broken = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int32_t m = mate[3 * f + k];
            if (m < 0) continue;
            const int32_t lg = label[m / 3];
            broken = broken || ((r3g_mt::label_par(l) ^ r3g_mt::label_par(lg)) != (int)hclash[3 * f + k]);
        }
        if (broken) atomicOr(&unori[r3g_mt::label_root(l)], 1u);
    }
}

__global__ __launch_bounds__(kT) void mt_sums(const float* __restrict__ verts, const int32_t* __restrict__ faces, int64_t nf,
                                              const int32_t* __restrict__ label, const unsigned* __restrict__ unori,
                                              int32_t* __restrict__ body, uint8_t* __restrict__ flip, long long* __restrict__ bodyvol,
                                              Small* __restrict__ sm) {
    unsigned bodies = 0, unorientable = 0;
    long long vol = 0, volfix = 0, area = 0;
    const uint32_t maxbits = sm->max_bits;             // written by mt_check, launches ago
    const int sv = r3g_mt::vol_scale(maxbits), sa = r3g_mt::area_scale(maxbits);
    const int64_t stride = (int64_t)gridDim.x * kT;
    const int64_t first = (int64_t)blockIdx.x * kT + threadIdx.x;
    for (int64_t f0 = first - threadIdx.x % 64; f0 < nf; f0 += stride) {       // whole waves stay in step for the body sums
        const int64_t f = f0 + threadIdx.x % 64;
        int32_t root = -1;
        long long q = 0;
        if (f < nf) {
            const int32_t l = label[f];
            uint8_t fl = 0;
            if (l >= 0) {
                root = r3g_mt::label_root(l);
                const bool u = unori[root] != 0;
                fl = u ? 0 : (uint8_t)r3g_mt::label_par(l);
                if (root == (int32_t)f) {
                    ++bodies;
                    unorientable += u;
                }
                if (verts) {
                    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
                    const float a[3] = {verts[3 * (int64_t)i0], verts[3 * (int64_t)i0 + 1], verts[3 * (int64_t)i0 + 2]};
                    const float b[3] = {verts[3 * (int64_t)i1], verts[3 * (int64_t)i1 + 1], verts[3 * (int64_t)i1 + 2]};
                    const float c[3] = {verts[3 * (int64_t)i2], verts[3 * (int64_t)i2 + 1], verts[3 * (int64_t)i2 + 2]};
                    bool fin = true;
#pragma unroll
                    for (int k = 0; k < 3; ++k) fin = fin && r3g_mt::finite_f(a[k]) && r3g_mt::finite_f(b[k]) && r3g_mt::finite_f(c[k]);
                    if (fin) {
                        const long long q0 = r3g_mt::quantise(r3g_mt::six_vol(a, b, c), sv);
                        q = fl ? -q0 : q0;
                        vol += q0;
                        if (!u) volfix += q;             // what outward = 2 looks at: the bodies it may reverse
                        area += r3g_mt::quantise(r3g_mt::two_area(a, b, c), sa);
                    }
                }
            }
            body[f] = root;
            flip[f] = fl;
        }
        if (verts) {
            // most waves lie inside one body: one add for the wave; otherwise one per lane
            const int32_t lead = __shfl(root, __ffsll((long long)__ballot(root >= 0)) - 1, 64);
            const bool one = __ballot(root >= 0 && root != lead) == 0;
            if (one) {
                const long long t = wave_sum_i64(q);
                if (threadIdx.x % 64 == 0 && lead >= 0 && t) atomicAdd((unsigned long long*)&bodyvol[lead], (unsigned long long)t);
            } else if (root >= 0 && q) {
                atomicAdd((unsigned long long*)&bodyvol[root], (unsigned long long)q);
            }
        }
    }
    add_count(&sm->bodies, bodies);
    add_count(&sm->unorientable, unorientable);
    if (verts) {
        vol = wave_sum_i64(vol), volfix = wave_sum_i64(volfix), area = wave_sum_i64(area);
        if ((threadIdx.x & 63) == 0) {
            if (vol) atomicAdd((unsigned long long*)&sm->six_volume_q, (unsigned long long)vol);
            if (volfix) atomicAdd((unsigned long long*)&sm->six_volume_fixed_q, (unsigned long long)volfix);
            if (area) atomicAdd((unsigned long long*)&sm->two_area_q, (unsigned long long)area);
        }
    }
}

__global__ __launch_bounds__(kT) void mt_apply(int32_t* __restrict__ faces, int64_t nf, const int32_t* __restrict__ body,
                                               const uint8_t* __restrict__ flip, const unsigned* __restrict__ unori,
                                               const long long* __restrict__ bodyvol, int outward, Small* __restrict__ sm) {
    unsigned nfaces = 0, nbodies = 0;
    const bool all = outward == 2 && sm->six_volume_fixed_q < 0;     // written by mt_sums; this kernel adds to other fields only
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const int32_t b = body[f];
        if (b < 0) continue;
        bool rev = flip[f] != 0;
        if (!unori[b] && (all || (outward == 1 && bodyvol[b] < 0))) {
            rev = !rev;
            nbodies += b == (int32_t)f;
        }
        if (rev) {
            const int32_t t = faces[3 * f];
            faces[3 * f] = faces[3 * f + 2];
            faces[3 * f + 2] = t;
            ++nfaces;
        }
    }
    add_count(&sm->faces_reversed, nfaces);
    add_count(&sm->bodies_reversed, nbodies);
}

}  // namespace

static_assert(sizeof(Small) == 136, "r3g_mt::Small travels through the context's pinned buffer");

size_t meshtopo_workspace_bytes(int64_t nv, int64_t nf, MeshtopoLayout* lay) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t F = (size_t)nf;
    lay->slots = r3g_mt::table_slots(nf);
    size_t o = 0;
    lay->off_small = o, o += 256;
    lay->off_label = o, o += up(4 * F);
    lay->off_mate = o, o += up(12 * F);
    lay->off_hslot = o, o += up(12 * F);
    lay->off_hclash = o, o += up(3 * F);
    lay->off_body = o, o += up(4 * F);
    lay->off_flip = o, o += up(F);
    lay->off_unori = o, o += up(4 * F);
    lay->off_bodyvol = o, o += up(8 * F);
    lay->off_vmark = o, o += up(4 * (((size_t)nv + 31) / 32) + 4);
    lay->off_keys = o, o += up(8 * (size_t)lay->slots);
    lay->off_counts = o, o += up(8 * (size_t)lay->slots);
    lay->off_lo = o, o += up(4 * (size_t)lay->slots);
    lay->off_hi = o, o += up(4 * (size_t)lay->slots);
    lay->total = o;
    return o;
}

hipError_t meshtopo_check(char* ws, const MeshtopoLayout& lay, const float* verts, int64_t nv, const int32_t* faces, int64_t nf,
                          hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small, 0, sizeof(Small), s));
    R3G_HIP(hipMemsetAsync(ws + lay.off_vmark, 0, 4 * (((size_t)nv + 31) / 32) + 4, s));
    hipLaunchKernelGGL(mt_check, dim3(grid_for(nf)), dim3(kT), 0, s, verts, nv, faces, nf, (int32_t*)(ws + lay.off_label),
                       (unsigned*)(ws + lay.off_vmark), (Small*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t meshtopo_edges(char* ws, const MeshtopoLayout& lay, const int32_t* faces, int64_t nf, hipStream_t s) {
    const size_t n = (size_t)lay.slots;
    R3G_HIP(hipMemsetAsync(ws + lay.off_keys, 0xFF, 8 * n, s));        // kEdgeEmpty
    R3G_HIP(hipMemsetAsync(ws + lay.off_counts, 0, 8 * n, s));
    R3G_HIP(hipMemsetAsync(ws + lay.off_lo, 0x7F, 4 * n, s));          // 0x7f7f7f7f: above every half-edge id (< 3 * 2^29)
    R3G_HIP(hipMemsetAsync(ws + lay.off_hi, 0xFF, 4 * n, s));          // -1
    hipLaunchKernelGGL(mt_insert, dim3(grid_for(nf)), dim3(kT), 0, s, faces, nf, (const int32_t*)(ws + lay.off_label),
                       (unsigned long long*)(ws + lay.off_keys), (unsigned long long*)(ws + lay.off_counts),
                       (int32_t*)(ws + lay.off_lo), (int32_t*)(ws + lay.off_hi), (uint32_t*)(ws + lay.off_hslot),
                       (uint64_t)(lay.slots - 1));
    hipLaunchKernelGGL(mt_classify, dim3(grid_for(3 * nf)), dim3(kT), 0, s, nf, (const int32_t*)(ws + lay.off_label),
                       (const uint32_t*)(ws + lay.off_hslot), (const unsigned long long*)(ws + lay.off_counts),
                       (const int32_t*)(ws + lay.off_lo), (const int32_t*)(ws + lay.off_hi), (int32_t*)(ws + lay.off_mate),
                       (uint8_t*)(ws + lay.off_hclash), (Small*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t meshtopo_round(char* ws, const MeshtopoLayout& lay, int64_t nf, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(Small, changed), 0, 4, s));
    hipLaunchKernelGGL(mt_round, dim3(grid_for(nf)), dim3(kT), 0, s, nf, (const int32_t*)(ws + lay.off_mate),
                       (const uint8_t*)(ws + lay.off_hclash), (int32_t*)(ws + lay.off_label), (Small*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t meshtopo_finish(char* ws, const MeshtopoLayout& lay, const float* verts, const int32_t* faces, int64_t nf, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_unori, 0, 4 * (size_t)nf, s));
    R3G_HIP(hipMemsetAsync(ws + lay.off_bodyvol, 0, 8 * (size_t)nf, s));
    hipLaunchKernelGGL(mt_verify, dim3(grid_for(nf)), dim3(kT), 0, s, nf, (const int32_t*)(ws + lay.off_mate),
                       (const uint8_t*)(ws + lay.off_hclash), (const int32_t*)(ws + lay.off_label), (unsigned*)(ws + lay.off_unori));
    hipLaunchKernelGGL(mt_sums, dim3(grid_for(nf)), dim3(kT), 0, s, verts, faces, nf, (const int32_t*)(ws + lay.off_label),
                       (const unsigned*)(ws + lay.off_unori), (int32_t*)(ws + lay.off_body), (uint8_t*)(ws + lay.off_flip),
                       (long long*)(ws + lay.off_bodyvol), (Small*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t meshtopo_apply(char* ws, const MeshtopoLayout& lay, int32_t* faces, int64_t nf, int outward, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(Small, faces_reversed), 0, 16, s));
    hipLaunchKernelGGL(mt_apply, dim3(grid_for(nf)), dim3(kT), 0, s, faces, nf, (const int32_t*)(ws + lay.off_body),
                       (const uint8_t*)(ws + lay.off_flip), (const unsigned*)(ws + lay.off_unori),
                       (const long long*)(ws + lay.off_bodyvol), outward, (Small*)(ws + lay.off_small));
    return hipGetLastError();
}

}  // namespace r3g
