// facecloud_kernels.hip -- for every triangle its nearest point of the context's cloud.
//
// fc_classify: one lane per face: the record of its three vertices, usable or not, and narrow (a cell box of at most kWideCells
//              cells) or wide; the wide faces go into a list through an integer cursor (no output depends on the list's order).
// fc_narrow:   one lane per face walks its own rings (facecloud_core.h); a cell is a run of aligned 16-byte loads.
// fc_wide:     one wave per wide face; the lanes take the cells of a ring's box with stride 64, and after each ring a butterfly
//              takes the lexicographic minimum (d2, index), so the stop test and the next ring's bounds are wave-uniform.  A
//              minimum does not depend on the order, so the result equals the narrow walk's.
// fc_gather:   the backward, one lane per vertex over its corners in ascending corner index; no floating-point atomics.
// -DR3G_FC_NO_WIDE sends every face down the narrow path (tools/bench_facecloud.py measures what the wide one is worth).
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_GRID_HD static __host__ __device__ __forceinline__
#define R3G_MD_HD static __host__ __device__ __forceinline__
#define R3G_CL_HD static __host__ __device__ __forceinline__
#define R3G_CL_HD_MEMBER __host__ __device__ __forceinline__
#define R3G_FC_HD static __host__ __device__ __forceinline__
#include "facecloud_kernels.h"
#include "mesh_launch.h"

namespace r3g {
namespace {

using r3g_fc::Best;
using r3g_fc::Grid;
using r3g_fc::kWave;
using r3g_fc::Pt;
using r3g_fc::Tri;
using r3g_fc::Walk;

constexpr int kWideBlocksMost = 1024;      // fc_wide's waves loop over the list

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// every lane ends with the same answer: the lexicographic minimum over the wave
__device__ __forceinline__ Best wave_best(Best b) {
    for (int d = 32; d >= 1; d >>= 1) {
        Best o;
        o.d = __shfl_xor(b.d, d, 64), o.i = __shfl_xor(b.i, d, 64);
        o.x = __shfl_xor(b.x, d, 64), o.y = __shfl_xor(b.y, d, 64), o.z = __shfl_xor(b.z, d, 64);
        b = r3g_fc::best_min(b, o);
    }
    return b;
}

// what a wave adds to the record: its tests, and the largest ring one of its lanes walked
__device__ __forceinline__ void wave_report(uint32_t ntests, int ring, FacecloudSmall* __restrict__ sm) {
    const unsigned long long t = wave_sum_u64((unsigned long long)ntests);
    const unsigned r = wave_max_u32((unsigned)ring);
    if ((threadIdx.x & 63) == 0) {
        if (t) atomicAdd(&sm->tests, t);
        if (r) atomicMax(&sm->max_ring, r);
    }
}

__global__ __launch_bounds__(kT) void fc_classify(Grid g, const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ tri,
                                                  int64_t n_faces, Tri* __restrict__ recs, int32_t* __restrict__ wide,
                                                  FacecloudSmall* __restrict__ sm) {
    const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long usable = 0;
    if (f < n_faces) {
        const Tri t = r3g_fc::make_record(verts, n_verts, tri[3 * f], tri[3 * f + 1], tri[3 * f + 2]);
        recs[f] = t;
        if (t.valid) {
            usable = 1;
#ifndef R3G_FC_NO_WIDE
            const Walk w = r3g_fc::walk_setup(g, t);
            if (r3g_fc::box_cells(w) > r3g_fc::kWideCells) wide[atomicAdd(&sm->wide, 1u)] = (int32_t)f;      // at most F entries
#endif
        }
    }
    usable = wave_sum_u64(usable);
    if ((threadIdx.x & 63) == 0 && usable) atomicAdd(&sm->usable, usable);
}

__global__ __launch_bounds__(kT) void fc_narrow(Grid g, const Pt* __restrict__ sorted, const unsigned* __restrict__ starts,
                                                const Tri* __restrict__ recs, int64_t n_faces, float* __restrict__ dist2,
                                                int32_t* __restrict__ index, float* __restrict__ weights, float* __restrict__ diff,
                                                FacecloudSmall* __restrict__ sm) {
    const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
    uint32_t ntests = 0;
    int ring = 0;
    if (f < n_faces) {
        const Tri t = recs[f];
        if (!t.valid) {
            r3g_fc::finish_unusable(dist2 + f, index + f, weights + 3 * f, diff + 3 * f);
        } else {
            const Walk w = r3g_fc::walk_setup(g, t);
            bool mine = true;
#ifndef R3G_FC_NO_WIDE
            mine = r3g_fc::box_cells(w) <= r3g_fc::kWideCells;
#endif
            if (mine) {
                Best b = r3g_fc::best_none();
                ring = r3g_fc::walk_narrow(g, sorted, starts, w, t, b, ntests);
                r3g_fc::finish(t, b, dist2 + f, index + f, weights + 3 * f, diff + 3 * f);
            }
        }
    }
    wave_report(ntests, ring, sm);
}

__global__ __launch_bounds__(kT) void fc_wide(Grid g, const Pt* __restrict__ sorted, const unsigned* __restrict__ starts,
                                              const Tri* __restrict__ recs, const int32_t* __restrict__ wide, int64_t n_faces,
                                              float* __restrict__ dist2, int32_t* __restrict__ index, float* __restrict__ weights,
                                              float* __restrict__ diff, FacecloudSmall* __restrict__ sm) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kT / kWave);
    int64_t n_wide = sm->wide;                 // written by fc_classify, the launch before this one
    n_wide = n_wide > n_faces ? n_faces : n_wide;
    uint32_t ntests = 0;
    int ring = 0;
    for (int64_t k = (int64_t)blockIdx.x * (kT / kWave) + threadIdx.x / kWave; k < n_wide; k += waves) {      // wave-uniform
        const int64_t f = wide[k];
        if (f < 0 || f >= n_faces) continue;
        const Tri t = recs[f];
        const Walk w = r3g_fc::walk_setup(g, t);
        Best b = r3g_fc::best_none();
        int r = 0;
        for (;; ++r) {
            r3g_fc::wide_ring_lane(g, sorted, starts, w, t, r, lane, b, ntests);
            b = wave_best(b);
            if (r3g_fc::walk_ends(g, w, r, b.d)) break;
        }
        ring = r > ring ? r : ring;
        if (lane == 0) r3g_fc::finish(t, b, dist2 + f, index + f, weights + 3 * f, diff + 3 * f);
    }
    wave_report(ntests, ring, sm);
}

__global__ __launch_bounds__(kT) void fc_gather(const float* __restrict__ grad_dist2, const int32_t* __restrict__ index,
                                                const float* __restrict__ weights, const float* __restrict__ diff,
                                                const int32_t* __restrict__ corner_start, const int32_t* __restrict__ corner_ids, int64_t n_verts,
                                                int64_t n_corners, float* __restrict__ grad_verts) {
    const int64_t v = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (v >= n_verts) return;
    r3g_fc::gather_vertex(grad_dist2, index, weights, diff, corner_ids, corner_start[v], corner_start[v + 1], n_corners, grad_verts + 3 * v);
}

}  // namespace

static_assert(sizeof(Tri) == 48 && sizeof(Pt) == 16, "three and one 16-byte loads");

size_t facecloud_workspace_bytes(int64_t n_faces, FacecloudLayout* lay) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    lay->off_small = o, o += up(sizeof(FacecloudSmall));
    lay->off_recs = o, o += up(sizeof(Tri) * (size_t)n_faces);
    lay->off_wide = o, o += up(4 * (size_t)n_faces);
    lay->total = o;
    return o;
}

hipError_t facecloud_classify(char* ws, const FacecloudLayout& lay, const Grid& g, const float* verts, int64_t n_verts, const int32_t* tri,
                              int64_t n_faces, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small, 0, sizeof(FacecloudSmall), s));
    hipLaunchKernelGGL(fc_classify, dim3(nblocks(n_faces, kT)), dim3(kT), 0, s, g, verts, n_verts, tri, n_faces, (Tri*)(ws + lay.off_recs),
                       (int32_t*)(ws + lay.off_wide), (FacecloudSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t facecloud_narrow(char* ws, const FacecloudLayout& lay, const Grid& g, const Pt* sorted, const unsigned* starts, int64_t n_faces,
                            float* dist2, int32_t* index, float* weights, float* diff, hipStream_t s) {
    hipLaunchKernelGGL(fc_narrow, dim3(nblocks(n_faces, kT)), dim3(kT), 0, s, g, sorted, starts, (const Tri*)(ws + lay.off_recs), n_faces, dist2,
                       index, weights, diff, (FacecloudSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t facecloud_wide(char* ws, const FacecloudLayout& lay, const Grid& g, const Pt* sorted, const unsigned* starts, int64_t n_faces,
                          float* dist2, int32_t* index, float* weights, float* diff, hipStream_t s) {
    const unsigned most = nblocks(n_faces, kT / kWave);
    hipLaunchKernelGGL(fc_wide, dim3(most > kWideBlocksMost ? kWideBlocksMost : most), dim3(kT), 0, s, g, sorted, starts,
                       (const Tri*)(ws + lay.off_recs), (const int32_t*)(ws + lay.off_wide), n_faces, dist2, index, weights, diff,
                       (FacecloudSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t facecloud_gather(const float* grad_dist2, const int32_t* index, const float* weights, const float* diff, const int32_t* corner_start,
                            const int32_t* corner_ids, int64_t n_verts, int64_t n_faces, float* grad_verts, hipStream_t s) {
    if (!n_verts) return hipSuccess;
    hipLaunchKernelGGL(fc_gather, dim3(nblocks(n_verts, kT)), dim3(kT), 0, s, grad_dist2, index, weights, diff, corner_start, corner_ids, n_verts,
                       3 * n_faces, grad_verts);
    return hipGetLastError();
}

}  // namespace r3g
