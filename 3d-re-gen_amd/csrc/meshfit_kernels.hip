// meshfit_kernels.hip -- closest points and the fused step of the mesh registration, on the grid
// that meshdist_kernels.hip builds.
//
// mf_closest: one lane per point, the ring walk of meshdist_core.h, then tri_closest on the winning face.
// mf_step<MODE>: one lane per point (several, in index order, beyond kFitMaxBlocks * kFitBlock points): move the point by
// the current similarity, walk, closest point, and add the point's terms (fit_point) to the lane's float64 sums.
// Reduction, in one fixed order: the wave butterfly (xor 32, 16, 8, 4, 2, 1), the block's four waves in index order through
// LDS, one record per block written with ordinary stores; mf_final, one block, then gives lane t the records t, t + 256, ...
// in index order and runs the same tree.  No floating-point atomics, and no integer ones either: the counts go the same way.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_GRID_HD static __host__ __device__ __forceinline__
#define R3G_MD_HD static __host__ __device__ __forceinline__
#include "mesh_launch.h"
#include "meshfit_kernels.h"

namespace r3g {
namespace {

using r3g_md::Grid;
using r3g_md::Sim;
using r3g_md::Tri;

__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(kT) void mf_closest(Grid g, const Tri* __restrict__ tris, const unsigned* __restrict__ starts,
                                                 const int32_t* __restrict__ pairs, const float* __restrict__ pts, int64_t n,
                                                 float* __restrict__ dist2, int32_t* __restrict__ face, float* __restrict__ closest) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    float d, qx, qy, qz;
    int32_t f;
    uint32_t ntests = 0;
    r3g_md::nearest(g, tris, starts, pairs, px, py, pz, &d, &f, &ntests);
    if (f >= 0) {
        d = r3g_md::tri_closest(px, py, pz, tris[f], &qx, &qy, &qz);     // the same bits as the walk's tri_dist2
    } else {
        d = qx = qy = qz = r3g_md::quiet_nan();
    }
    dist2[i] = d;
    face[i] = f;
    closest[3 * i] = qx, closest[3 * i + 1] = qy, closest[3 * i + 2] = qz;
}

template <int MODE>
__global__ __launch_bounds__(kT) void mf_step(Grid g, const Tri* __restrict__ tris, const unsigned* __restrict__ starts,
                                              const int32_t* __restrict__ pairs, const float* __restrict__ pts, int64_t n,
                                              const float* __restrict__ weights, Sim x, float md2, MeshfitRecord* __restrict__ partial) {
    constexpr int K = MODE == r3g_md::kFitPlane ? r3g_md::kFitPlaneTerms : r3g_md::kFitPointTerms;
    __shared__ double sh[4][K];
    __shared__ unsigned long long shi[4][2];
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    unsigned long long used = 0, tests = 0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
        uint32_t u = 0, nt = 0;
        r3g_md::fit_point<MODE>(g, tris, starts, pairs, x, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], weights ? weights[i] : 1.0f,
                                md2, acc, &u, &nt);
        used += u;
        tests += nt;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum_f64(acc[k]);
        if (lane == 0) sh[wave][k] = v;
    }
    used = wave_sum_u64(used);
    tests = wave_sum_u64(tests);
    if (lane == 0) shi[wave][0] = used, shi[wave][1] = tests;
    __syncthreads();
    MeshfitRecord* out = partial + blockIdx.x;
    if (threadIdx.x < K) out->sums[threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
    if (threadIdx.x == 64) out->used = shi[0][0] + shi[1][0] + shi[2][0] + shi[3][0];
    if (threadIdx.x == 65) out->tests = shi[0][1] + shi[1][1] + shi[2][1] + shi[3][1];
}

// one block: lane t sums the records t, t + 256, ... in index order, then the tree of mf_step
__global__ __launch_bounds__(kT) void mf_final(const MeshfitRecord* __restrict__ partial, int nb, int K, MeshfitRecord* __restrict__ out) {
    __shared__ double sh[4][r3g_md::kFitMaxTerms];
    __shared__ unsigned long long shi[4][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = 0; k < K; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nb; b += kT) v = v + partial[b].sums[k];
        v = wave_sum_f64(v);
        if (lane == 0) sh[wave][k] = v;
    }
    unsigned long long used = 0, tests = 0;
    for (int b = threadIdx.x; b < nb; b += kT) used += partial[b].used, tests += partial[b].tests;
    used = wave_sum_u64(used);
    tests = wave_sum_u64(tests);
    if (lane == 0) shi[wave][0] = used, shi[wave][1] = tests;
    __syncthreads();
    if (threadIdx.x < 38)
        out->sums[threadIdx.x] = (int)threadIdx.x < K ? ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x] : 0.0;
    if (threadIdx.x == 64) out->used = shi[0][0] + shi[1][0] + shi[2][0] + shi[3][0];
    if (threadIdx.x == 65) out->tests = shi[0][1] + shi[1][1] + shi[2][1] + shi[3][1];
}

}  // namespace

static_assert(sizeof(MeshfitRecord) == 8 * r3g_md::kFitRecord, "a partial record is kFitRecord 8-byte slots");
static_assert(r3g_md::kFitMaxTerms <= 38 && r3g_md::kFitBlock == kT, "the sums fit the record; the tree is four waves");

hipError_t meshfit_closest(char* md_ws, const GridCsrLayout& lay, const Grid& g, const int32_t* pairs, const float* points, int64_t n,
                           float* dist2, int32_t* face, float* closest, hipStream_t s) {
    hipLaunchKernelGGL(mf_closest, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, s, g, (const Tri*)(md_ws + lay.off_recs),
                       (const unsigned*)(md_ws + lay.off_starts), pairs, points, n, dist2, face, closest);
    return hipGetLastError();
}

hipError_t meshfit_step(char* ws, const char* md_ws, const GridCsrLayout& lay, const Grid& g, const int32_t* pairs, const float* points,
                        int64_t n, const float* weights, const Sim& x, int mode, float md2, hipStream_t s) {
    MeshfitRecord* rec = (MeshfitRecord*)ws;
    const unsigned nb = (unsigned)r3g_md::fit_blocks(n);
    const Tri* tris = (const Tri*)(md_ws + lay.off_recs);
    const unsigned* starts = (const unsigned*)(md_ws + lay.off_starts);
    if (mode == r3g_md::kFitPlane)
        hipLaunchKernelGGL(mf_step<r3g_md::kFitPlane>, dim3(nb), dim3(kT), 0, s, g, tris, starts, pairs, points, n, weights, x, md2, rec + 1);
    else
        hipLaunchKernelGGL(mf_step<r3g_md::kFitPoint>, dim3(nb), dim3(kT), 0, s, g, tris, starts, pairs, points, n, weights, x, md2, rec + 1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mf_final, dim3(1), dim3(kT), 0, s, (const MeshfitRecord*)(rec + 1), (int)nb, r3g_md::fit_terms(mode), rec);
    return hipGetLastError();
}

}  // namespace r3g
