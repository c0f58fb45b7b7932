// cloud_kernels.hip -- exact k nearest neighbours between point clouds on a uniform grid.
//
// Build: records (packed 16-byte copies with the original index, bounding box), then the home-cell builder of
// grid_csr_device.h, which moves the usable records into cell order: a cell is a run of aligned 16-byte loads.
// Query: one lane per query point walks its own Chebyshev rings (cloud_core.h).  k == 1 keeps its pair in registers; a
// larger k keeps each lane's sorted list in LDS, laid out [slot][lane]: slot j of lane l is dword j * lanes + l, so the
// lanes of a wave hit distinct banks whichever slots they are at, and no register array is indexed dynamically.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_GRID_HD static __host__ __device__ __forceinline__
#define R3G_MD_HD static __host__ __device__ __forceinline__
#define R3G_CL_HD static __host__ __device__ __forceinline__
#define R3G_CL_HD_MEMBER __host__ __device__ __forceinline__
#include "cloud_kernels.h"
#include "grid_csr_device.h"

namespace r3g {
namespace {

using r3g_cl::Grid;
using r3g_cl::Pt;

// lanes per block of the query: the lists of a block take k * lanes * 8 bytes of LDS, at most 32 KiB either way, so at
// least two blocks (five, by LDS alone) fit the 160 KiB of a CU
constexpr int kLanesSmallK = 256, kLanesLargeK = 128, kSmallK = 16;
static_assert(kSmallK * kLanesSmallK * 8 <= 32768 && r3g_cl::kMaxK * kLanesLargeK * 8 <= 32768, "the lists of a block");

__global__ __launch_bounds__(kT) void cl_records(const float* __restrict__ points, int64_t n, Pt* __restrict__ recs,
                                                 GridCsrSmall* __restrict__ sm) {
    float lo[3] = {r3g_cl::kInf, r3g_cl::kInf, r3g_cl::kInf}, hi[3] = {-r3g_cl::kInf, -r3g_cl::kInf, -r3g_cl::kInf};
    unsigned long long skipped = 0;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
        Pt p;
        p.x = points[3 * i], p.y = points[3 * i + 1], p.z = points[3 * i + 2];
        p.index = (int32_t)i;
        if (r3g_cl::pt_finite(p.x, p.y, p.z)) {
            lo[0] = r3g_grid::fmin2(lo[0], p.x), lo[1] = r3g_grid::fmin2(lo[1], p.y), lo[2] = r3g_grid::fmin2(lo[2], p.z);
            hi[0] = r3g_grid::fmax2(hi[0], p.x), hi[1] = r3g_grid::fmax2(hi[1], p.y), hi[2] = r3g_grid::fmax2(hi[2], p.z);
        } else {
            p.x = p.y = p.z = 0.0f;
            p.index = -1;
            ++skipped;
        }
        recs[i] = p;
    }
    csr_records_reduce<3>(lo, hi, skipped, false, sm);
}

// a lane's k-list in LDS: d and i point at the lane's slot 0
struct LdsStore {
    float* d;
    int32_t* i;
    int stride;
    __device__ __forceinline__ float get_d(int j) const { return d[j * stride]; }
    __device__ __forceinline__ int32_t get_i(int j) const { return i[j * stride]; }
    __device__ __forceinline__ void set(int j, float v, int32_t x) { d[j * stride] = v, i[j * stride] = x; }
};

template <bool K1, int LANES>
__global__ __launch_bounds__(LANES) void cl_knn(Grid g, const Pt* __restrict__ sorted, const unsigned* __restrict__ starts,
                                                const float* __restrict__ queries, int64_t n, int k, float* __restrict__ dist2,
                                                int32_t* __restrict__ index, GridCsrSmall* __restrict__ sm) {
    extern __shared__ float lds[];      // K1: none.  Otherwise float [k][LANES], then int32 [k][LANES]
    const int64_t i = (int64_t)blockIdx.x * LANES + threadIdx.x;
    uint32_t ntests = 0;
    if (i < n) {
        const float px = queries[3 * i], py = queries[3 * i + 1], pz = queries[3 * i + 2];
        if (K1) {
            r3g_cl::NoStore st;
            r3g_cl::knn<true>(g, sorted, starts, px, py, pz, 1, st, dist2 + i, index + i, &ntests);
        } else {
            LdsStore st{lds + threadIdx.x, (int32_t*)(lds + k * LANES) + threadIdx.x, LANES};
            r3g_cl::knn<false>(g, sorted, starts, px, py, pz, k, st, dist2 + i * k, index + i * k, &ntests);
        }
    }
    const unsigned long long t = wave_sum_u64((unsigned long long)ntests);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(&sm->tests, t);
}

}  // namespace

static_assert(sizeof(Pt) == 16, "a target point is one 16-byte load");

hipError_t cloud_records(char* ws, const GridCsrLayout& lay, const float* points, int64_t n, hipStream_t s) {
    R3G_HIP(csr_records_begin<3>(ws, lay, s));
    hipLaunchKernelGGL(cl_records, dim3(grid_for(n)), dim3(kT), 0, s, points, n, (Pt*)(ws + lay.off_recs),
                       (GridCsrSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t cloud_fill(char* ws, const GridCsrLayout& lay, int64_t n, const Grid& g, Pt* sorted, hipStream_t s) {
    return csr_fill_home_launch<3, Pt>(ws, lay, n, g, sorted, s);
}

hipError_t cloud_knn(char* ws, const GridCsrLayout& lay, const Grid& g, const Pt* sorted, const float* queries, int64_t n, int k,
                     float* dist2, int32_t* index, hipStream_t s) {
    if (k < 1 || k > r3g_cl::kMaxK) return hipErrorInvalidValue;
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(GridCsrSmall, tests), 0, 8, s));
    const unsigned* starts = (const unsigned*)(ws + lay.off_starts);
    GridCsrSmall* sm = (GridCsrSmall*)(ws + lay.off_small);
    if (k == 1)
        hipLaunchKernelGGL((cl_knn<true, kLanesSmallK>), dim3(nblocks(n, kLanesSmallK)), dim3(kLanesSmallK), 0, s, g, sorted, starts,
                           queries, n, k, dist2, index, sm);
    else if (k <= kSmallK)
        hipLaunchKernelGGL((cl_knn<false, kLanesSmallK>), dim3(nblocks(n, kLanesSmallK)), dim3(kLanesSmallK),
                           (size_t)k * kLanesSmallK * 8, s, g, sorted, starts, queries, n, k, dist2, index, sm);
    else
        hipLaunchKernelGGL((cl_knn<false, kLanesLargeK>), dim3(nblocks(n, kLanesLargeK)), dim3(kLanesLargeK),
                           (size_t)k * kLanesLargeK * 8, s, g, sorted, starts, queries, n, k, dist2, index, sm);
    return hipGetLastError();
}

}  // namespace r3g
