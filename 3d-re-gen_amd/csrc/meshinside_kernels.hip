// meshinside_kernels.hip -- ray-crossing count against a grid of columns in CSR form.
//
// Build: records (index check, projected padded copies, usability, projected bounding box), then the shared builder of
// grid_csr_device.h.  Query: one lane per point sums the crossings of the faces listed in its column (meshinside_core.h).
// The order of the faces inside a column, which the builder leaves open, only permutes the terms of an integer sum.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_GRID_HD static __host__ __device__ __forceinline__
#define R3G_MI_HD static __host__ __device__ __forceinline__
#include "grid_csr_device.h"
#include "meshinside_kernels.h"

namespace r3g {
namespace {

using r3g_mi::Grid2;
using r3g_mi::Rec;

__global__ __launch_bounds__(kT) void mi_records(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ faces,
                                                 int64_t nf, int axis, Rec* __restrict__ recs, GridCsrSmall* __restrict__ sm) {
    float lo[2] = {r3g_mi::kInf, r3g_mi::kInf}, hi[2] = {-r3g_mi::kInf, -r3g_mi::kInf};
    unsigned long long skipped = 0;
    bool bad = false;
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        Rec r;
        r.au = r.av = r.aw = r.bu = r.bv = r.bw = r.cu = r.cv = r.cw = 0.0f;
        r.ia = -1, r.ib = r.ic = 0;
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) {
            bad = true;                                   // nothing is read through a bad index
        } else {
            const float a[3] = {verts[3 * (int64_t)i0], verts[3 * (int64_t)i0 + 1], verts[3 * (int64_t)i0 + 2]};
            const float b[3] = {verts[3 * (int64_t)i1], verts[3 * (int64_t)i1 + 1], verts[3 * (int64_t)i1 + 2]};
            const float c[3] = {verts[3 * (int64_t)i2], verts[3 * (int64_t)i2 + 1], verts[3 * (int64_t)i2 + 2]};
            r = r3g_mi::make_rec(a, i0, b, i1, c, i2, axis);
            if (r3g_mi::rec_finite(r)) {
                float mn[2], mx[2];
                r3g_mi::grid_box(r, mn, mx);
                for (int k = 0; k < 2; ++k) lo[k] = r3g_grid::fmin2(lo[k], mn[k]), hi[k] = r3g_grid::fmax2(hi[k], mx[k]);
                if (!r3g_mi::rec_usable(r)) r.ia = -1;     // zero projected area: takes part in nothing
            } else {
                ++skipped;
                r.ia = -1;
            }
        }
        recs[f] = r;
    }
    csr_records_reduce<2>(lo, hi, skipped, bad, sm);
}

__global__ __launch_bounds__(kT) void mi_query(Grid2 g, int axis, const Rec* __restrict__ recs, const unsigned* __restrict__ starts,
                                               const int32_t* __restrict__ pairs, const float* __restrict__ pts, int64_t n,
                                               int32_t* __restrict__ count, GridCsrSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    uint32_t ntests = 0;
    if (i < n) count[i] = r3g_mi::count_crossings(g, axis, recs, starts, pairs, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], &ntests);
    const unsigned long long t = wave_sum_u64((unsigned long long)ntests);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(&sm->tests, t);
}

}  // namespace

static_assert(sizeof(Rec) == 48, "face records are three 16-byte loads");

hipError_t meshinside_records(char* ws, const GridCsrLayout& lay, const float* verts, int64_t nv, const int32_t* faces,
                              int64_t nf, int axis, hipStream_t s) {
    R3G_HIP(csr_records_begin<2>(ws, lay, s));
    hipLaunchKernelGGL(mi_records, dim3(grid_for(nf)), dim3(kT), 0, s, verts, nv, faces, nf, axis, (Rec*)(ws + lay.off_recs),
                       (GridCsrSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t grid_csr_count_pairs(char* ws, const GridCsrLayout& lay, int64_t nf, const Grid2& g, hipStream_t s) {
    return csr_count_pairs_launch<2, Rec>(ws, lay, nf, g, s);
}

hipError_t grid_csr_fill(char* ws, const GridCsrLayout& lay, int64_t nf, const Grid2& g, int32_t* pairs, hipStream_t s) {
    return csr_fill_launch<2, Rec>(ws, lay, nf, g, pairs, s);
}

hipError_t meshinside_query(char* ws, const GridCsrLayout& lay, const Grid2& g, int axis, const int32_t* pairs,
                            const float* points, int64_t n, int32_t* count, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(GridCsrSmall, tests), 0, 8, s));
    hipLaunchKernelGGL(mi_query, dim3(nblocks(n, kT)), dim3(kT), 0, s, g, axis, (const Rec*)(ws + lay.off_recs),
                       (const unsigned*)(ws + lay.off_starts), pairs, points, n, count, (GridCsrSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

}  // namespace r3g
