// meshdist_kernels.hip -- exact nearest-triangle query on a uniform grid in CSR form.
//
// Build: records (index check, padded copies, bounding box), then the shared builder of grid_csr_device.h.  Query: one lane
// per point walks its own Chebyshev rings (meshdist_core.h).  The order of the faces inside a cell, which the builder leaves
// open, is absorbed by the (dist2, face) comparison.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_GRID_HD static __host__ __device__ __forceinline__
#define R3G_MD_HD static __host__ __device__ __forceinline__
#include "grid_csr_device.h"
#include "meshdist_kernels.h"

namespace r3g {
namespace {

using r3g_md::Grid;
using r3g_md::Tri;

__global__ __launch_bounds__(kT) void md_records(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ faces,
                                                 int64_t nf, Tri* __restrict__ tris, GridCsrSmall* __restrict__ sm) {
    float lo[3] = {r3g_md::kInf, r3g_md::kInf, r3g_md::kInf}, hi[3] = {-r3g_md::kInf, -r3g_md::kInf, -r3g_md::kInf};
    unsigned long long skipped = 0;
    bool bad = false;
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        Tri t;
        t.valid = 0;
        t.pad1 = t.pad2 = 0;
        t.ax = t.ay = t.az = t.bx = t.by = t.bz = t.cx = t.cy = t.cz = 0.0f;
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) {
            bad = true;                                   // nothing is read through a bad index
        } else {
            t.ax = verts[3 * (int64_t)i0], t.ay = verts[3 * (int64_t)i0 + 1], t.az = verts[3 * (int64_t)i0 + 2];
            t.bx = verts[3 * (int64_t)i1], t.by = verts[3 * (int64_t)i1 + 1], t.bz = verts[3 * (int64_t)i1 + 2];
            t.cx = verts[3 * (int64_t)i2], t.cy = verts[3 * (int64_t)i2 + 1], t.cz = verts[3 * (int64_t)i2 + 2];
            if (r3g_md::tri_finite(t)) {
                t.valid = 1;
                float mn[3], mx[3];
                r3g_md::grid_box(t, mn, mx);
                for (int a = 0; a < 3; ++a) lo[a] = r3g_grid::fmin2(lo[a], mn[a]), hi[a] = r3g_grid::fmax2(hi[a], mx[a]);
            } else {
                ++skipped;
            }
        }
        tris[f] = t;
    }
    csr_records_reduce<3>(lo, hi, skipped, bad, sm);
}

__global__ __launch_bounds__(kT) void md_query(Grid g, const Tri* __restrict__ tris, const unsigned* __restrict__ starts,
                                               const int32_t* __restrict__ pairs, const float* __restrict__ pts, int64_t n,
                                               float* __restrict__ dist2, int32_t* __restrict__ face, GridCsrSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    uint32_t ntests = 0;
    if (i < n) {
        float d;
        int32_t f;
        r3g_md::nearest(g, tris, starts, pairs, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], &d, &f, &ntests);
        dist2[i] = d;
        face[i] = f;
    }
    const unsigned long long t = wave_sum_u64((unsigned long long)ntests);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(&sm->tests, t);
}

}  // namespace

static_assert(sizeof(Tri) == 48, "triangle records are three 16-byte loads");

hipError_t meshdist_records(char* ws, const GridCsrLayout& lay, const float* verts, int64_t nv, const int32_t* faces,
                            int64_t nf, hipStream_t s) {
    R3G_HIP(csr_records_begin<3>(ws, lay, s));
    hipLaunchKernelGGL(md_records, dim3(grid_for(nf)), dim3(kT), 0, s, verts, nv, faces, nf, (Tri*)(ws + lay.off_recs),
                       (GridCsrSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t grid_csr_count_pairs(char* ws, const GridCsrLayout& lay, int64_t nf, const Grid& g, hipStream_t s) {
    return csr_count_pairs_launch<3, Tri>(ws, lay, nf, g, s);
}

hipError_t grid_csr_fill(char* ws, const GridCsrLayout& lay, int64_t nf, const Grid& g, int32_t* pairs, hipStream_t s) {
    return csr_fill_launch<3, Tri>(ws, lay, nf, g, pairs, s);
}

hipError_t meshdist_query(char* ws, const GridCsrLayout& lay, const Grid& g, const int32_t* pairs, const float* points,
                          int64_t n, float* dist2, int32_t* face, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(GridCsrSmall, tests), 0, 8, s));
    hipLaunchKernelGGL(md_query, dim3(nblocks(n, kT)), dim3(kT), 0, s, g, (const Tri*)(ws + lay.off_recs),
                       (const unsigned*)(ws + lay.off_starts), pairs, points, n, dist2, face, (GridCsrSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

}  // namespace r3g
