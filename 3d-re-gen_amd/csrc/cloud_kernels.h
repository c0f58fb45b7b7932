// cloud_kernels.h -- host-side interface of cloud_kernels.hip (internal to libr3g.so)
#ifndef R3G_CLOUD_KERNELS_H
#define R3G_CLOUD_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cloud_core.h"
#include "grid_csr_kernels.h"

namespace r3g {

// (the workspace: grid_csr_workspace_bytes with the 16-byte record r3g_cl::Pt)
// copy the points into packed records (index -1: a non-finite coordinate), bounding box and `skipped` into GridCsrSmall
hipError_t cloud_records(char* ws, const GridCsrLayout& lay, const float* points, int64_t n, hipStream_t s);
// per-cell counts -> exclusive scan -> the usable records into sorted [n - skipped] in cell order
hipError_t cloud_fill(char* ws, const GridCsrLayout& lay, int64_t n, const r3g_cl::Grid& g, r3g_cl::Pt* sorted, hipStream_t s);
// dist2 [n][k], index [n][k]; k in [1, kMaxK]
hipError_t cloud_knn(char* ws, const GridCsrLayout& lay, const r3g_cl::Grid& g, const r3g_cl::Pt* sorted, const float* queries,
                     int64_t n, int k, float* dist2, int32_t* index, hipStream_t s);

}  // namespace r3g
#endif
