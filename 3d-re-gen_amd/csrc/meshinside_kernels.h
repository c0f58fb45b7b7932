// meshinside_kernels.h -- host-side interface of meshinside_kernels.hip (internal to libr3g.so)
#ifndef R3G_MESHINSIDE_KERNELS_H
#define R3G_MESHINSIDE_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "grid_csr_kernels.h"
#include "meshinside_core.h"

namespace r3g {

// (the workspace: grid_csr_workspace_bytes with this record)
// validate the indices, project the faces into padded records (unusable ones marked), projected bounding box and
// `skipped` into GridCsrSmall
hipError_t meshinside_records(char* ws, const GridCsrLayout& lay, const float* verts, int64_t nv, const int32_t* faces,
                              int64_t nf, int axis, hipStream_t s);
// GridCsrSmall::pairs for grid g (touches no column)
hipError_t grid_csr_count_pairs(char* ws, const GridCsrLayout& lay, int64_t nf, const r3g_mi::Grid2& g, hipStream_t s);
// per-column counts -> exclusive scan -> fill of pairs [GridCsrSmall::pairs] with face ids
hipError_t grid_csr_fill(char* ws, const GridCsrLayout& lay, int64_t nf, const r3g_mi::Grid2& g, int32_t* pairs, hipStream_t s);
hipError_t meshinside_query(char* ws, const GridCsrLayout& lay, const r3g_mi::Grid2& g, int axis, const int32_t* pairs,
                            const float* points, int64_t n, int32_t* count, hipStream_t s);

}  // namespace r3g
#endif
