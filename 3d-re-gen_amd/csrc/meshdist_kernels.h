// meshdist_kernels.h -- host-side interface of meshdist_kernels.hip (internal to libr3g.so)
#ifndef R3G_MESHDIST_KERNELS_H
#define R3G_MESHDIST_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "grid_csr_kernels.h"
#include "meshdist_core.h"

namespace r3g {

// (the workspace: grid_csr_workspace_bytes with this record)
// validate the indices, copy the faces into padded records, bounding box and `skipped` into GridCsrSmall
hipError_t meshdist_records(char* ws, const GridCsrLayout& lay, const float* verts, int64_t nv, const int32_t* faces,
                            int64_t nf, hipStream_t s);
// GridCsrSmall::pairs for grid g (touches no cell)
hipError_t grid_csr_count_pairs(char* ws, const GridCsrLayout& lay, int64_t nf, const r3g_md::Grid& g, hipStream_t s);
// per-cell counts -> exclusive scan -> fill of pairs [GridCsrSmall::pairs] with face ids
hipError_t grid_csr_fill(char* ws, const GridCsrLayout& lay, int64_t nf, const r3g_md::Grid& g, int32_t* pairs, hipStream_t s);
hipError_t meshdist_query(char* ws, const GridCsrLayout& lay, const r3g_md::Grid& g, const int32_t* pairs, const float* points,
                          int64_t n, float* dist2, int32_t* face, hipStream_t s);

}  // namespace r3g
#endif
