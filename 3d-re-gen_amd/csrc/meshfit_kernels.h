// meshfit_kernels.h -- host-side interface of meshfit_kernels.hip (internal to libr3g.so): closest points and the fused
// step of the mesh registration, both against the grid of the last r3g_meshdist_build
#ifndef R3G_MESHFIT_KERNELS_H
#define R3G_MESHFIT_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "meshdist_kernels.h"

namespace r3g {

// what a step leaves at the start of its workspace and what is read back: the sums in the fixed order of the reduction,
// then the integer counts (integer sums: no order to fix)
struct MeshfitRecord {
    double sums[38];                // fit_terms(mode) of them in use
    unsigned long long used;        // points that took part
    unsigned long long tests;       // point-triangle tests of the walk
};

// one MeshfitRecord for the result, then one per block
inline size_t meshfit_workspace_bytes() { return sizeof(MeshfitRecord) * (size_t)(1 + r3g_md::kFitMaxBlocks); }

// dist2 [n], face [n], closest [n][3] (GridCsrSmall::tests of the distance workspace receives the test count)
hipError_t meshfit_closest(char* md_ws, const GridCsrLayout& lay, const r3g_md::Grid& g, const int32_t* pairs, const float* points,
                           int64_t n, float* dist2, int32_t* face, float* closest, hipStream_t s);
// one accumulation: fit_blocks(n) partial records, then their sum into the first record of `ws`
hipError_t meshfit_step(char* ws, const char* md_ws, const GridCsrLayout& lay, const r3g_md::Grid& g, const int32_t* pairs,
                        const float* points, int64_t n, const float* weights, const r3g_md::Sim& x, int mode, float md2, hipStream_t s);

}  // namespace r3g
#endif
