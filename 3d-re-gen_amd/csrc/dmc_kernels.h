// dmc_kernels.h -- host-side launch interface of dmc_kernels.hip (internal to libr3g.so)
#ifndef R3G_DMC_KERNELS_H
#define R3G_DMC_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "surf_compact_kernels.h"

namespace r3g {

size_t dmc_workspace_bytes(int n0, int n1, int n2, SurfWorkspaceLayout* lay);

// classify + scan (surf_scan_launch).  After the stream drains: status word at ws+off_small, totals {nV, nQ, nNZ} at +16.
hipError_t dmc_count_launch(const float* grid, int n0, int n1, int n2, double level, int manifold, char* ws,
                            const SurfWorkspaceLayout& lay, hipStream_t stream);

// vertices + quads.  xf9 = {grid_size[3], bbox_size[3], bbox_min[3]} or null (index-space vertices).
hipError_t dmc_emit_launch(const float* grid, int n0, int n1, int n2, double level, char* ws,
                           const SurfWorkspaceLayout& lay, float* verts, int32_t* faces, const double* xf9,
                           int reversed, hipStream_t stream);

}  // namespace r3g
#endif
