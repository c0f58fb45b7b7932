// mc_kernels.h -- host-side launch interface of mc_kernels.hip (internal to libr3g.so)
#ifndef R3G_MC_KERNELS_H
#define R3G_MC_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "options.h"
#include "surf_compact_kernels.h"

namespace r3g {

extern const Option g_mc_options[];   // the "mc_*" switches
size_t mc_workspace_bytes(int n0, int n1, int n2, SurfWorkspaceLayout* lay);

// K1 + K2 (surf_scan_launch).  After the stream drains: status word at ws+off_small, totals {nV, nF, nNZ} at +16.
hipError_t mc_count_launch(const float* grid, int n0, int n1, int n2, double level, int classic, char* ws,
                           const SurfWorkspaceLayout& lay, hipStream_t stream);

// K3 + K4.  xf9 = {grid_size[3], bbox_size[3], bbox_min[3]} or null (index-space vertices).
hipError_t mc_emit_launch(const float* grid, int n0, int n1, int n2, double level, char* ws,
                          const SurfWorkspaceLayout& lay, float* verts, int32_t* faces, const double* xf9,
                          int reversed, hipStream_t stream);

}  // namespace r3g
#endif
