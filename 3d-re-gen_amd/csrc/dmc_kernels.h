// dmc_kernels.h -- host-side launch interface of dmc_kernels.hip (internal to libr3g.so)
#ifndef R3G_DMC_KERNELS_H
#define R3G_DMC_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace r3g {

struct DmcWorkspaceLayout {
    uint32_t nblk, nchunk, ncells;
    uint32_t nnz;                     // non-empty blocks: filled in by the caller from totals[2] after the count pass
    uint64_t off_small, small_bytes;  // status(u32) @0, totals {nV, nQ, nNZ} (3 x u64) @16, chunk sums @64; zeroed per call
    uint64_t off_blk, off_blkoff, off_nz, off_act, off_ctab;
};

size_t dmc_workspace_bytes(int n0, int n1, int n2, DmcWorkspaceLayout* lay);

// classify + scan.  After the stream drains: status word at ws+off_small, totals {nV, nQ, nNZ} at +16.
hipError_t dmc_count_launch(const float* grid, int n0, int n1, int n2, double level, int manifold, char* ws,
                            const DmcWorkspaceLayout& lay, hipStream_t stream);

// vertices + quads.  xf9 = {grid_size[3], bbox_size[3], bbox_min[3]} or null (index-space vertices).
hipError_t dmc_emit_launch(const float* grid, int n0, int n1, int n2, double level, char* ws,
                           const DmcWorkspaceLayout& lay, float* verts, int32_t* faces, const double* xf9,
                           int reversed, hipStream_t stream);

}  // namespace r3g
#endif
