// surf_compact_kernels.h -- host-side interface of the compaction skeleton that marching cubes and dual marching cubes
// share (internal to libr3g.so): the workspace of a count pass, what the context keeps between count and emit, and the
// block-sum scan of surf_compact_kernels.hip.  The device half is surf_compact_device.h.
#ifndef R3G_SURF_COMPACT_KERNELS_H
#define R3G_SURF_COMPACT_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dev_buf.h"

namespace r3g {

// small | blk | blkoff | nz | act | table, each aligned to 256 B
struct SurfWorkspaceLayout {
    uint32_t nblk, nchunk, ncells;
    uint32_t nnz;                     // non-empty blocks: filled in by the caller from totals[2] after the count pass
    uint64_t off_small, small_bytes;  // status(u32) @0, totals {nV, nF or nQ, nNZ} (3 x u64) @16, chunk sums @64, chunk nz after them
    uint64_t zero_bytes;              // small + blk: for a classify kernel that writes only the non-empty entries of blk
    uint64_t off_blk, off_blkoff, off_nz, off_act;
    uint64_t off_table;               // the extractor's own table between its two emit kernels (table_bytes, never initialised)
};

size_t surf_workspace_bytes(int n0, int n1, int n2, uint64_t table_bytes, SurfWorkspaceLayout* lay);

inline unsigned* surf_status(char* ws, const SurfWorkspaceLayout& lay) { return (unsigned*)(ws + lay.off_small); }
inline unsigned long long* surf_totals(char* ws, const SurfWorkspaceLayout& lay) { return (unsigned long long*)(ws + lay.off_small + 16); }
inline unsigned long long* surf_chunk_sums(char* ws, const SurfWorkspaceLayout& lay) { return (unsigned long long*)(ws + lay.off_small + 64); }
inline unsigned* surf_chunk_nz(char* ws, const SurfWorkspaceLayout& lay) { return (unsigned*)(ws + lay.off_small + 64 + 8 * (size_t)lay.nchunk); }

// K2: exclusive scan of the block sums (one workgroup per 1024-block chunk), the list of non-empty blocks, the totals
hipError_t surf_scan_launch(char* ws, const SurfWorkspaceLayout& lay, hipStream_t stream);

// what an extractor keeps in the context between its count and its emit
struct SurfState {
    DevBuf ws;
    SurfWorkspaceLayout lay{};
    const float* grid = nullptr;
    int n[3] = {0, 0, 0};
    double level = 0.0;
    bool counted = false;
};

}  // namespace r3g
#endif
