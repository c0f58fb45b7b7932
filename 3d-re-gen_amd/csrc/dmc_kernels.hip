// dmc_kernels.hip -- dual marching cubes on gfx950 (HBM-bound index work, no MFMA).  Definition: DESIGN.md section 4c.
//
// One vertex per surface patch of a cell and one quad per crossed grid edge, read from the (R+1)^3 fp32 grid that stays
// in HBM.  Launch structure (cells linearised axis 2 fastest, 256 cells per block, as in mc_kernels.hip):
//   K1 dmc_classify : one thread per cell: case from the 8 corners, manifold rule from the neighbour across the
//                     tunnelling face (recomputed from the grid, rare), {patch count, quad count} -> per-block
//                     compacted records of the active cells with their in-block prefix, block sums, chunk sums.
//   K2 surf_scan    : exclusive scan of the block sums (one workgroup per 1024-block chunk) + the list of non-empty blocks
//                     (surf_compact_kernels.hip).
//   K3 dmc_vertices : one thread per ACTIVE cell: fp64 patch centroids, float32 store, cell table {first vertex, case}.
//   K4 dmc_quads    : one thread per ACTIVE cell: its up to three quads, vertex ids through the cell table of the four
//                     cells around the edge, diagonal chosen on the stored float32 positions.
// Every output position is block offset + in-block prefix, both from scans: nothing depends on the order workgroups run
// in, and the only atomics are integer adds on the chunk totals.  Only K1 touches the whole grid.
// The skeleton around the per-cell bodies -- block compaction at the end of K1, the scan, the workspace, the emit kernels'
// walk over the non-empty blocks -- is the one of marching cubes: surf_compact_device.h, surf_compact_kernels.{h,hip}.
//
// Built with -ffp-contract=off: centroid, output transform and diagonal test must not be fused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define R3G_DEV static __device__ __forceinline__
#define R3G_LUT_QUAL static __device__ const
#include "dmc_cell.h"
#include "dmc_kernels.h"
#include "prof.h"
#include "surf_compact_device.h"

#pragma clang fp contract(off)

using namespace r3g_dmc;
using namespace r3g_surf;

namespace {

__device__ __forceinline__ void cell_coords(uint32_t c, const Dims& d, int& i, int& j, int& k) {
    const uint32_t c2 = (uint32_t)(d.n2 - 1), c1 = (uint32_t)(d.n1 - 1);
    const uint32_t row = c / c2;
    k = (int)(c - row * c2);
    i = (int)(row / c1);
    j = (int)(row - (uint32_t)i * c1);
}

__global__ __launch_bounds__(kBlock) void dmc_classify(const float* __restrict__ grid, Dims d, uint32_t ncells, double level,
                                                       int manifold, uint2* __restrict__ act, uint4* __restrict__ blk,
                                                       unsigned long long* __restrict__ chunk_sums,
                                                       unsigned* __restrict__ chunk_nz, unsigned* __restrict__ status) {
    const int tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t c = b * kBlock + tid;
    unsigned flags = 0;
    int i = 0, j = 0, k = 0, cs = 0;
    if (c < ncells) {
        cell_coords(c, d, i, j, k);
        cs = cell_case(grid, d, i, j, k, level, &flags);
    }
    const bool active = cs != 0 && cs != 255;
    publish_range_flags(flags, status);
    // most blocks contain no surface cell: they publish zeros and leave
    if (!__syncthreads_or(active ? 1 : 0)) {
        if (tid == 0) blk[b] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const unsigned rec = active ? classify_cell(grid, d, i, j, k, level, cs, manifold != 0) : 0u;
    publish_block(rec, rec_patches(rec), rec_quads(rec), b, act, blk, chunk_sums, chunk_nz);
}

// K3 / K4, as mc_vertices / mc_faces: one thread per active cell, found through the shared EmitMap.
__global__ __launch_bounds__(kEmitWg) void dmc_vertices(const float* __restrict__ grid, Dims d, double level,
                                                       const uint2* __restrict__ act, const uint4* __restrict__ blk,
                                                       const uint2* __restrict__ blkoff, const uint32_t* __restrict__ nzlist,
                                                       uint32_t nnz, CellRef* __restrict__ ctab, float* __restrict__ verts,
                                                       Xform xf, int use_xf) {
    __shared__ EmitMap map;
    emit_map_build(&map, blk, nzlist, nnz);
    for (unsigned item = threadIdx.x;; item += kEmitWg) {
        uint32_t b;
        unsigned slot;
        if (!emit_map_find(&map, item, &b, &slot)) break;
        const uint32_t voff = blkoff[b].x;
        const uint2 a = act[(size_t)b * kBlock + slot];
        const uint32_t c = b * kBlock + (a.y & 0xFFu);
        int i, j, k;
        cell_coords(c, d, i, j, k);
        emit_cell_vertices(a.x, voff + ((a.y >> 8) & 0xFFFu), grid, d, i, j, k, level, (int64_t)c, ctab, verts, xf, use_xf != 0);
    }
}

__global__ __launch_bounds__(kEmitWg) void dmc_quads(Dims d, const uint2* __restrict__ act, const uint4* __restrict__ blk,
                                                    const uint2* __restrict__ blkoff, const uint32_t* __restrict__ nzlist,
                                                    uint32_t nnz, const CellRef* __restrict__ ctab,
                                                    const float* __restrict__ verts, int32_t* __restrict__ faces, int reversed) {
    __shared__ EmitMap map;
    emit_map_build(&map, blk, nzlist, nnz);
    for (unsigned item = threadIdx.x;; item += kEmitWg) {
        uint32_t b;
        unsigned slot;
        if (!emit_map_find(&map, item, &b, &slot)) break;
        const uint2 a = act[(size_t)b * kBlock + slot];
        if (rec_quads(a.x) == 0u) continue;
        const uint32_t c = b * kBlock + (a.y & 0xFFu);
        int i, j, k;
        cell_coords(c, d, i, j, k);
        emit_cell_quads(a.x, blkoff[b].y + (a.y >> 20), d, i, j, k, ctab, verts, faces, reversed != 0);
    }
}

}  // namespace

namespace r3g {

size_t dmc_workspace_bytes(int n0, int n1, int n2, SurfWorkspaceLayout* lay) {
    // cell table: written and read for active cells only, never initialised
    return surf_workspace_bytes(n0, n1, n2, sizeof(CellRef) * (uint64_t)(n0 - 1) * (n1 - 1) * (n2 - 1), lay);
}

hipError_t dmc_count_launch(const float* grid, int n0, int n1, int n2, double level, int manifold, char* ws,
                            const SurfWorkspaceLayout& lay, hipStream_t stream) {
    // small only: dmc_classify writes every entry of blk[]
    hipError_t e = hipMemsetAsync(ws + lay.off_small, 0, lay.small_bytes, stream);
    if (e != hipSuccess) return e;
    const Dims d = {n0, n1, n2};
    {
        ProfScope ps(PC_MC_CLASSIFY, 4.0 * (double)n0 * n1 * n2, stream);
        hipLaunchKernelGGL(dmc_classify, dim3(lay.nblk), dim3(kBlock), 0, stream, grid, d, lay.ncells, level, manifold,
                           (uint2*)(ws + lay.off_act), (uint4*)(ws + lay.off_blk), surf_chunk_sums(ws, lay),
                           surf_chunk_nz(ws, lay), surf_status(ws, lay));
    }
    ProfScope ps2(PC_MC_OTHER, 0.0, stream);
    return surf_scan_launch(ws, lay, stream);
}

hipError_t dmc_emit_launch(const float* grid, int n0, int n1, int n2, double level, char* ws,
                           const SurfWorkspaceLayout& lay, float* verts, int32_t* faces, const double* xf9, int reversed,
                           hipStream_t stream) {
    if (lay.nnz == 0) return hipSuccess;
    const Xform xf = xform_from(xf9);
    const Dims d = {n0, n1, n2};
    ProfScope ps(PC_MC_OTHER, 0.0, stream);
    const uint32_t* nz = (const uint32_t*)(ws + lay.off_nz);
    const uint32_t wgs = (lay.nnz + kEmitGroup - 1) / kEmitGroup;
    hipLaunchKernelGGL(dmc_vertices, dim3(wgs), dim3(kEmitWg), 0, stream, grid, d, level, (const uint2*)(ws + lay.off_act),
                       (const uint4*)(ws + lay.off_blk), (const uint2*)(ws + lay.off_blkoff), nz, (uint32_t)lay.nnz,
                       (CellRef*)(ws + lay.off_table), verts, xf, xf9 ? 1 : 0);
    hipLaunchKernelGGL(dmc_quads, dim3(wgs), dim3(kEmitWg), 0, stream, d, (const uint2*)(ws + lay.off_act),
                       (const uint4*)(ws + lay.off_blk), (const uint2*)(ws + lay.off_blkoff), nz, (uint32_t)lay.nnz,
                       (const CellRef*)(ws + lay.off_table), (const float*)verts, faces, reversed);
    return hipGetLastError();
}

}  // namespace r3g
