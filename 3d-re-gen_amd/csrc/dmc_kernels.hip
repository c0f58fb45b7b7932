// dmc_kernels.hip -- dual marching cubes on gfx950 (HBM-bound index work, no MFMA).  Definition: DESIGN.md section 4c.
//
// One vertex per surface patch of a cell and one quad per crossed grid edge, read from the (R+1)^3 fp32 grid that stays
// in HBM.  Launch structure (cells linearised axis 2 fastest, 256 cells per block, as in mc_kernels.hip):
//   K1 dmc_classify : one thread per cell: case from the 8 corners, manifold rule from the neighbour across the
//                     tunnelling face (recomputed from the grid, rare), {patch count, quad count} -> per-block
//                     compacted records of the active cells with their in-block prefix, block sums, chunk sums.
//   K2 dmc_scan     : exclusive scan of the block sums (one workgroup per 1024-block chunk) + the list of non-empty blocks.
//   K3 dmc_vertices : one thread per ACTIVE cell: fp64 patch centroids, float32 store, cell table {first vertex, case}.
//   K4 dmc_quads    : one thread per ACTIVE cell: its up to three quads, vertex ids through the cell table of the four
//                     cells around the edge, diagonal chosen on the stored float32 positions.
// Every output position is block offset + in-block prefix, both from scans: nothing depends on the order workgroups run
// in, and the only atomics are integer adds on the chunk totals.  Only K1 touches the whole grid.
//
// Built with -ffp-contract=off: centroid, output transform and diagonal test must not be fused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define R3G_DEV static __device__ __forceinline__
#define R3G_LUT_QUAL static __device__ const
#include "dmc_cell.h"
#include "dmc_kernels.h"
#include "prof.h"

#pragma clang fp contract(off)

using namespace r3g_dmc;

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 1024;  // blocks per scan chunk

__device__ __forceinline__ void cell_coords(uint32_t c, const Dims& d, int& i, int& j, int& k) {
    const uint32_t c2 = (uint32_t)(d.n2 - 1), c1 = (uint32_t)(d.n1 - 1);
    const uint32_t row = c / c2;
    k = (int)(c - row * c2);
    i = (int)(row / c1);
    j = (int)(row - (uint32_t)i * c1);
}

// inclusive scan of a packed 3x16-bit counter across the 64 lanes of a wave
__device__ __forceinline__ unsigned long long wave_inclusive_scan(unsigned long long v, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long n = __shfl_up(v, s, 64);
        if (lane >= s) v += n;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void dmc_classify(const float* __restrict__ grid, Dims d, uint32_t ncells, double level,
                                                       int manifold, uint2* __restrict__ act, uint4* __restrict__ blk,
                                                       unsigned long long* __restrict__ chunk_sums,
                                                       unsigned* __restrict__ chunk_nz, unsigned* __restrict__ status) {
    __shared__ unsigned long long wave_tot[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t b = blockIdx.x;
    const uint32_t c = b * kBlock + tid;
    unsigned flags = 0;
    int i = 0, j = 0, k = 0, cs = 0;
    if (c < ncells) {
        cell_coords(c, d, i, j, k);
        cs = cell_case(grid, d, i, j, k, level, &flags);
    }
    const bool active = cs != 0 && cs != 255;
    // range flags: one global atomic per wave, and only while it would still change the status word
    {
        const unsigned long long le = __ballot(flags & R3G_DMC_FLAG_LE), ge = __ballot(flags & R3G_DMC_FLAG_GE),
                                 nn = __ballot(flags & R3G_DMC_FLAG_NAN);
        const unsigned wf = (le ? R3G_DMC_FLAG_LE : 0u) | (ge ? R3G_DMC_FLAG_GE : 0u) | (nn ? R3G_DMC_FLAG_NAN : 0u);
        if (lane == 0 && (wf & ~*(volatile unsigned*)status)) atomicOr(status, wf);
    }
    // most blocks contain no surface cell: they publish zeros and leave
    if (!__syncthreads_or(active ? 1 : 0)) {
        if (tid == 0) blk[b] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const unsigned rec = active ? classify_cell(grid, d, i, j, k, level, cs, manifold != 0) : 0u;
    // packed counters: [0..15] vertices, [16..31] quads, [32..47] active cells
    const unsigned long long mine = (unsigned long long)rec_patches(rec) | ((unsigned long long)rec_quads(rec) << 16) |
                                    ((unsigned long long)(rec ? 1u : 0u) << 32);
    const unsigned long long incl = wave_inclusive_scan(mine, lane);
    if (lane == 63) wave_tot[wid] = incl;
    __syncthreads();
    unsigned long long base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        const unsigned long long t = wave_tot[w];
        if (w < wid) base += t;
        total += t;
    }
    const unsigned long long excl = base + incl - mine;
    if (rec) {
        const unsigned vloc = (unsigned)(excl & 0xFFFFu), qloc = (unsigned)((excl >> 16) & 0xFFFFu);
        const unsigned arank = (unsigned)((excl >> 32) & 0xFFFFu);
        act[(size_t)b * kBlock + arank] = make_uint2(rec, (unsigned)tid | (vloc << 8) | (qloc << 20));
    }
    if (tid == 0) {
        const unsigned sv = (unsigned)(total & 0xFFFFu), sq = (unsigned)((total >> 16) & 0xFFFFu);
        const unsigned sa = (unsigned)((total >> 32) & 0xFFFFu);
        blk[b] = make_uint4(sv, sq, sa, 0u);
        if (sv | sq) atomicAdd(&chunk_sums[b / kChunk], (unsigned long long)sv | ((unsigned long long)sq << 32));
        if (sa) atomicAdd(&chunk_nz[b / kChunk], 1u);
    }
}

// One workgroup per chunk of 1024 block sums.  base = sum of all earlier chunks, then an exclusive scan inside the
// chunk.  The last block publishes the totals {vertices, quads, non-empty blocks}.
__global__ __launch_bounds__(kChunk) void dmc_scan(const uint4* __restrict__ blk, uint32_t nblk,
                                                   const unsigned long long* __restrict__ chunk_sums,
                                                   const unsigned* __restrict__ chunk_nz, uint2* __restrict__ blkoff,
                                                   uint32_t* __restrict__ nzlist, unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long s_red[kChunk / 64];
    __shared__ unsigned long long s_wave[kChunk / 64];
    __shared__ unsigned s_red_nz[kChunk / 64];
    __shared__ unsigned s_wave_nz[kChunk / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t ch = blockIdx.x;
    // both halves stay below 2^32 for any grid the API admits, so packed 2x32 adds cannot carry
    unsigned long long part = 0;
    unsigned part_nz = 0;
    for (uint32_t n = tid; n < ch; n += kChunk) {
        part += chunk_sums[n];
        part_nz += chunk_nz[n];
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        part += __shfl_xor(part, s, 64);
        part_nz += __shfl_xor(part_nz, s, 64);
    }
    if (lane == 0) { s_red[wid] = part; s_red_nz[wid] = part_nz; }
    const uint32_t bi = ch * kChunk + tid;
    unsigned long long mine = 0;
    unsigned mine_nz = 0;
    if (bi < nblk) {
        const uint4 s = blk[bi];
        mine = (unsigned long long)s.x | ((unsigned long long)s.y << 32);
        mine_nz = s.z ? 1u : 0u;
    }
    unsigned long long incl = mine;
    unsigned incl_nz = mine_nz;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long n = __shfl_up(incl, s, 64);
        const unsigned nn = __shfl_up(incl_nz, s, 64);
        if (lane >= s) { incl += n; incl_nz += nn; }
    }
    if (lane == 63) { s_wave[wid] = incl; s_wave_nz[wid] = incl_nz; }
    __syncthreads();
    unsigned long long base = 0;
    unsigned base_nz = 0;
#pragma unroll
    for (int w = 0; w < kChunk / 64; ++w) {
        base += s_red[w];
        base_nz += s_red_nz[w];
        if (w < wid) { base += s_wave[w]; base_nz += s_wave_nz[w]; }
    }
    const unsigned long long excl = base + incl - mine;
    const unsigned excl_nz = base_nz + incl_nz - mine_nz;
    if (bi < nblk) blkoff[bi] = make_uint2((unsigned)(excl & 0xFFFFFFFFull), (unsigned)(excl >> 32));
    if (mine_nz) nzlist[excl_nz] = bi;
    if (bi == nblk - 1) {
        const unsigned long long tot = excl + mine;
        totals[0] = tot & 0xFFFFFFFFull;
        totals[1] = tot >> 32;
        totals[2] = excl_nz + mine_nz;
    }
}

// K3 / K4 geometry, as mc_vertices / mc_faces: a workgroup of 256 threads takes 8 consecutive non-empty blocks and
// spreads their active cells over its threads (a smooth surface leaves ~11 active cells in a block).
constexpr int kEmitGroup = 8;
constexpr int kEmitWg = 256;

struct EmitMap {
    unsigned pre[kEmitGroup + 1];
    uint32_t blk_id[kEmitGroup];
};
__device__ __forceinline__ void emit_map_build(EmitMap* m, const uint4* __restrict__ blk, const uint32_t* __restrict__ nzlist,
                                               uint32_t nnz) {
    if (threadIdx.x == 0) {
        unsigned run = 0;
#pragma unroll
        for (int n = 0; n < kEmitGroup; ++n) {
            const uint32_t g = blockIdx.x * kEmitGroup + n;
            m->pre[n] = run;
            if (g < nnz) {
                const uint32_t b = nzlist[g];
                m->blk_id[n] = b;
                run += blk[b].z;
            } else {
                m->blk_id[n] = 0;
            }
        }
        m->pre[kEmitGroup] = run;
    }
    __syncthreads();
}
__device__ __forceinline__ bool emit_map_find(const EmitMap* m, unsigned item, uint32_t* b, unsigned* local) {
    if (item >= m->pre[kEmitGroup]) return false;
    int n = 0;
#pragma unroll
    for (int q = 1; q < kEmitGroup; ++q) n += (item >= m->pre[q]) ? 1 : 0;
    *b = m->blk_id[n];
    *local = item - m->pre[n];
    return true;
}

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

size_t dmc_workspace_bytes(int n0, int n1, int n2, DmcWorkspaceLayout* lay) {
    const uint64_t ncells = (uint64_t)(n0 - 1) * (n1 - 1) * (n2 - 1);
    const uint64_t nblk = (ncells + kBlock - 1) / kBlock;
    const uint64_t nchunk = (nblk + kChunk - 1) / kChunk;
    auto align = [](uint64_t v) { return (v + 255) & ~(uint64_t)255; };
    uint64_t o = 0;
    lay->nblk = (uint32_t)nblk;
    lay->nchunk = (uint32_t)nchunk;
    lay->ncells = (uint32_t)ncells;
    lay->nnz = 0;
    // [status u32 | pad | totals 3xu64 @16 | chunk_sums u64 x nchunk @64 | chunk_nz u32 x nchunk]: zeroed per call
    lay->off_small = o;
    lay->small_bytes = align(64 + 12 * nchunk);
    o += lay->small_bytes;
    lay->off_blk = o;    o += align(16 * nblk);
    lay->off_blkoff = o; o += align(8 * nblk);
    lay->off_nz = o;     o += align(4 * nblk);
    lay->off_act = o;    o += align(8 * nblk * kBlock);
    lay->off_ctab = o;   o += align(sizeof(CellRef) * ncells);   // written and read for active cells only: never initialised
    return (size_t)o;
}

hipError_t dmc_count_launch(const float* grid, int n0, int n1, int n2, double level, int manifold, char* ws,
                            const DmcWorkspaceLayout& lay, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(ws + lay.off_small, 0, lay.small_bytes, stream);
    if (e != hipSuccess) return e;
    unsigned* status = (unsigned*)(ws + lay.off_small);
    unsigned long long* totals = (unsigned long long*)(ws + lay.off_small + 16);
    unsigned long long* chunk_sums = (unsigned long long*)(ws + lay.off_small + 64);
    unsigned* chunk_nz = (unsigned*)(ws + lay.off_small + 64 + 8 * (size_t)lay.nchunk);
    const Dims d = {n0, n1, n2};
    {
        ProfScope ps(PC_MC_CLASSIFY, 4.0 * (double)n0 * n1 * n2, stream);
        hipLaunchKernelGGL(dmc_classify, dim3(lay.nblk), dim3(kBlock), 0, stream, grid, d, lay.ncells, level, manifold,
                           (uint2*)(ws + lay.off_act), (uint4*)(ws + lay.off_blk), chunk_sums, chunk_nz, status);
    }
    ProfScope ps2(PC_MC_OTHER, 0.0, stream);
    hipLaunchKernelGGL(dmc_scan, dim3(lay.nchunk), dim3(kChunk), 0, stream, (const uint4*)(ws + lay.off_blk), lay.nblk,
                       chunk_sums, chunk_nz, (uint2*)(ws + lay.off_blkoff), (uint32_t*)(ws + lay.off_nz), totals);
    return hipGetLastError();
}

hipError_t dmc_emit_launch(const float* grid, int n0, int n1, int n2, double level, char* ws,
                           const DmcWorkspaceLayout& lay, float* verts, int32_t* faces, const double* xf9, int reversed,
                           hipStream_t stream) {
    if (lay.nnz == 0) return hipSuccess;
    Xform xf;
    for (int a = 0; a < 3; ++a) {
        xf.grid_size[a] = xf9 ? xf9[a] : 1.0;
        xf.bbox_size[a] = xf9 ? xf9[3 + a] : 1.0;
        xf.bbox_min[a] = xf9 ? xf9[6 + a] : 0.0;
    }
    const Dims d = {n0, n1, n2};
    ProfScope ps(PC_MC_OTHER, 0.0, stream);
    const uint32_t* nz = (const uint32_t*)(ws + lay.off_nz);
    const uint32_t wgs = (lay.nnz + kEmitGroup - 1) / kEmitGroup;
    hipLaunchKernelGGL(dmc_vertices, dim3(wgs), dim3(kEmitWg), 0, stream, grid, d, level, (const uint2*)(ws + lay.off_act),
                       (const uint4*)(ws + lay.off_blk), (const uint2*)(ws + lay.off_blkoff), nz, (uint32_t)lay.nnz,
                       (CellRef*)(ws + lay.off_ctab), verts, xf, xf9 ? 1 : 0);
    hipLaunchKernelGGL(dmc_quads, dim3(wgs), dim3(kEmitWg), 0, stream, d, (const uint2*)(ws + lay.off_act),
                       (const uint4*)(ws + lay.off_blk), (const uint2*)(ws + lay.off_blkoff), nz, (uint32_t)lay.nnz,
                       (const CellRef*)(ws + lay.off_ctab), (const float*)verts, faces, reversed);
    return hipGetLastError();
}

}  // namespace r3g
