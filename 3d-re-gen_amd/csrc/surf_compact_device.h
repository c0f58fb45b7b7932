// surf_compact_device.h -- device half of the compaction skeleton that marching cubes (mc_kernels.hip) and dual marching
// cubes (dmc_kernels.hip) share.  Cells are linearised in scan order, 256 per block.  A classify kernel leaves, per block,
// the compacted records of its active cells with their in-block prefix, the block's sums, and the sums per scan chunk;
// surf_scan (surf_compact_kernels.hip) turns those into block offsets and the list of non-empty blocks; the emit kernels
// walk that list through an EmitMap.  Every output position is block offset + in-block prefix: nothing depends on the
// order workgroups run in.  Integers only.
#ifndef R3G_SURF_COMPACT_DEVICE_H
#define R3G_SURF_COMPACT_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surf_common.h"

namespace r3g_surf {

constexpr int kBlock = 256;   // cells per block
constexpr int kChunk = 1024;  // blocks per scan chunk

// inclusive scan of a packed 3x16-bit counter across the 64 lanes of a wave
static __device__ __forceinline__ unsigned long long wave_inclusive_scan(unsigned long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long n = __shfl_up(v, d, 64);
        if (lane >= d) v += n;
    }
    return v;
}

// range flags (R3G_SURF_FLAG_*): one global atomic per wave, and only while it would still change the status word
static __device__ __forceinline__ void publish_range_flags(unsigned flags, unsigned* status) {
    const unsigned long long le = __ballot(flags & R3G_SURF_FLAG_LE), ge = __ballot(flags & R3G_SURF_FLAG_GE),
                             nn = __ballot(flags & R3G_SURF_FLAG_NAN);
    const unsigned wf = (le ? R3G_SURF_FLAG_LE : 0u) | (ge ? R3G_SURF_FLAG_GE : 0u) | (nn ? R3G_SURF_FLAG_NAN : 0u);
    if ((threadIdx.x & 63) == 0 && (wf & ~*(volatile unsigned*)status)) atomicOr(status, wf);
}

// Tail of a classify kernel with one thread per cell; all kBlock threads of block b call it.  rec is the thread's record
// (0: inactive cell), nv / nf what its cell adds to the two outputs (vertices; triangles or quads).  Leaves the records
// of the active cells in act[b * kBlock ...] as {rec, thread | vertex prefix << 8 | face prefix << 20}, the block's sums
// {vertices, faces, active cells} in blk[b], and adds them to the chunk's totals.
static __device__ __forceinline__ void publish_block(unsigned rec, unsigned nv, unsigned nf, uint32_t b,
                                                     uint2* __restrict__ act, uint4* __restrict__ blk,
                                                     unsigned long long* __restrict__ chunk_sums,
                                                     unsigned* __restrict__ chunk_nz) {
    __shared__ unsigned long long wave_tot[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // packed counters: [0..15] vertices, [16..31] faces, [32..47] active cells
    const unsigned long long mine = (unsigned long long)nv | ((unsigned long long)nf << 16) |
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
        const unsigned vloc = (unsigned)(excl & 0xFFFFu), floc = (unsigned)((excl >> 16) & 0xFFFFu);
        const unsigned arank = (unsigned)((excl >> 32) & 0xFFFFu);
        act[(size_t)b * kBlock + arank] = make_uint2(rec, (unsigned)tid | (vloc << 8) | (floc << 20));
    }
    if (tid == 0) {
        const unsigned sv = (unsigned)(total & 0xFFFFu), sf = (unsigned)((total >> 16) & 0xFFFFu);
        const unsigned sa = (unsigned)((total >> 32) & 0xFFFFu);
        blk[b] = make_uint4(sv, sf, sa, 0u);
        if (sv | sf) atomicAdd(&chunk_sums[b / kChunk], (unsigned long long)sv | ((unsigned long long)sf << 32));
        if (sa) atomicAdd(&chunk_nz[b / kChunk], 1u);
    }
}

// Emit geometry: a workgroup of 256 threads takes kEmitGroup (8) CONSECUTIVE non-empty blocks and spreads their active
// cells over its threads (a prefix over the blocks' active counts in LDS, a short linear search).  A block of a smooth
// surface holds ~11 active cells: with a 64-thread workgroup per non-empty block five lanes in six idled, and an
// object-sized mesh took 19 855 workgroups per kernel (profiles/r05_mc_timeline.md); 24 blocks per workgroup measured
// slower (too few workgroups).
constexpr int kEmitGroup = 8;
constexpr int kEmitWg = 256;

struct EmitMap {
    unsigned pre[kEmitGroup + 1];
    uint32_t blk_id[kEmitGroup];
};
static __device__ __forceinline__ void emit_map_build(EmitMap* m, const uint4* __restrict__ blk,
                                                      const uint32_t* __restrict__ nzlist, uint32_t nnz) {
    if (threadIdx.x == 0) {
        unsigned run = 0;
#pragma unroll
        for (int j = 0; j < kEmitGroup; ++j) {
            const uint32_t g = blockIdx.x * kEmitGroup + j;
            m->pre[j] = run;
            if (g < nnz) {
                const uint32_t b = nzlist[g];
                m->blk_id[j] = b;
                run += blk[b].z;
            } else {
                m->blk_id[j] = 0;
            }
        }
        m->pre[kEmitGroup] = run;
    }
    __syncthreads();
}
// the calling thread's (block, index of an active cell in it) for item `i` of the workgroup's cells, or false when i is past them
static __device__ __forceinline__ bool emit_map_find(const EmitMap* m, unsigned i, uint32_t* b, unsigned* local) {
    if (i >= m->pre[kEmitGroup]) return false;
    int j = 0;
#pragma unroll
    for (int k = 1; k < kEmitGroup; ++k) j += (i >= m->pre[k]) ? 1 : 0;
    *b = m->blk_id[j];
    *local = i - m->pre[j];
    return true;
}

}  // namespace r3g_surf
#endif
