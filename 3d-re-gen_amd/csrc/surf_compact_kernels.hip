// surf_compact_kernels.hip -- the part of the compaction skeleton of marching cubes and dual marching cubes that does not
// depend on the extractor: the workspace layout and K2, the scan of the block sums.  Integers only, so no
// -ffp-contract flag.  The classify and emit kernels are in mc_kernels.hip / dmc_kernels.hip (helpers: surf_compact_device.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "surf_compact_device.h"
#include "surf_compact_kernels.h"

using namespace r3g_surf;

namespace {

// One workgroup per chunk of 1024 block sums.  base = sum of all earlier chunks (<= a few hundred
// values), then an exclusive scan inside the chunk.  The last block publishes the totals {vertices, faces, non-empty blocks}.
__global__ __launch_bounds__(kChunk) void surf_scan(const uint4* __restrict__ blk, uint32_t nblk,
                                                    const unsigned long long* __restrict__ chunk_sums,
                                                    const unsigned* __restrict__ chunk_nz,
                                                    uint2* __restrict__ blkoff, uint32_t* __restrict__ nzlist,
                                                    unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long s_red[kChunk / 64];
    __shared__ unsigned long long s_wave[kChunk / 64];
    __shared__ unsigned s_red_nz[kChunk / 64];
    __shared__ unsigned s_wave_nz[kChunk / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t ch = blockIdx.x;
    // both halves are < 2^32 in total for any grid the API admits, so packed 2x32 adds cannot carry
    unsigned long long part = 0;
    unsigned part_nz = 0;
    for (uint32_t i = tid; i < ch; i += kChunk) {
        part += chunk_sums[i];
        part_nz += chunk_nz[i];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        part += __shfl_xor(part, d, 64);
        part_nz += __shfl_xor(part_nz, d, 64);
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
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long n = __shfl_up(incl, d, 64);
        const unsigned nn = __shfl_up(incl_nz, d, 64);
        if (lane >= d) { incl += n; incl_nz += nn; }
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

}  // namespace

namespace r3g {

size_t surf_workspace_bytes(int n0, int n1, int n2, uint64_t table_bytes, SurfWorkspaceLayout* lay) {
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
    lay->zero_bytes = o - lay->off_small;
    lay->off_blkoff = o; o += align(8 * nblk);
    lay->off_nz = o;     o += align(4 * nblk);
    lay->off_act = o;    o += align(8 * nblk * kBlock);
    lay->off_table = o;  o += align(table_bytes);
    return (size_t)o;
}

hipError_t surf_scan_launch(char* ws, const SurfWorkspaceLayout& lay, hipStream_t stream) {
    hipLaunchKernelGGL(surf_scan, dim3(lay.nchunk), dim3(kChunk), 0, stream, (const uint4*)(ws + lay.off_blk), lay.nblk,
                       surf_chunk_sums(ws, lay), surf_chunk_nz(ws, lay), (uint2*)(ws + lay.off_blkoff),
                       (uint32_t*)(ws + lay.off_nz), surf_totals(ws, lay));
    return hipGetLastError();
}

}  // namespace r3g
