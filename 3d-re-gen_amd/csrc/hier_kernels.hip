// hier_kernels.hip -- planner passes of the hierarchical volume decoder (gfx950, wave64).  See hier_kernels.h and DESIGN.md.
//
// All of them are streaming passes over at most (R+1)^3 points.  The mask of the fine lattice is one bit per point in the order of
// the linear index (a wave's 64 lanes are 64 consecutive points, their ballot is the word), so that an active point's rank in the
// ascending list is the popcount prefix of its word plus the popcount below its bit: the list and the merge need no sort, no
// scatter and no atomics.  Every count is an integer; nothing depends on the order in which workgroups run.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hier_kernels.h"
#include "prof.h"
#include "scan_device.h"

namespace r3g {

namespace {

constexpr int kMaxBlocks = 2048;   // grids are capped (256 CUs x 8 workgroups) and grid-strided

inline int capped_blocks(int64_t items, int per_block) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, kMaxBlocks));
}

__device__ __forceinline__ bool above(float g, double level) { return (double)g > level; }   // the marching-cubes inside test; NaN: false

// steps 1-3: cand(p) = some 6-neighbour on the other side of the level, or |G(p) - level| < band
__global__ __launch_bounds__(256) void hier_cand_kernel(const float* __restrict__ G, int nc, double level, double band,
                                                        uint8_t* __restrict__ cand) {
    const int64_t total = (int64_t)nc * nc * nc;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t sj = nc, si = (int64_t)nc * nc;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const int k = (int)(p % nc), j = (int)((p / nc) % nc), i = (int)(p / si);
        const float g = G[p];
        const bool s = above(g, level);
        bool c = fabs((double)g - level) < band;
        if (i > 0) c |= above(G[p - si], level) != s;
        if (i + 1 < nc) c |= above(G[p + si], level) != s;
        if (j > 0) c |= above(G[p - sj], level) != s;
        if (j + 1 < nc) c |= above(G[p + sj], level) != s;
        if (k > 0) c |= above(G[p - 1], level) != s;
        if (k + 1 < nc) c |= above(G[p + 1], level) != s;
        cand[p] = c ? 1 : 0;
    }
}

// step 4: one dilation by the 3x3x3 box, clipped to the grid
__global__ __launch_bounds__(256) void hier_dilate_kernel(const uint8_t* __restrict__ in, int nc, uint8_t* __restrict__ out) {
    const int64_t total = (int64_t)nc * nc * nc;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
        const int k = (int)(p % nc), j = (int)((p / nc) % nc), i = (int)(p / ((int64_t)nc * nc));
        const int i0 = max(i - 1, 0), i1 = min(i + 1, nc - 1), j0 = max(j - 1, 0), j1 = min(j + 1, nc - 1);
        const int k0 = max(k - 1, 0), k1 = min(k + 1, nc - 1);
        unsigned any = 0;
        for (int a = i0; a <= i1; ++a)
            for (int b = j0; b <= j1; ++b)
                for (int c = k0; c <= k1; ++c) any |= in[((int64_t)a * nc + b) * nc + c];
        out[p] = any ? 1 : 0;
    }
}

// step 5: F(q) = some coarse p with C(p) and |2p - q| <= r on every axis (the seed 2p dilated r times); a wave owns word w
__global__ __launch_bounds__(256) void hier_mask_kernel(const uint8_t* __restrict__ C, int nc, int nf, int r, int64_t fine_pts,
                                                        int64_t nwords, unsigned long long* __restrict__ words) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t w = wave; w < nwords; w += nwaves) {      // wave-uniform trip count
        const int64_t q = w * 64 + lane;
        bool act = false;
        if (q < fine_pts) {
            const int k = (int)(q % nf), j = (int)((q / nf) % nf), i = (int)(q / ((int64_t)nf * nf));
            // p in [ceil((x - r) / 2), floor((x + r) / 2)], clipped
            const int i0 = max((i - r + 1) >> 1, 0), i1 = min((i + r) >> 1, nc - 1);
            const int j0 = max((j - r + 1) >> 1, 0), j1 = min((j + r) >> 1, nc - 1);
            const int k0 = max((k - r + 1) >> 1, 0), k1 = min((k + r) >> 1, nc - 1);
            unsigned any = 0;
            for (int a = i0; a <= i1; ++a)
                for (int b = j0; b <= j1; ++b)
                    for (int c = k0; c <= k1; ++c) any |= C[((int64_t)a * nc + b) * nc + c];
            act = any != 0;
        }
        const unsigned long long word = __ballot(act);
        if (lane == 0) words[w] = word;
    }
}

// an element of the scan (scan_device.h) is the popcount of a mask word
struct PopcLoad {
    const unsigned long long* words;
    __device__ unsigned operator()(int64_t w) const { return (unsigned)__popcll(words[w]); }
};

// scan_sums with another ending: the grand total goes to small[0] as 64 bits, and the same launch resets small[1]
__global__ __launch_bounds__(kScanSumsThreads) void hier_scan_bsum_kernel(unsigned* __restrict__ bsum, unsigned nblocks,
                                                                          unsigned long long* __restrict__ small) {
    __shared__ unsigned lds[kScanSumsThreads / 64];
    const unsigned total = scan_sums_in_place<kScanSumsThreads / 64>(bsum, nblocks, lds);
    if (threadIdx.x == 0) {
        small[0] = total;
        small[1] = 0;                                      // the unsafe-cell counter of this select
    }
}

// step 6: a point's rank = prefix of its word + set bits below its own; ranks rise with q, so the stores are coalesced
__global__ __launch_bounds__(256) void hier_indices_kernel(const unsigned long long* __restrict__ words,
                                                           const unsigned* __restrict__ prefix, int64_t fine_pts,
                                                           int32_t* __restrict__ idx) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < fine_pts; q += stride) {
        const unsigned long long word = words[q >> 6];
        const int b = (int)(q & 63);
        if ((word >> b) & 1ull) idx[prefix[q >> 6] + (unsigned)__popcll(word & ((1ull << b) - 1ull))] = (int32_t)q;
    }
}

// step 8: four consecutive points per lane (one 16-byte store; 4 | 64, so they share a word)
__global__ __launch_bounds__(256) void hier_merge_kernel(const unsigned long long* __restrict__ words,
                                                         const unsigned* __restrict__ prefix, const float* __restrict__ coarse,
                                                         const float* __restrict__ values, int nc, int nf, int64_t fine_pts,
                                                         float* __restrict__ fine) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; q0 < fine_pts; q0 += stride) {
        const unsigned long long word = words[q0 >> 6];
        const unsigned base = prefix[q0 >> 6];
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t q = q0 + e;
            v[e] = 0.f;
            if (q < fine_pts) {
                const int b = (int)(q & 63);
                if ((word >> b) & 1ull) {
                    v[e] = values[base + (unsigned)__popcll(word & ((1ull << b) - 1ull))];
                } else {
                    const int k = (int)(q % nf), j = (int)((q / nf) % nf), i = (int)(q / ((int64_t)nf * nf));
                    v[e] = coarse[((int64_t)(i >> 1) * nc + (j >> 1)) * nc + (k >> 1)];
                }
            }
        }
        if (q0 + 3 < fine_pts) {
            *reinterpret_cast<float4*>(fine + q0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (q0 + e < fine_pts) fine[q0 + e] = v[e];
        }
    }
}

// mixed cells of the final grid with a corner outside the mask (their triangles would rest on a filled value)
__global__ __launch_bounds__(256) void hier_unsafe_kernel(const unsigned long long* __restrict__ words, const float* __restrict__ fine,
                                                          int nf, double level, unsigned long long* __restrict__ counter) {
    const int m = nf - 1;
    const int64_t cells = (int64_t)m * m * m;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t rounds = (cells + stride - 1) / stride;       // uniform trip count: the ballot below needs whole waves
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned mine = 0;
    for (int64_t it = 0; it < rounds; ++it, c += stride) {
        if (c >= cells) continue;
        const int k = (int)(c % m), j = (int)((c / m) % m), i = (int)(c / ((int64_t)m * m));
        int n_above = 0;
        bool all_active = true;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int64_t q = ((int64_t)(i + (d >> 2)) * nf + (j + ((d >> 1) & 1))) * nf + (k + (d & 1));
            n_above += above(fine[q], level) ? 1 : 0;
            all_active = all_active && ((words[q >> 6] >> (q & 63)) & 1ull);
        }
        if (n_above > 0 && n_above < 8 && !all_active) ++mine;
    }
    // integer sum: wave reduction, one atomic per wave
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(counter, (unsigned long long)mine);
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t hier_workspace_bytes(int nc, HierLayout* lay) {
    HierLayout l;
    l.nc = nc;
    l.nf = 2 * nc - 1;
    l.coarse_pts = (int64_t)nc * nc * nc;
    l.fine_pts = (int64_t)l.nf * l.nf * l.nf;
    l.nwords = (l.fine_pts + 63) / 64;
    l.nblocks = (int)((l.nwords + kScanTile - 1) / kScanTile);
    size_t off = 0;
    l.off_small = off; off += 256;
    l.off_cand = off; off += align256((size_t)l.coarse_pts);
    l.off_dil = off; off += align256((size_t)l.coarse_pts);
    l.off_words = off; off += align256((size_t)l.nwords * 8);
    l.off_prefix = off; off += align256((size_t)l.nwords * 4);
    l.off_bsum = off; off += align256(scan_scratch_elems(l.nwords) * 4);
    l.total = off;
    if (lay) *lay = l;
    return off;
}

hipError_t hier_select_launch(const float* coarse, double level, double band, int is_finest, char* ws, const HierLayout& lay,
                              hipStream_t s) {
    uint8_t* cand = reinterpret_cast<uint8_t*>(ws + lay.off_cand);
    uint8_t* dil = reinterpret_cast<uint8_t*>(ws + lay.off_dil);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(ws + lay.off_words);
    unsigned* prefix = reinterpret_cast<unsigned*>(ws + lay.off_prefix);
    unsigned* bsum = reinterpret_cast<unsigned*>(ws + lay.off_bsum);
    unsigned long long* small = reinterpret_cast<unsigned long long*>(ws + lay.off_small);
    const int e = is_finest ? 0 : 1;
    // bytes: the coarse grid once (its neighbours come from cache), the byte masks, the words three times, the prefix once
    ProfScope prof_scope_(PC_ELEMWISE, (double)lay.coarse_pts * (4 + 1 + 3 * e) + (double)lay.nwords * (3 * 8 + 4), s);
    hipLaunchKernelGGL(hier_cand_kernel, dim3(capped_blocks(lay.coarse_pts, 256)), dim3(256), 0, s, coarse, lay.nc, level, band, cand);
    if (e) hipLaunchKernelGGL(hier_dilate_kernel, dim3(capped_blocks(lay.coarse_pts, 256)), dim3(256), 0, s, cand, lay.nc, dil);
    hipLaunchKernelGGL(hier_mask_kernel, dim3(capped_blocks(lay.nwords, 4)), dim3(256), 0, s, e ? dil : cand, lay.nc, lay.nf, 2 - e,
                       lay.fine_pts, lay.nwords, words);
    // the scan of scan_device.h over the words' popcounts, with hier_scan_bsum_kernel in the place of scan_sums
    hipLaunchKernelGGL(scan_tile_sums<PopcLoad>, dim3(lay.nblocks), dim3(kScanThreads), 0, s, PopcLoad{words}, lay.nwords, bsum);
    hipLaunchKernelGGL(hier_scan_bsum_kernel, dim3(1), dim3(kScanSumsThreads), 0, s, bsum, (unsigned)lay.nblocks, small);
    hipLaunchKernelGGL(scan_tile_apply<PopcLoad>, dim3(lay.nblocks), dim3(kScanThreads), 0, s, PopcLoad{words}, lay.nwords,
                       (const unsigned*)bsum, prefix);
    return hipGetLastError();
}

hipError_t hier_indices_launch(const char* ws, const HierLayout& lay, int32_t* idx, hipStream_t s) {
    ProfScope prof_scope_(PC_ELEMWISE, (double)lay.nwords * 12, s);      // + 4 bytes per active point
    hipLaunchKernelGGL(hier_indices_kernel, dim3(capped_blocks(lay.fine_pts, 256)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(ws + lay.off_words),
                       reinterpret_cast<const unsigned*>(ws + lay.off_prefix), lay.fine_pts, idx);
    return hipGetLastError();
}

hipError_t hier_merge_launch(const char* ws, const HierLayout& lay, const float* coarse, const float* values, float* fine,
                             hipStream_t s) {
    ProfScope prof_scope_(PC_ELEMWISE, (double)lay.fine_pts * 4 + (double)lay.coarse_pts * 4 + (double)lay.nwords * 12, s);
    hipLaunchKernelGGL(hier_merge_kernel, dim3(capped_blocks((lay.fine_pts + 3) / 4, 256)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(ws + lay.off_words),
                       reinterpret_cast<const unsigned*>(ws + lay.off_prefix), coarse, values, lay.nc, lay.nf, lay.fine_pts, fine);
    return hipGetLastError();
}

hipError_t hier_unsafe_launch(char* ws, const HierLayout& lay, const float* fine, double level, hipStream_t s) {
    unsigned long long* small = reinterpret_cast<unsigned long long*>(ws + lay.off_small);
    hipError_t e = hipMemsetAsync(small + 1, 0, 8, s);
    if (e != hipSuccess) return e;
    ProfScope prof_scope_(PC_ELEMWISE, (double)lay.fine_pts * 4 + (double)lay.nwords * 8, s);
    const int64_t cells = (int64_t)(lay.nf - 1) * (lay.nf - 1) * (lay.nf - 1);
    hipLaunchKernelGGL(hier_unsafe_kernel, dim3(capped_blocks(cells, 256)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(ws + lay.off_words), fine, lay.nf, level, small + 1);
    return hipGetLastError();
}

}  // namespace r3g
