// scan_device.h -- the one exclusive prefix sum of 32-bit counts that the mesh and volume stacks share (integers only):
// the scan of one value per thread over a workgroup, and the device-wide scan in three launches (a sum per tile of 2048
// elements, one workgroup over the tile sums, the tile's base plus the prefix inside the tile).  An element's value comes
// from a Load functor, so flags, counts and the popcounts of mask words go through the same kernels.  Every sum is taken
// modulo 2^32, so the result is the same bits whatever the launch shape.  Internal to each translation unit that includes
// it (as mesh_launch.h); the plain-array instantiation is exported once by scan_kernels.hip.
#ifndef R3G_SCAN_DEVICE_H
#define R3G_SCAN_DEVICE_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace r3g {
namespace {

constexpr int kScanThreads = 256;                      // of the tile kernels
constexpr int kScanItems = 8;                          // consecutive elements per thread
constexpr int kScanTile = kScanThreads * kScanItems;   // 2048 elements per block
constexpr int kScanSumsThreads = 1024;                 // of the one workgroup that scans the tile sums, kScanItems a thread:
                                                       // 8192 sums a trip, so a grid of 256^3 + 1 cells (8193 tiles) takes two

// words of scratch (the tile sums) that a scan of n elements is given
constexpr size_t scan_scratch_elems(int64_t n) { return (size_t)((n + kScanTile - 1) / kScanTile) + 1; }

// exclusive prefix of v over a workgroup of NW waves; *total = the workgroup's sum.  lds: NW words; ends with a barrier,
// so lds is free again afterwards.  Every thread of the workgroup calls it.
template <int NW>
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* lds, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned n = __shfl_up(incl, d, 64);
        if (lane >= d) incl += n;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    unsigned base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const unsigned t = lds[w];
        if (w < wave) base += t;
        sum += t;
    }
    __syncthreads();
    *total = sum;
    return base + incl - v;
}

// a plain array of counts
struct ScanLoadU32 {
    const unsigned* a;
    __device__ unsigned operator()(int64_t i) const { return a[i]; }
};

// kScanItems consecutive elements from `base` on (0 past n) into v; returns their sum.  A thread that lies wholly inside
// [0, n) tests nothing per element, so that its loads, and its stores below, merge into 16-byte ones.
template <class Load>
__device__ __forceinline__ unsigned scan_load_items(const Load& in, int64_t base, int64_t n, unsigned* v) {
    if (base + kScanItems <= n) {
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) v[i] = in(base + i);
    } else {
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) v[i] = base + i < n ? in(base + i) : 0u;
    }
    unsigned s = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) s += v[i];
    return s;
}

// out[base + i] = run + v[0] + ... + v[i - 1] for the elements below n
__device__ __forceinline__ void scan_store_items(unsigned* out, int64_t base, int64_t n, unsigned run, const unsigned* v) {
    unsigned r[kScanItems];
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        r[i] = run;
        run += v[i];
    }
    if (base + kScanItems <= n) {
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) out[base + i] = r[i];
    } else {
#pragma unroll
        for (int i = 0; i < kScanItems; ++i)
            if (base + i < n) out[base + i] = r[i];
    }
}

template <class Load>
__global__ __launch_bounds__(kScanThreads) void scan_tile_sums(Load in, int64_t n, unsigned* __restrict__ tile_sums) {
    __shared__ unsigned lds[kScanThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    unsigned v[kScanItems], total;
    (void)block_exclusive_scan<kScanThreads / 64>(scan_load_items(in, base, n, v), lds, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// exclusive scan of sums[0, nb) in place by one workgroup of NW waves, every thread of which calls it; returns the total.
// A trip of the loop covers NW * 64 * kScanItems sums.
template <int NW>
__device__ __forceinline__ unsigned scan_sums_in_place(unsigned* sums, unsigned nb, unsigned* lds) {
    unsigned carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += NW * 64 * kScanItems) {      // uniform trip count
        const int64_t base = b0 + (int64_t)threadIdx.x * kScanItems;
        unsigned v[kScanItems], total;
        const unsigned s = scan_load_items(ScanLoadU32{sums}, base, nb, v);
        scan_store_items(sums, base, nb, carry + block_exclusive_scan<NW>(s, lds, &total), v);
        carry += total;
    }
    return carry;
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void scan_sums(unsigned* tile_sums, unsigned nb, unsigned* __restrict__ total_or_null) {
    __shared__ unsigned lds[NW];
    const unsigned total = scan_sums_in_place<NW>(tile_sums, nb, lds);
    if (total_or_null && threadIdx.x == 0) *total_or_null = total;
}

// out may be the array that `in` reads: a thread holds all its elements before it writes, and no other thread reads them
template <class Load>
__global__ __launch_bounds__(kScanThreads) void scan_tile_apply(Load in, int64_t n, const unsigned* __restrict__ tile_sums,
                                                                unsigned* out) {
    __shared__ unsigned lds[kScanThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    unsigned v[kScanItems], total;
    const unsigned s = scan_load_items(in, base, n, v);
    scan_store_items(out, base, n, tile_sums[blockIdx.x] + block_exclusive_scan<kScanThreads / 64>(s, lds, &total), v);
}

// out[i] = in(0) + ... + in(i - 1) for i in [0, n), *d_total_or_null = the sum of all; tile_sums: scan_scratch_elems(n)
// words of scratch.  Three launches; n == 0 only writes the total.
template <class Load>
hipError_t exclusive_scan(Load in, int64_t n, unsigned* out, unsigned* tile_sums, unsigned* d_total_or_null, hipStream_t s) {
    const unsigned nb = (unsigned)((n + kScanTile - 1) / kScanTile);
    if (nb) hipLaunchKernelGGL(scan_tile_sums<Load>, dim3(nb), dim3(kScanThreads), 0, s, in, n, tile_sums);
    if (nb || d_total_or_null)
        hipLaunchKernelGGL(scan_sums<kScanSumsThreads / 64>, dim3(1), dim3(kScanSumsThreads), 0, s, tile_sums, nb, d_total_or_null);
    if (nb) hipLaunchKernelGGL(scan_tile_apply<Load>, dim3(nb), dim3(kScanThreads), 0, s, in, n, (const unsigned*)tile_sums, out);
    return hipGetLastError();
}

}  // namespace
}  // namespace r3g
#endif
