// grid_csr_kernels.hip -- the part of the grid build (grid_csr.h) that does not depend on the record type: the workspace
// layout and the exclusive scan that turns per-cell counts into CSR row starts.  Integers only.
#include "grid_csr_kernels.h"
#include "mesh_launch.h"

namespace r3g {
namespace {

constexpr int kScanItems = kCsrScanTile / kT;  // per thread
constexpr int kSumItemsSmall = 4;              // one block scans the tile sums: 1024 of them (2^20 columns + 1 make 513) ...
constexpr int kSumItemsLarge = 40;             // ... or 10240 (2^24 cells + 1 make 8193)

// exclusive scan of one tile of ITEMS * kT elements per block (in place allowed); the tile's total goes to sums[block]
template <int ITEMS>
__global__ __launch_bounds__(kT) void csr_scan_tile(const unsigned* in, unsigned* out, int64_t n, unsigned* sums) {
    __shared__ unsigned sh[kT];
    const int64_t base = ((int64_t)blockIdx.x * kT + threadIdx.x) * ITEMS;
    unsigned v[ITEMS], total = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        v[i] = base + i < n ? in[base + i] : 0u;
        total += v[i];
    }
    sh[threadIdx.x] = total;
    __syncthreads();
    for (int d = 1; d < kT; d <<= 1) {
        const unsigned add = threadIdx.x >= (unsigned)d ? sh[threadIdx.x - d] : 0u;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned run = sh[threadIdx.x] - total;      // exclusive prefix of this thread inside the tile
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    if (sums && threadIdx.x == kT - 1) sums[blockIdx.x] = sh[kT - 1];
}

__global__ __launch_bounds__(kT) void csr_scan_add(unsigned* out, int64_t n, const unsigned* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * kCsrScanTile + threadIdx.x;
    const unsigned add = sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const int64_t j = i + (int64_t)k * kT;
        if (j < n) out[j] += add;
    }
}

}  // namespace

static_assert(kScanItems * kT == kCsrScanTile && kCsrScanMax == (int64_t)kT * kSumItemsLarge * kCsrScanTile, "the scan's shape");

size_t grid_csr_workspace_bytes(int64_t nf, size_t record_bytes, int64_t cells, GridCsrLayout* lay) {
    const size_t cells1 = (size_t)cells + 1;
    const size_t tiles = (cells1 + kCsrScanTile - 1) / kCsrScanTile;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 0;
    lay->off_small = o, o += 256;
    lay->off_recs = o, o += up(record_bytes * (size_t)nf);
    lay->off_counts = o, o += up(4 * cells1);
    lay->off_starts = o, o += up(4 * cells1);
    lay->off_sums = o, o += up(4 * tiles);
    lay->total = o;
    return o;
}

hipError_t csr_exclusive_scan(const unsigned* counts, unsigned* starts, int64_t n1, unsigned* sums, hipStream_t s) {
    if (n1 > kCsrScanMax) return hipErrorInvalidValue;
    const unsigned tiles = nblocks(n1, kCsrScanTile);
    hipLaunchKernelGGL(csr_scan_tile<kScanItems>, dim3(tiles), dim3(kT), 0, s, counts, starts, n1, sums);
    if (tiles <= (unsigned)(kT * kSumItemsSmall))
        hipLaunchKernelGGL(csr_scan_tile<kSumItemsSmall>, dim3(1), dim3(kT), 0, s, (const unsigned*)sums, sums, (int64_t)tiles,
                           (unsigned*)nullptr);
    else
        hipLaunchKernelGGL(csr_scan_tile<kSumItemsLarge>, dim3(1), dim3(kT), 0, s, (const unsigned*)sums, sums, (int64_t)tiles,
                           (unsigned*)nullptr);
    hipLaunchKernelGGL(csr_scan_add, dim3(tiles), dim3(kT), 0, s, starts, n1, (const unsigned*)sums);
    return hipGetLastError();
}

}  // namespace r3g
