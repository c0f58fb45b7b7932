// grid_csr_device.h -- the device build of a grid in CSR form (grid_csr.h) as templates over (D, record type): the end of
// the records kernel, the pair count, the per-cell count and fill, and the launch sequences around them.  Included by
// meshdist_kernels.hip, meshinside_kernels.hip and cloud_kernels.hip only; the anonymous namespace gives each its own kernels, so no kernel
// symbol is shared between code objects.  Integer atomics only, and their order decides nothing: the bounding box is a
// min / max, the counts are sums, and the order of the records inside a cell is left open by contract.
#ifndef R3G_GRID_CSR_DEVICE_H
#define R3G_GRID_CSR_DEVICE_H
#include <stddef.h>

#include "grid_csr_kernels.h"
#include "mesh_launch.h"
#include "scan_kernels.h"

namespace r3g {
namespace {

using r3g_grid::GridN;

// how a records kernel ends: the lane's box over its usable records, its skipped count and bad-index flag -> GridCsrSmall
template <int D>
__device__ __forceinline__ void csr_records_reduce(const float* lo, const float* hi, unsigned long long skipped, bool bad,
                                                   GridCsrSmall* __restrict__ sm) {
    unsigned elo[D], ehi[D];
    for (int a = 0; a < D; ++a) {
        elo[a] = r3g_grid::enc_float(lo[a]);
        ehi[a] = r3g_grid::enc_float(hi[a]);
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned l = __shfl_xor(elo[a], d, 64), h = __shfl_xor(ehi[a], d, 64);
            elo[a] = l < elo[a] ? l : elo[a];
            ehi[a] = h > ehi[a] ? h : ehi[a];
        }
    }
    skipped = wave_sum_u64(skipped);
    const unsigned long long anybad = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < D; ++a) {
            atomicMin(&sm->box[a], elo[a]);
            atomicMax(&sm->box[D + a], ehi[a]);
        }
        if (skipped) atomicAdd(&sm->skipped, skipped);
        if (anybad) atomicOr(&sm->bad_index, 1u);
    }
}

template <int D, class R>
__global__ __launch_bounds__(kT) void csr_count_pairs(const R* __restrict__ recs, int64_t nf, GridN<D> g, GridCsrSmall* __restrict__ sm) {
    unsigned long long n = 0;
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const R r = recs[f];
        if (grid_member(r)) n += (unsigned long long)r3g_grid::pairs(g, r);
    }
    n = wave_sum_u64(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&sm->pairs, n);
}

// FILL == false: counts[cell] += 1;  FILL == true: pairs[starts[cell] + cursor[cell]++] = f
template <int D, class R, bool FILL>
__global__ __launch_bounds__(kT) void csr_bin(const R* __restrict__ recs, int64_t nf, GridN<D> g, unsigned* __restrict__ counts,
                                              const unsigned* __restrict__ starts, int32_t* __restrict__ pairs) {
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const R r = recs[f];
        if (!grid_member(r)) continue;
        r3g_grid::for_each_cell(g, r, [&](int cell) {
            const unsigned slot = atomicAdd(&counts[cell], 1u);
            if (FILL) pairs[starts[cell] + slot] = (int32_t)f;
        });
    }
}

// before a records kernel: GridCsrSmall cleared, the lower corner of its box set to the largest code
template <int D>
hipError_t csr_records_begin(char* ws, const GridCsrLayout& lay, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small, 0, sizeof(GridCsrSmall), s));
    return hipMemsetAsync(ws + lay.off_small + offsetof(GridCsrSmall, box), 0xFF, 4 * D, s);
}

// GridCsrSmall::pairs for grid g (touches no cell)
template <int D, class R>
hipError_t csr_count_pairs_launch(char* ws, const GridCsrLayout& lay, int64_t nf, const GridN<D>& g, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(GridCsrSmall, pairs), 0, 8, s));
    hipLaunchKernelGGL((csr_count_pairs<D, R>), dim3(grid_for(nf)), dim3(kT), 0, s, (const R*)(ws + lay.off_recs), nf, g,
                       (GridCsrSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

// per-cell counts -> exclusive scan -> fill of pairs [GridCsrSmall::pairs] with record ids
template <int D, class R>
hipError_t csr_fill_launch(char* ws, const GridCsrLayout& lay, int64_t nf, const GridN<D>& g, int32_t* pairs, hipStream_t s) {
    const int64_t n1 = r3g_grid::cells<D>(g.res) + 1;          // the extra element receives the total
    unsigned* counts = (unsigned*)(ws + lay.off_counts);
    unsigned* starts = (unsigned*)(ws + lay.off_starts);
    const R* recs = (const R*)(ws + lay.off_recs);
    R3G_HIP(hipMemsetAsync(counts, 0, 4 * (size_t)n1, s));
    hipLaunchKernelGGL((csr_bin<D, R, false>), dim3(grid_for(nf)), dim3(kT), 0, s, recs, nf, g, counts, (const unsigned*)nullptr,
                       (int32_t*)nullptr);
    R3G_HIP(exclusive_scan_u32(counts, starts, n1, (unsigned*)(ws + lay.off_sums), nullptr, s));
    R3G_HIP(hipMemsetAsync(counts, 0, 4 * (size_t)n1, s));
    hipLaunchKernelGGL((csr_bin<D, R, true>), dim3(grid_for(nf)), dim3(kT), 0, s, recs, nf, g, counts, (const unsigned*)starts, pairs);
    return hipGetLastError();
}

// ---- records with one home cell each (grid_csr.h, the last section) ------------------------------------------------------------
// FILL == false: counts[home] += 1;  FILL == true: sorted[starts[home] + cursor[home]++] = the record
template <int D, class R, bool FILL>
__global__ __launch_bounds__(kT) void csr_bin_home(const R* __restrict__ recs, int64_t n, GridN<D> g, unsigned* __restrict__ counts,
                                                   const unsigned* __restrict__ starts, R* __restrict__ sorted) {
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < n; f += (int64_t)gridDim.x * kT) {
        const R r = recs[f];
        if (!grid_member(r)) continue;
        const int cell = grid_home(g, r);
        const unsigned slot = atomicAdd(&counts[cell], 1u);
        if (FILL) sorted[starts[cell] + slot] = r;
    }
}

// per-cell counts -> exclusive scan -> the member records into sorted [members] in cell order
template <int D, class R>
hipError_t csr_fill_home_launch(char* ws, const GridCsrLayout& lay, int64_t n, const GridN<D>& g, R* sorted, hipStream_t s) {
    const int64_t n1 = r3g_grid::cells<D>(g.res) + 1;          // the extra element receives the total
    unsigned* counts = (unsigned*)(ws + lay.off_counts);
    unsigned* starts = (unsigned*)(ws + lay.off_starts);
    const R* recs = (const R*)(ws + lay.off_recs);
    R3G_HIP(hipMemsetAsync(counts, 0, 4 * (size_t)n1, s));
    hipLaunchKernelGGL((csr_bin_home<D, R, false>), dim3(grid_for(n)), dim3(kT), 0, s, recs, n, g, counts, (const unsigned*)nullptr,
                       (R*)nullptr);
    R3G_HIP(exclusive_scan_u32(counts, starts, n1, (unsigned*)(ws + lay.off_sums), nullptr, s));
    R3G_HIP(hipMemsetAsync(counts, 0, 4 * (size_t)n1, s));
    hipLaunchKernelGGL((csr_bin_home<D, R, true>), dim3(grid_for(n)), dim3(kT), 0, s, recs, n, g, counts, (const unsigned*)starts, sorted);
    return hipGetLastError();
}

}  // namespace
}  // namespace r3g
#endif
