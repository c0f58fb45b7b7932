// meshinside_kernels.hip -- ray-crossing count against a grid of columns in CSR form.
//
// Build: records (index check, projected padded copies, usability, projected bounding box) -> pair count per candidate
// resolution (host halves it while the total is too high) -> per-column count -> exclusive scan -> fill.  Query: one lane per
// point sums the crossings of the faces listed in its column (meshinside_core.h).  Integer atomics only; their order decides
// nothing: the bounding box is a min / max, the counts are sums, and the order of the faces inside a column only permutes
// the terms of an integer sum.
#include <hip/hip_runtime.h>

#include <atomic>

#pragma clang fp contract(off)

#define R3G_MI_HD static __host__ __device__ __forceinline__
#include "meshinside_kernels.h"

namespace r3g {
namespace {

using r3g_mi::Grid2;
using r3g_mi::Rec;

constexpr int kT = 256;
constexpr int kScanItems = 8;                  // per thread: a scan tile is 2048 elements
constexpr int kScanTile = kT * kScanItems;
constexpr int kSumItems = 4;                   // one block scans the tile sums: 2^20 columns + 1 make 513 tiles, 1024 fit

inline unsigned nblocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
inline unsigned grid_for(int64_t n) {
    const unsigned b = nblocks(n, kT);
    return b < 1 ? 1 : (b > 4096 ? 4096 : b);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(kT) void mi_records(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ faces,
                                                 int64_t nf, int axis, Rec* __restrict__ recs, MeshinsideSmall* __restrict__ sm) {
    float lo[2] = {r3g_mi::kInf, r3g_mi::kInf}, hi[2] = {-r3g_mi::kInf, -r3g_mi::kInf};
    unsigned long long skipped = 0;
    bool bad = false;
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        Rec r;
        r.au = r.av = r.aw = r.bu = r.bv = r.bw = r.cu = r.cv = r.cw = 0.0f;
        r.ia = -1, r.ib = r.ic = 0;
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) {
            bad = true;                                   // nothing is read through a bad index
        } else {
            const float a[3] = {verts[3 * (int64_t)i0], verts[3 * (int64_t)i0 + 1], verts[3 * (int64_t)i0 + 2]};
            const float b[3] = {verts[3 * (int64_t)i1], verts[3 * (int64_t)i1 + 1], verts[3 * (int64_t)i1 + 2]};
            const float c[3] = {verts[3 * (int64_t)i2], verts[3 * (int64_t)i2 + 1], verts[3 * (int64_t)i2 + 2]};
            r = r3g_mi::make_rec(a, i0, b, i1, c, i2, axis);
            if (r3g_mi::rec_finite(r)) {
                lo[0] = r3g_mi::fmin2(lo[0], r3g_mi::fmin2(r.au, r3g_mi::fmin2(r.bu, r.cu)));
                lo[1] = r3g_mi::fmin2(lo[1], r3g_mi::fmin2(r.av, r3g_mi::fmin2(r.bv, r.cv)));
                hi[0] = r3g_mi::fmax2(hi[0], r3g_mi::fmax2(r.au, r3g_mi::fmax2(r.bu, r.cu)));
                hi[1] = r3g_mi::fmax2(hi[1], r3g_mi::fmax2(r.av, r3g_mi::fmax2(r.bv, r.cv)));
                if (!r3g_mi::rec_usable(r)) r.ia = -1;     // zero projected area: takes part in nothing
            } else {
                ++skipped;
                r.ia = -1;
            }
        }
        recs[f] = r;
    }
    unsigned elo[2], ehi[2];
    for (int a = 0; a < 2; ++a) {
        elo[a] = r3g_mi::enc_float(lo[a]);
        ehi[a] = r3g_mi::enc_float(hi[a]);
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned l = __shfl_xor(elo[a], d, 64), h = __shfl_xor(ehi[a], d, 64);
            elo[a] = l < elo[a] ? l : elo[a];
            ehi[a] = h > ehi[a] ? h : ehi[a];
        }
    }
    skipped = wave_sum_u64(skipped);
    const unsigned long long anybad = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 2; ++a) {
            atomicMin(&sm->box[a], elo[a]);
            atomicMax(&sm->box[2 + a], ehi[a]);
        }
        if (skipped) atomicAdd(&sm->skipped, skipped);
        if (anybad) atomicOr(&sm->bad_index, 1u);
    }
}

__global__ __launch_bounds__(kT) void mi_count_pairs(const Rec* __restrict__ recs, int64_t nf, Grid2 g, MeshinsideSmall* __restrict__ sm) {
    unsigned long long n = 0;
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const Rec r = recs[f];
        if (r.ia >= 0) n += (unsigned long long)r3g_mi::rec_pairs(g, r);
    }
    n = wave_sum_u64(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&sm->pairs, n);
}

// FILL == false: counts[col] += 1;  FILL == true: pairs[starts[col] + cursor[col]++] = f
template <bool FILL>
__global__ __launch_bounds__(kT) void mi_bin(const Rec* __restrict__ recs, int64_t nf, Grid2 g, unsigned* __restrict__ counts,
                                             const unsigned* __restrict__ starts, int32_t* __restrict__ pairs) {
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const Rec r = recs[f];
        if (r.ia < 0) continue;
        int lo[2], hi[2];
        r3g_mi::rec_range(g, r, lo, hi);
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
                const int col = r3g_mi::col_index(g, x, y);
                const unsigned slot = atomicAdd(&counts[col], 1u);
                if (FILL) pairs[starts[col] + slot] = (int32_t)f;
            }
    }
}

// exclusive scan of one tile of ITEMS * kT elements per block (in place allowed); the tile's total goes to sums[block]
template <int ITEMS>
__global__ __launch_bounds__(kT) void mi_scan_tile(const unsigned* in, unsigned* out, int64_t n, unsigned* sums) {
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

__global__ __launch_bounds__(kT) void mi_scan_add(unsigned* out, int64_t n, const unsigned* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * kScanTile + threadIdx.x;
    const unsigned add = sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const int64_t j = i + (int64_t)k * kT;
        if (j < n) out[j] += add;
    }
}

__global__ __launch_bounds__(kT) void mi_query(Grid2 g, int axis, const Rec* __restrict__ recs, const unsigned* __restrict__ starts,
                                               const int32_t* __restrict__ pairs, const float* __restrict__ pts, int64_t n,
                                               int32_t* __restrict__ count, MeshinsideSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    uint32_t ntests = 0;
    if (i < n) count[i] = r3g_mi::count_crossings(g, axis, recs, starts, pairs, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], &ntests);
    const unsigned long long t = wave_sum_u64((unsigned long long)ntests);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(&sm->tests, t);
}

#define R3G_HIP(x)                         \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

std::atomic<int64_t> g_tests{0};

}  // namespace

static_assert(sizeof(Rec) == 48, "face records are three 16-byte loads");
static_assert(sizeof(MeshinsideSmall) == 48, "MeshinsideSmall travels through the 64-byte pinned buffer");
static_assert(((size_t)r3g_mi::kMaxRes * r3g_mi::kMaxRes + 1 + kScanTile - 1) / kScanTile <= (size_t)kT * kSumItems,
              "one block scans the tile sums");

size_t meshinside_workspace_bytes(int64_t nf, int res_max, MeshinsideLayout* lay) {
    const size_t cols1 = (size_t)res_max * res_max + 1;
    const size_t tiles = ((size_t)cols1 + kScanTile - 1) / kScanTile;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 0;
    lay->off_small = o, o += 256;
    lay->off_recs = o, o += up(sizeof(Rec) * (size_t)nf);
    lay->off_counts = o, o += up(4 * cols1);
    lay->off_starts = o, o += up(4 * cols1);
    lay->off_sums = o, o += up(4 * tiles);
    lay->total = o;
    return o;
}

hipError_t meshinside_records(char* ws, const MeshinsideLayout& lay, const float* verts, int64_t nv, const int32_t* faces,
                              int64_t nf, int axis, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small, 0, sizeof(MeshinsideSmall), s));
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(MeshinsideSmall, box), 0xFF, 8, s));     // lo[2] = the largest code
    hipLaunchKernelGGL(mi_records, dim3(grid_for(nf)), dim3(kT), 0, s, verts, nv, faces, nf, axis, (Rec*)(ws + lay.off_recs),
                       (MeshinsideSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t meshinside_count_pairs(char* ws, const MeshinsideLayout& lay, int64_t nf, const Grid2& g, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(MeshinsideSmall, pairs), 0, 8, s));
    hipLaunchKernelGGL(mi_count_pairs, dim3(grid_for(nf)), dim3(kT), 0, s, (const Rec*)(ws + lay.off_recs), nf, g,
                       (MeshinsideSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t meshinside_fill(char* ws, const MeshinsideLayout& lay, int64_t nf, const Grid2& g, int32_t* pairs, hipStream_t s) {
    const int64_t n1 = (int64_t)g.res * g.res + 1;          // the extra element receives the total
    const unsigned tiles = nblocks(n1, kScanTile);
    if (tiles > (unsigned)(kT * kSumItems)) return hipErrorInvalidValue;
    unsigned* counts = (unsigned*)(ws + lay.off_counts);
    unsigned* starts = (unsigned*)(ws + lay.off_starts);
    unsigned* sums = (unsigned*)(ws + lay.off_sums);
    const Rec* recs = (const Rec*)(ws + lay.off_recs);
    R3G_HIP(hipMemsetAsync(counts, 0, 4 * (size_t)n1, s));
    hipLaunchKernelGGL(mi_bin<false>, dim3(grid_for(nf)), dim3(kT), 0, s, recs, nf, g, counts, (const unsigned*)nullptr,
                       (int32_t*)nullptr);
    hipLaunchKernelGGL(mi_scan_tile<kScanItems>, dim3(tiles), dim3(kT), 0, s, (const unsigned*)counts, starts, n1, sums);
    hipLaunchKernelGGL(mi_scan_tile<kSumItems>, dim3(1), dim3(kT), 0, s, (const unsigned*)sums, sums, (int64_t)tiles,
                       (unsigned*)nullptr);
    hipLaunchKernelGGL(mi_scan_add, dim3(tiles), dim3(kT), 0, s, starts, n1, (const unsigned*)sums);
    R3G_HIP(hipMemsetAsync(counts, 0, 4 * (size_t)n1, s));
    hipLaunchKernelGGL(mi_bin<true>, dim3(grid_for(nf)), dim3(kT), 0, s, recs, nf, g, counts, (const unsigned*)starts, pairs);
    return hipGetLastError();
}

hipError_t meshinside_query(char* ws, const MeshinsideLayout& lay, const Grid2& g, int axis, const int32_t* pairs,
                            const float* points, int64_t n, int32_t* count, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(MeshinsideSmall, tests), 0, 8, s));
    hipLaunchKernelGGL(mi_query, dim3(nblocks(n, kT)), dim3(kT), 0, s, g, axis, (const Rec*)(ws + lay.off_recs),
                       (const unsigned*)(ws + lay.off_starts), pairs, points, n, count, (MeshinsideSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

void meshinside_add_tests(int64_t n) { g_tests += n; }
int64_t meshinside_tests_total() { return g_tests.load(); }

}  // namespace r3g
