// plane_kernels.hip -- the plane fit on the device (the definition is plane_core.h).
//
// pl_table:   one lane per hypothesis: (p0, unit normal, valid) from its triple, and count[h] = 0.
// pl_count:   the hot path.  A block keeps kCountPoints = 1024 rows in registers, widened to float64 once (a row that is not
//             usable, or past n, is held as NaN: its distance compares false), and its waves walk the table.  The entry is the
//             same for the whole wave, so it comes through the scalar cache; a test is 3 subtractions, 3 products, 2 sums, one
//             compare.  A wave's count of a hypothesis is four ballots and popcounts; lane j keeps the count of the j-th
//             hypothesis of a tile of 64, the four waves meet in LDS once per tile and the block adds its 64 totals to
//             count[] with integer atomics (none where the total is 0).  Integers: the result does not depend on the schedule.
//             Small clouds leave CUs idle with one block per 1024 rows, so blockIdx.y splits the table (a split that depends
//             on n, n_hyp and the CU count alone); rows are then read once per split, from a cloud of at most 6 MB.
// pl_argmax:  one block over the table: max of r3g_pl::winner_key over the valid entries, the valid count, the winner's entry.
// pl_mask:    one lane per row: the winner's inlier test, uint8.
// pl_sums<P>: one block per chunk of 1024 rows, pl_tree<P>: one block over the chunks' partials; P = 0 the coordinate sums
//             and the centroid, P = 1 the scatter about it.  The order is plane_core.h's; no floating-point atomics.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_PL_HD static __host__ __device__ __forceinline__
#include "plane_kernels.h"

namespace r3g {
namespace {

using r3g_pl::Hyp;
using r3g_pl::kBlock;
using r3g_pl::kCountPoints;
using r3g_pl::kHypTile;
using r3g_pl::kMomChunk;
using r3g_pl::kPerLane;

static_assert(kBlock == 256 && kHypTile == 64 && kMomChunk == 4 * kBlock, "four waves; a tile is one count per lane; four rows a slot");
static_assert(sizeof(Hyp) == 56 && sizeof(PlaneSmall) == 192 && sizeof(PlanePartial) == 64, "layouts the host reads back");

__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffu), d, 64), hi = __shfl_xor((unsigned)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void pl_table(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ triples, int n_hyp,
                                                   Hyp* __restrict__ hyp, uint32_t* __restrict__ count) {
    const int h = blockIdx.x * kBlock + threadIdx.x;
    if (h >= n_hyp) return;
    hyp[h] = r3g_pl::make_hyp(pts, n, triples[3 * h], triples[3 * h + 1], triples[3 * h + 2]);
    count[h] = 0u;
}

__global__ __launch_bounds__(kBlock) void pl_count(const float* __restrict__ pts, int64_t n, const Hyp* __restrict__ hyp, int n_hyp,
                                                   int hyp_per_y, double threshold, uint32_t* __restrict__ count,
                                                   PlaneSmall* __restrict__ small) {
    __shared__ unsigned sh[4][kHypTile];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * kCountPoints + threadIdx.x;
    double qx[kPerLane], qy[kPerLane], qz[kPerLane];
    unsigned n_usable = 0;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
        const int64_t i = base + (int64_t)k * kBlock;
        bool ok = false;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (i < n) {
            x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
            ok = r3g_pl::usable(x, y, z);
        }
        const double nan = __builtin_nan("");
        qx[k] = ok ? (double)x : nan, qy[k] = ok ? (double)y : nan, qz[k] = ok ? (double)z : nan;
        n_usable += (unsigned)__popcll(__ballot(ok));
    }
    if (blockIdx.y == 0 && lane == 0 && n_usable) atomicAdd(&small->usable, (unsigned long long)n_usable);
    const int h_lo = blockIdx.y * hyp_per_y;
    const int h_hi = min(n_hyp, h_lo + hyp_per_y);
    for (int t0 = h_lo; t0 < h_hi; t0 += kHypTile) {
        const int m = min(kHypTile, h_hi - t0);
        unsigned mine = 0;
        for (int j = 0; j < m; ++j) {
            const Hyp* __restrict__ e = hyp + (t0 + j);      // the same entry for every lane: scalar loads
            unsigned c = 0;
            if (e->valid) {
                const double p0[3] = {e->p0[0], e->p0[1], e->p0[2]}, nr[3] = {e->n[0], e->n[1], e->n[2]};
#pragma unroll
                for (int k = 0; k < kPerLane; ++k) c += (unsigned)__popcll(__ballot(r3g_pl::inlier(p0, nr, qx[k], qy[k], qz[k], threshold)));
            }
            if (lane == j) mine = c;
        }
        sh[wave][lane] = mine;
        __syncthreads();
        if ((int)threadIdx.x < m) {
            const unsigned total = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
            if (total) atomicAdd(&count[t0 + threadIdx.x], total);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void pl_argmax(const Hyp* __restrict__ hyp, const uint32_t* __restrict__ count, int n_hyp,
                                                    PlaneSmall* __restrict__ small) {
    __shared__ unsigned long long shk[4];
    __shared__ unsigned shv[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long key = 0;
    unsigned valid = 0;
    for (int h = threadIdx.x; h < n_hyp; h += kBlock)
        if (hyp[h].valid) {
            const unsigned long long k = r3g_pl::winner_key(count[h], (uint32_t)h);
            key = k > key ? k : key;
            ++valid;
        }
    key = wave_max_u64(key);
    for (int d = 32; d >= 1; d >>= 1) valid += __shfl_xor(valid, d, 64);
    if (lane == 0) shk[wave] = key, shv[wave] = valid;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) key = shk[w] > key ? shk[w] : key;
        small->key = key;
        small->valid = shv[0] + shv[1] + shv[2] + shv[3];
        small->pad = 0;
        if (key) small->best = hyp[r3g_pl::key_h(key)];      // (otherwise the zeros plane_table left there)
    }
}

__global__ __launch_bounds__(kBlock) void pl_mask(const float* __restrict__ pts, int64_t n, const PlaneSmall* __restrict__ small,
                                                  double threshold, uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const Hyp* __restrict__ e = &small->best;
    bool in = false;
    if (e->valid) {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const double p0[3] = {e->p0[0], e->p0[1], e->p0[2]}, nr[3] = {e->n[0], e->n[1], e->n[2]};
        in = r3g_pl::usable(x, y, z) && r3g_pl::inlier(p0, nr, (double)x, (double)y, (double)z, threshold);
    }
    mask[i] = in ? 1 : 0;
}

// the block's tree over its 256 slots (plane_core.h): butterfly per wave, then ((g0 + g1) + g2) + g3 by the threads k < K
template <int K>
__device__ __forceinline__ void block_tree(const double (&acc)[K], unsigned long long cnt, unsigned long long skip, double (&sh)[4][6],
                                           unsigned long long (&shi)[4][2], PlanePartial* out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum_f64(acc[k]);
        if (lane == 0) sh[wave][k] = v;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        cnt += ((unsigned long long)__shfl_xor((unsigned)(cnt >> 32), d, 64) << 32) | __shfl_xor((unsigned)(cnt & 0xffffffffu), d, 64);
        skip += ((unsigned long long)__shfl_xor((unsigned)(skip >> 32), d, 64) << 32) | __shfl_xor((unsigned)(skip & 0xffffffffu), d, 64);
    }
    if (lane == 0) shi[wave][0] = cnt, shi[wave][1] = skip;
    __syncthreads();
    if (threadIdx.x < 6) out->v[threadIdx.x] = (int)threadIdx.x < K ? ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x] : 0.0;
    if (threadIdx.x == 64) out->n = shi[0][0] + shi[1][0] + shi[2][0] + shi[3][0];
    if (threadIdx.x == 65) out->skipped = shi[0][1] + shi[1][1] + shi[2][1] + shi[3][1];
}

// P = 0: sums of the coordinates; P = 1: sums of the six products about small->mom.c
template <int P>
__global__ __launch_bounds__(kBlock) void pl_sums(const float* __restrict__ pts, int64_t n, const uint8_t* __restrict__ mask,
                                                  const PlaneSmall* __restrict__ small, PlanePartial* __restrict__ partial) {
    constexpr int K = P == 0 ? 3 : 6;
    __shared__ double sh[4][6];
    __shared__ unsigned long long shi[4][2];
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (P == 1) cx = small->mom.c[0], cy = small->mom.c[1], cz = small->mom.c[2];
    unsigned long long cnt = 0, skip = 0;
#pragma unroll
    for (int r = 0; r < kMomChunk / kBlock; ++r) {
        const int64_t i = (int64_t)blockIdx.x * kMomChunk + r * kBlock + threadIdx.x;
        double t[K];
#pragma unroll
        for (int k = 0; k < K; ++k) t[k] = 0.0;
        if (i < n && (!mask || mask[i])) {
            const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
            if (r3g_pl::usable(x, y, z)) {
                ++cnt;
                if constexpr (P == 0) {
                    t[0] = (double)x, t[1] = (double)y, t[2] = (double)z;
                } else {
                    const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
                    t[0] = dx * dx, t[1] = dx * dy, t[2] = dx * dz;
                    t[3] = dy * dy, t[4] = dy * dz, t[5] = dz * dz;
                }
            } else {
                ++skip;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = acc[k] + t[k];
    }
    block_tree<K>(acc, cnt, skip, sh, shi, partial + blockIdx.x);
}

template <int P>
__global__ __launch_bounds__(kBlock) void pl_tree(const PlanePartial* __restrict__ partial, int64_t nb, PlaneSmall* __restrict__ small,
                                                  PlanePartial* __restrict__ scratch) {
    constexpr int K = P == 0 ? 3 : 6;
    __shared__ double sh[4][6];
    __shared__ unsigned long long shi[4][2];
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    unsigned long long cnt = 0, skip = 0;
    for (int64_t b = threadIdx.x; b < nb; b += kBlock) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = acc[k] + partial[b].v[k];
        cnt += partial[b].n, skip += partial[b].skipped;
    }
    block_tree<K>(acc, cnt, skip, sh, shi, scratch);
    __syncthreads();
    if (threadIdx.x == 0) {
        r3g_pl::Moments* m = &small->mom;
        if (P == 0) {
            m->n = scratch->n, m->skipped = scratch->skipped;
            for (int a = 0; a < 3; ++a) {
                m->sum[a] = scratch->v[a];
                m->c[a] = scratch->n ? scratch->v[a] / (double)scratch->n : 0.0;
            }
        } else {
            for (int a = 0; a < 6; ++a) m->s[a] = scratch->v[a];
        }
    }
}

}  // namespace

size_t plane_workspace_bytes(int64_t n_points, int64_t n_hyp, bool own_count, bool own_mask, PlaneLayout* lay) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t o = 0;
    lay->off_small = o, o += up(sizeof(PlaneSmall));
    lay->off_hyp = o, o += up(sizeof(Hyp) * (size_t)n_hyp);
    lay->off_count = o, o += own_count ? up(4 * (size_t)n_hyp) : 0;      // (a caller's d_count / d_mask is written directly)
    lay->off_mask = o, o += own_mask ? up((size_t)n_points) : 0;
    lay->off_partial = o, o += up(sizeof(PlanePartial) * ((size_t)r3g_pl::mom_chunks(n_points) + 1));      // [0] is the tree's scratch
    lay->total = o;
    return o;
}

hipError_t plane_table(char* ws, const PlaneLayout& lay, const float* points, int64_t n, const int32_t* triples, int n_hyp, uint32_t* count,
                       hipStream_t s) {
    hipError_t e = hipMemsetAsync(ws + lay.off_small, 0, sizeof(PlaneSmall), s);
    if (e != hipSuccess || n_hyp == 0) return e;
    hipLaunchKernelGGL(pl_table, dim3((unsigned)((n_hyp + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, points, n, triples, n_hyp,
                       (Hyp*)(ws + lay.off_hyp), count);
    return hipGetLastError();
}

hipError_t plane_count(char* ws, const PlaneLayout& lay, const float* points, int64_t n, int n_hyp, double threshold, uint32_t* count,
                       int num_cu, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const int64_t nbx = (n + kCountPoints - 1) / kCountPoints;
    const int tiles = (n_hyp + kHypTile - 1) / kHypTile;
    const int64_t want = 2 * (int64_t)(num_cu > 0 ? num_cu : 256);
    int ny = 1;
    if (nbx < want) ny = (int)((want + nbx - 1) / nbx);
    if (ny > tiles) ny = tiles;
    if (ny < 1) ny = 1;
    const int hyp_per_y = ((tiles + ny - 1) / ny) * kHypTile;
    hipLaunchKernelGGL(pl_count, dim3((unsigned)nbx, (unsigned)ny), dim3(kBlock), 0, s, points, n, (const Hyp*)(ws + lay.off_hyp), n_hyp,
                       hyp_per_y > 0 ? hyp_per_y : kHypTile, threshold, count, (PlaneSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t plane_winner(char* ws, const PlaneLayout& lay, const float* points, int64_t n, int n_hyp, double threshold, const uint32_t* count,
                        uint8_t* mask, hipStream_t s) {
    PlaneSmall* small = (PlaneSmall*)(ws + lay.off_small);
    hipLaunchKernelGGL(pl_argmax, dim3(1), dim3(kBlock), 0, s, (const Hyp*)(ws + lay.off_hyp), count, n_hyp, small);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(pl_mask, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, points, n, (const PlaneSmall*)small, threshold,
                       mask);
    return hipGetLastError();
}

hipError_t plane_moments(char* ws, const PlaneLayout& lay, const float* points, int64_t n, const uint8_t* mask, hipStream_t s) {
    PlaneSmall* small = (PlaneSmall*)(ws + lay.off_small);
    PlanePartial* scratch = (PlanePartial*)(ws + lay.off_partial);
    PlanePartial* partial = scratch + 1;
    const int64_t nb = r3g_pl::mom_chunks(n);
    hipError_t e;
    if (nb) {
        hipLaunchKernelGGL(pl_sums<0>, dim3((unsigned)nb), dim3(kBlock), 0, s, points, n, mask, (const PlaneSmall*)small, partial);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pl_tree<0>, dim3(1), dim3(kBlock), 0, s, (const PlanePartial*)partial, nb, small, scratch);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (nb) {
        hipLaunchKernelGGL(pl_sums<1>, dim3((unsigned)nb), dim3(kBlock), 0, s, points, n, mask, (const PlaneSmall*)small, partial);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pl_tree<1>, dim3(1), dim3(kBlock), 0, s, (const PlanePartial*)partial, nb, small, scratch);
    return hipGetLastError();
}

}  // namespace r3g
