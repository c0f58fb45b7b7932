// meshdist_kernels.hip -- exact nearest-triangle query on a uniform grid in CSR form.
//
// Build: records (index check, padded copies, bounding box) -> pair count per candidate resolution (host halves it while
// the total is too high) -> per-cell count -> exclusive scan -> fill.  Query: one lane per point walks its own Chebyshev
// rings (meshdist_core.h).  Integer atomics only; their order decides nothing: the bounding box is a min / max, the counts
// are sums, and the order of the faces inside a cell is absorbed by the (dist2, face) comparison.
#include <hip/hip_runtime.h>

#include <atomic>

#pragma clang fp contract(off)

#define R3G_MD_HD static __host__ __device__ __forceinline__
#include "meshdist_kernels.h"

namespace r3g {
namespace {

using r3g_md::Grid;
using r3g_md::Tri;

constexpr int kT = 256;
constexpr int kScanItems = 8;                  // per thread: a scan tile is 2048 elements
constexpr int kScanTile = kT * kScanItems;
constexpr int kSumItems = 40;                  // one block scans the tile sums: 2^24 cells + 1 make 8193 tiles, 10240 fit

inline unsigned nblocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
inline unsigned grid_for(int64_t n) {
    const unsigned b = nblocks(n, kT);
    return b < 1 ? 1 : (b > 4096 ? 4096 : b);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(kT) void md_records(const float* __restrict__ verts, int64_t nv, const int32_t* __restrict__ faces,
                                                 int64_t nf, Tri* __restrict__ tris, MeshdistSmall* __restrict__ sm) {
    float lo[3] = {r3g_md::kInf, r3g_md::kInf, r3g_md::kInf}, hi[3] = {-r3g_md::kInf, -r3g_md::kInf, -r3g_md::kInf};
    unsigned long long skipped = 0;
    bool bad = false;
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        Tri t;
        t.valid = 0;
        t.pad1 = t.pad2 = 0;
        t.ax = t.ay = t.az = t.bx = t.by = t.bz = t.cx = t.cy = t.cz = 0.0f;
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) {
            bad = true;                                   // nothing is read through a bad index
        } else {
            t.ax = verts[3 * (int64_t)i0], t.ay = verts[3 * (int64_t)i0 + 1], t.az = verts[3 * (int64_t)i0 + 2];
            t.bx = verts[3 * (int64_t)i1], t.by = verts[3 * (int64_t)i1 + 1], t.bz = verts[3 * (int64_t)i1 + 2];
            t.cx = verts[3 * (int64_t)i2], t.cy = verts[3 * (int64_t)i2 + 1], t.cz = verts[3 * (int64_t)i2 + 2];
            if (r3g_md::tri_finite(t)) {
                t.valid = 1;
                lo[0] = r3g_md::fmin2(lo[0], r3g_md::fmin2(t.ax, r3g_md::fmin2(t.bx, t.cx)));
                lo[1] = r3g_md::fmin2(lo[1], r3g_md::fmin2(t.ay, r3g_md::fmin2(t.by, t.cy)));
                lo[2] = r3g_md::fmin2(lo[2], r3g_md::fmin2(t.az, r3g_md::fmin2(t.bz, t.cz)));
                hi[0] = r3g_md::fmax2(hi[0], r3g_md::fmax2(t.ax, r3g_md::fmax2(t.bx, t.cx)));
                hi[1] = r3g_md::fmax2(hi[1], r3g_md::fmax2(t.ay, r3g_md::fmax2(t.by, t.cy)));
                hi[2] = r3g_md::fmax2(hi[2], r3g_md::fmax2(t.az, r3g_md::fmax2(t.bz, t.cz)));
            } else {
                ++skipped;
            }
        }
        tris[f] = t;
    }
    unsigned elo[3], ehi[3];
    for (int a = 0; a < 3; ++a) {
        elo[a] = r3g_md::enc_float(lo[a]);
        ehi[a] = r3g_md::enc_float(hi[a]);
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned l = __shfl_xor(elo[a], d, 64), h = __shfl_xor(ehi[a], d, 64);
            elo[a] = l < elo[a] ? l : elo[a];
            ehi[a] = h > ehi[a] ? h : ehi[a];
        }
    }
    skipped = wave_sum_u64(skipped);
    const unsigned long long anybad = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) {
            atomicMin(&sm->box[a], elo[a]);
            atomicMax(&sm->box[3 + a], ehi[a]);
        }
        if (skipped) atomicAdd(&sm->skipped, skipped);
        if (anybad) atomicOr(&sm->bad_index, 1u);
    }
}

__global__ __launch_bounds__(kT) void md_count_pairs(const Tri* __restrict__ tris, int64_t nf, Grid g, MeshdistSmall* __restrict__ sm) {
    unsigned long long n = 0;
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const Tri t = tris[f];
        if (t.valid) n += (unsigned long long)r3g_md::tri_pairs(g, t);
    }
    n = wave_sum_u64(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&sm->pairs, n);
}

// FILL == false: counts[cell] += 1;  FILL == true: pairs[starts[cell] + cursor[cell]++] = f
template <bool FILL>
__global__ __launch_bounds__(kT) void md_bin(const Tri* __restrict__ tris, int64_t nf, Grid g, unsigned* __restrict__ counts,
                                             const unsigned* __restrict__ starts, int32_t* __restrict__ pairs) {
    for (int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x; f < nf; f += (int64_t)gridDim.x * kT) {
        const Tri t = tris[f];
        if (!t.valid) continue;
        int lo[3], hi[3];
        r3g_md::tri_range(g, t, lo, hi);
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int x = lo[0]; x <= hi[0]; ++x) {
                    const int cell = r3g_md::cell_index(g, x, y, z);
                    const unsigned slot = atomicAdd(&counts[cell], 1u);
                    if (FILL) pairs[starts[cell] + slot] = (int32_t)f;
                }
    }
}

// exclusive scan of one tile of ITEMS * kT elements per block (in place allowed); the tile's total goes to sums[block]
template <int ITEMS>
__global__ __launch_bounds__(kT) void md_scan_tile(const unsigned* in, unsigned* out, int64_t n, unsigned* sums) {
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

__global__ __launch_bounds__(kT) void md_scan_add(unsigned* out, int64_t n, const unsigned* __restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * kScanTile + threadIdx.x;
    const unsigned add = sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const int64_t j = i + (int64_t)k * kT;
        if (j < n) out[j] += add;
    }
}

__global__ __launch_bounds__(kT) void md_query(Grid g, const Tri* __restrict__ tris, const unsigned* __restrict__ starts,
                                               const int32_t* __restrict__ pairs, const float* __restrict__ pts, int64_t n,
                                               float* __restrict__ dist2, int32_t* __restrict__ face, MeshdistSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    uint32_t ntests = 0;
    if (i < n) {
        float d;
        int32_t f;
        r3g_md::nearest(g, tris, starts, pairs, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], &d, &f, &ntests);
        dist2[i] = d;
        face[i] = f;
    }
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

static_assert(sizeof(Tri) == 48, "triangle records are three 16-byte loads");
static_assert(sizeof(MeshdistSmall) == 56, "MeshdistSmall travels through the 64-byte pinned buffer");

size_t meshdist_workspace_bytes(int64_t nf, int res_max, MeshdistLayout* lay) {
    const size_t cells1 = (size_t)res_max * res_max * res_max + 1;
    const size_t tiles = ((size_t)cells1 + kScanTile - 1) / kScanTile;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 0;
    lay->off_small = o, o += 256;
    lay->off_tris = o, o += up(sizeof(Tri) * (size_t)nf);
    lay->off_counts = o, o += up(4 * cells1);
    lay->off_starts = o, o += up(4 * cells1);
    lay->off_sums = o, o += up(4 * tiles);
    lay->total = o;
    return o;
}

hipError_t meshdist_records(char* ws, const MeshdistLayout& lay, const float* verts, int64_t nv, const int32_t* faces,
                            int64_t nf, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small, 0, sizeof(MeshdistSmall), s));
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(MeshdistSmall, box), 0xFF, 12, s));     // lo[3] = the largest code
    hipLaunchKernelGGL(md_records, dim3(grid_for(nf)), dim3(kT), 0, s, verts, nv, faces, nf, (Tri*)(ws + lay.off_tris),
                       (MeshdistSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t meshdist_count_pairs(char* ws, const MeshdistLayout& lay, int64_t nf, const Grid& g, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(MeshdistSmall, pairs), 0, 8, s));
    hipLaunchKernelGGL(md_count_pairs, dim3(grid_for(nf)), dim3(kT), 0, s, (const Tri*)(ws + lay.off_tris), nf, g,
                       (MeshdistSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t meshdist_fill(char* ws, const MeshdistLayout& lay, int64_t nf, const Grid& g, int32_t* pairs, hipStream_t s) {
    const int64_t n1 = (int64_t)g.res * g.res * g.res + 1;          // the extra element receives the total
    const unsigned tiles = nblocks(n1, kScanTile);
    if (tiles > (unsigned)(kT * kSumItems)) return hipErrorInvalidValue;
    unsigned* counts = (unsigned*)(ws + lay.off_counts);
    unsigned* starts = (unsigned*)(ws + lay.off_starts);
    unsigned* sums = (unsigned*)(ws + lay.off_sums);
    const Tri* tris = (const Tri*)(ws + lay.off_tris);
    R3G_HIP(hipMemsetAsync(counts, 0, 4 * (size_t)n1, s));
    hipLaunchKernelGGL(md_bin<false>, dim3(grid_for(nf)), dim3(kT), 0, s, tris, nf, g, counts, (const unsigned*)nullptr,
                       (int32_t*)nullptr);
    hipLaunchKernelGGL(md_scan_tile<kScanItems>, dim3(tiles), dim3(kT), 0, s, (const unsigned*)counts, starts, n1, sums);
    hipLaunchKernelGGL(md_scan_tile<kSumItems>, dim3(1), dim3(kT), 0, s, (const unsigned*)sums, sums, (int64_t)tiles,
                       (unsigned*)nullptr);
    hipLaunchKernelGGL(md_scan_add, dim3(tiles), dim3(kT), 0, s, starts, n1, (const unsigned*)sums);
    R3G_HIP(hipMemsetAsync(counts, 0, 4 * (size_t)n1, s));
    hipLaunchKernelGGL(md_bin<true>, dim3(grid_for(nf)), dim3(kT), 0, s, tris, nf, g, counts, (const unsigned*)starts, pairs);
    return hipGetLastError();
}

hipError_t meshdist_query(char* ws, const MeshdistLayout& lay, const Grid& g, const int32_t* pairs, const float* points,
                          int64_t n, float* dist2, int32_t* face, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small + offsetof(MeshdistSmall, tests), 0, 8, s));
    hipLaunchKernelGGL(md_query, dim3(nblocks(n, kT)), dim3(kT), 0, s, g, (const Tri*)(ws + lay.off_tris),
                       (const unsigned*)(ws + lay.off_starts), pairs, points, n, dist2, face, (MeshdistSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

void meshdist_add_tests(int64_t n) { g_tests += n; }
int64_t meshdist_tests_total() { return g_tests.load(); }

}  // namespace r3g
