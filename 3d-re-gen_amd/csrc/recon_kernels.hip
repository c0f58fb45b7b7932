// recon_kernels.hip -- Poisson surface on a uniform lattice: splat, divergence, geometric multigrid, sample.
//
// Splat and sample: one lane per point; the sums are 64-bit integer atomics, so their order decides nothing.
// Solver: stencil passes, one lane per node of the flat index (i2 fastest: a wave reads and writes consecutive floats), float32,
// no atomics; a sweep reads one buffer and writes the other.  The passes are bound by HBM traffic (a sweep reads x and b and
// writes x once; the six neighbours come from cache), so nothing is fused through LDS.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_RC_HD static __host__ __device__ __forceinline__
#include "mesh_launch.h"
#include "recon_kernels.h"

namespace r3g {
namespace {

using r3g_rc::Lattice;

struct AtomicAdd {
    unsigned long long* ch;
    int64_t n3;
    __device__ __forceinline__ void operator()(int c, int64_t at, int64_t v) const {
        atomicAdd(ch + c * n3 + at, (unsigned long long)v);
    }
};

__global__ __launch_bounds__(kT) void rc_splat(const float* __restrict__ points, const float* __restrict__ normals, int64_t n, Lattice L,
                                               unsigned long long* __restrict__ channels, ReconSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long used = 0;
    if (i < n) {
        const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        const float nr[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
        if (r3g_rc::usable(p, nr)) {
            AtomicAdd add{channels, (int64_t)L.n * L.n * L.n};
            r3g_rc::splat_point(L, p, nr, add);
            used = 1;
        }
    }
    used = wave_sum_u64(used);
    if ((threadIdx.x & 63) == 0 && used) atomicAdd(&sm->usable, used);
}

// flat node index -> (i0, i1, i2)
__device__ __forceinline__ bool node_of(int64_t at, int n, int* i0, int* i1, int* i2) {
    if (at >= (int64_t)n * n * n) return false;
    const int row = (int)(at / n);
    *i2 = (int)(at - (int64_t)row * n);
    *i0 = row / n;
    *i1 = row - *i0 * n;
    return true;
}

__global__ __launch_bounds__(kT) void rc_rhs(const int64_t* __restrict__ channels, Lattice L, float* __restrict__ b) {
    const int64_t at = (int64_t)blockIdx.x * kT + threadIdx.x;
    int i0, i1, i2;
    if (node_of(at, L.n, &i0, &i1, &i2)) b[at] = r3g_rc::rhs_node(channels, L, i0, i1, i2);
}

__global__ __launch_bounds__(kT) void rc_smooth(const float* __restrict__ x, const float* __restrict__ b, float* __restrict__ out, int n,
                                                float h2) {
    const int64_t at = (int64_t)blockIdx.x * kT + threadIdx.x;
    int i0, i1, i2;
    if (node_of(at, n, &i0, &i1, &i2)) out[at] = r3g_rc::smooth_node(x, b, n, h2, i0, i1, i2);
}

// one lane per COARSE node: its right-hand side from the fine residual, and its start value 0
__global__ __launch_bounds__(kT) void rc_restrict(const float* __restrict__ xf, const float* __restrict__ bf, int nf, float inv_h2f,
                                                  float* __restrict__ bc, float* __restrict__ xc) {
    const float w4[4] = R3G_RC_FULL_WEIGHTS;
    const int64_t at = (int64_t)blockIdx.x * kT + threadIdx.x;
    int i0, i1, i2;
    if (node_of(at, (nf + 1) / 2, &i0, &i1, &i2)) {
        bc[at] = r3g_rc::restrict_node(xf, bf, nf, inv_h2f, w4, i0, i1, i2);
        xc[at] = 0.0f;
    }
}

// in place: a lane reads and writes its own fine node only
__global__ __launch_bounds__(kT) void rc_prolong(float* __restrict__ xf, const float* __restrict__ xc, int nf) {
    const int64_t at = (int64_t)blockIdx.x * kT + threadIdx.x;
    int i0, i1, i2;
    if (node_of(at, nf, &i0, &i1, &i2)) xf[at] = r3g_rc::prolong_node(xf, xc, nf, i0, i1, i2);
}

// the 3^3 level: its one interior node is number 13
__global__ void rc_coarsest(float* __restrict__ x, const float* __restrict__ b, float h2) {
    if (blockIdx.x == 0 && threadIdx.x == 0) x[13] = r3g_rc::coarsest_value(b[13], h2);
}

struct LoadFixed {
    const int64_t* ch;
    __device__ __forceinline__ float operator()(int64_t at) const { return r3g_rc::from_fixed(ch[at]); }
};
struct LoadFloat {
    const float* x;
    __device__ __forceinline__ float operator()(int64_t at) const { return x[at]; }
};

template <class Load>
__global__ __launch_bounds__(kT) void rc_sample(Load load, const float* __restrict__ points, const float* __restrict__ normals, int64_t n,
                                                Lattice L, float* __restrict__ out, ReconSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long used = 0, sum = 0;
    if (i < n) {
        const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        bool ok = r3g_rc::finite3(p);
        if (ok && normals) {
            const float nr[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
            ok = r3g_rc::usable(p, nr);
        }
        float v = __builtin_nanf("");
        if (ok) {
            v = r3g_rc::sample_point(L, p, load);
            if (r3g_rc::finite1(v)) used = 1, sum = (unsigned long long)r3g_rc::to_fixed(v);
        }
        if (out) out[i] = v;
    }
    used = wave_sum_u64(used), sum = wave_sum_u64(sum);
    if ((threadIdx.x & 63) == 0 && used) atomicAdd(&sm->usable, used), atomicAdd(&sm->sum, sum);
}

}  // namespace

hipError_t recon_splat(ReconState* st, const float* points, const float* normals, int64_t n, hipStream_t s) {
    const int depth = st->lat.depth;
    R3G_HIP(hipMemsetAsync(st->channels.p, 0, recon_channels_bytes(depth), s));
    hipLaunchKernelGGL(rc_splat, dim3(nblocks(n, kT)), dim3(kT), 0, s, points, normals, n, st->lat, (unsigned long long*)st->channels.p,
                       (ReconSmall*)(st->channels.p + recon_small_offset(depth)));
    return hipGetLastError();
}

hipError_t recon_solve(ReconState* st, int cycles, hipStream_t s) {
    const int depth = st->lat.depth;
    float* lv = (float*)st->levels.p;
    auto buf = [&](int d, int which) { return lv + recon_level_offset(depth, d, which); };
    auto blocks = [](int d) { return dim3(nblocks(recon_nodes(d), kT)); };
    auto n_of = [](int d) { return (1 << d) + 1; };
    float h2[r3g_rc::kMaxDepth + 1], inv_h2[r3g_rc::kMaxDepth + 1];
    for (int d = 1; d <= depth; ++d) r3g_rc::level_h2(depth, st->side, d, &h2[d], &inv_h2[d]);
    auto sweeps = [&](int d) {      // two sweeps: x -> buffer -> x
        hipLaunchKernelGGL(rc_smooth, blocks(d), dim3(kT), 0, s, buf(d, 0), buf(d, 2), buf(d, 1), n_of(d), h2[d]);
        hipLaunchKernelGGL(rc_smooth, blocks(d), dim3(kT), 0, s, buf(d, 1), buf(d, 2), buf(d, 0), n_of(d), h2[d]);
    };
    hipLaunchKernelGGL(rc_rhs, blocks(depth), dim3(kT), 0, s, (const int64_t*)st->channels.p, st->lat, buf(depth, 2));
    R3G_HIP(hipMemsetAsync(buf(depth, 0), 0, (size_t)recon_nodes(depth) * 4, s));
    for (int c = 0; c < cycles; ++c) {
        for (int d = depth; d >= 2; --d) {
            sweeps(d);
            hipLaunchKernelGGL(rc_restrict, blocks(d - 1), dim3(kT), 0, s, buf(d, 0), buf(d, 2), n_of(d), inv_h2[d], buf(d - 1, 2),
                               buf(d - 1, 0));
        }
        hipLaunchKernelGGL(rc_coarsest, dim3(1), dim3(64), 0, s, buf(1, 0), buf(1, 2), h2[1]);
        for (int d = 2; d <= depth; ++d) {
            hipLaunchKernelGGL(rc_prolong, blocks(d), dim3(kT), 0, s, buf(d, 0), buf(d - 1, 0), n_of(d));
            sweeps(d);
        }
        R3G_HIP(hipGetLastError());
    }
    return hipGetLastError();
}

hipError_t recon_sample(ReconState* st, int field, const float* points, const float* normals, int64_t n, float* values_out,
                        hipStream_t s) {
    const int depth = st->lat.depth;
    ReconSmall* sm = (ReconSmall*)(st->channels.p + recon_small_offset(depth));
    R3G_HIP(hipMemsetAsync(sm, 0, sizeof(ReconSmall), s));
    if (field == 0)
        hipLaunchKernelGGL((rc_sample<LoadFixed>), dim3(nblocks(n, kT)), dim3(kT), 0, s, LoadFixed{(const int64_t*)st->channels.p}, points,
                           normals, n, st->lat, values_out, sm);
    else
        hipLaunchKernelGGL((rc_sample<LoadFloat>), dim3(nblocks(n, kT)), dim3(kT), 0, s,
                           LoadFloat{(const float*)st->levels.p + recon_level_offset(depth, depth, 0)}, points, normals, n, st->lat,
                           values_out, sm);
    return hipGetLastError();
}

}  // namespace r3g
