// orient_kernels.hip -- consistent orientation of point normals over the k-nearest-neighbour graph (part A):
// the minimum spanning forest under (1 - |u_i . u_j|, min, max) by Boruvka rounds, with every node's parity to its root.
//
// A round: every lane scans its own row and offers each edge that leaves its component to BOTH components (the rows are
// directed, the graph is not), first the weight's bits, then the (min, max) pair among the edges that attain it, by integer
// atomicMin; every root hooks along its edge (a mutual pair keeps the lower root); pointer jumping, buffer to buffer, flattens
// the trees and carries the parities.  Integer atomics only: the forest is unique, so their order decides nothing.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_RC_HD static __host__ __device__ __forceinline__
#define R3G_OR_HD static __host__ __device__ __forceinline__
#include "mesh_launch.h"
#include "orient_kernels.h"

namespace r3g {
namespace {

__global__ __launch_bounds__(kT) void or_prepare(const float* __restrict__ points, const float* __restrict__ normals, int64_t n,
                                                 float* __restrict__ q, float* __restrict__ unit, int32_t* __restrict__ comp,
                                                 uint8_t* __restrict__ par, OrientSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long used = 0;
    if (i < n) {
        const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        const float nr[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
        float u[3] = {0.0f, 0.0f, 0.0f};
        const bool ok = r3g_rc::usable(p, nr);
        if (ok) r3g_rc::unit_normal(nr, u), used = 1;
        const float nan = __builtin_nanf("");
        for (int a = 0; a < 3; ++a) q[3 * i + a] = ok ? p[a] : nan, unit[3 * i + a] = u[a];
        comp[i] = ok ? (int32_t)i : -1;
        par[i] = 0;
    }
    used = wave_sum_u64(used);
    if ((threadIdx.x & 63) == 0 && used) atomicAdd(&sm->usable, used);
}

__global__ __launch_bounds__(kT) void or_reset(int64_t n, uint32_t* __restrict__ best_w, unsigned long long* __restrict__ best_pair) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i < n) best_w[i] = r3g_or::kNoWeight, best_pair[i] = r3g_or::kNoPair;
}

// PAIRS false: the weight's bits.  true: the (min, max) pair among the edges that attain a component's weight
template <bool PAIRS>
__global__ __launch_bounds__(kT) void or_offer(const int32_t* __restrict__ idx, int k, int64_t n, const int32_t* __restrict__ comp,
                                               const float* __restrict__ unit, uint32_t* __restrict__ best_w,
                                               unsigned long long* __restrict__ best_pair) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int32_t ci = comp[i];
    if (ci < 0) return;
    r3g_or::each_neighbour(idx + i * (k + 1), k, (int32_t)i, [&](int32_t j) {
        const int32_t cj = comp[j];
        if (cj == ci) return;
        const uint32_t w = r3g_or::weight_bits(r3g_or::dot3(unit + 3 * i, unit + 3 * (int64_t)j));
        if (!PAIRS) {
            atomicMin(best_w + ci, w);
            atomicMin(best_w + cj, w);
        } else {
            const unsigned long long p = r3g_or::pack_pair((int32_t)i, j);
            if (best_w[ci] == w) atomicMin(best_pair + ci, p);
            if (best_w[cj] == w) atomicMin(best_pair + cj, p);
        }
    });
}

// hook the roots and copy the rest: (comp, par) -> (comp_out, par_out)
__global__ __launch_bounds__(kT) void or_hook(int64_t n, const int32_t* __restrict__ comp, const uint8_t* __restrict__ par,
                                              const unsigned long long* __restrict__ best_pair, const float* __restrict__ unit,
                                              int32_t* __restrict__ comp_out, uint8_t* __restrict__ par_out, OrientSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long merged = 0;
    if (i < n) {
        int32_t c = comp[i];
        uint8_t p = par[i];
        if (c == (int32_t)i) {
            int32_t to;
            uint8_t pt;
            if (r3g_or::hook((int32_t)i, best_pair[i], comp, par, (const uint64_t*)best_pair, unit, &to, &pt)) c = to, p = pt, merged = 1;
        }
        comp_out[i] = c;
        par_out[i] = p;
    }
    merged = wave_sum_u64(merged);
    if ((threadIdx.x & 63) == 0 && merged) atomicAdd(&sm->merged, merged);
}

// one doubling step, buffer to buffer: the parent's parent, and the parity to it
__global__ __launch_bounds__(kT) void or_jump(int64_t n, const int32_t* __restrict__ comp, const uint8_t* __restrict__ par,
                                              int32_t* __restrict__ comp_out, uint8_t* __restrict__ par_out) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int32_t c = comp[i];
    comp_out[i] = c < 0 ? -1 : comp[c];
    par_out[i] = c < 0 ? (uint8_t)0 : (uint8_t)(par[i] ^ par[c]);
}

__global__ __launch_bounds__(kT) void or_tree_reset(int64_t n, int32_t* __restrict__ tree_min, unsigned long long* __restrict__ top) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i < n) tree_min[i] = 0x7fffffff, top[i] = 0;
}

__global__ __launch_bounds__(kT) void or_tree_reduce(int64_t n, const int32_t* __restrict__ comp, const float* __restrict__ q,
                                                     int32_t* __restrict__ tree_min, unsigned long long* __restrict__ top) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const int32_t c = comp[i];
    if (c < 0) return;
    atomicMin(tree_min + c, (int32_t)i);
    atomicMax(top + c, (unsigned long long)r3g_or::top_key(q[3 * i + 2], (int32_t)i));
}

__global__ __launch_bounds__(kT) void or_sign(int64_t n, const int32_t* __restrict__ comp, const uint8_t* __restrict__ par,
                                              const int32_t* __restrict__ tree_min, const unsigned long long* __restrict__ top,
                                              const float* __restrict__ normals, int8_t* __restrict__ sign, int32_t* __restrict__ tree,
                                              OrientSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long trees = 0, flipped = 0;
    if (i < n) {
        const int32_t c = comp[i];
        if (c < 0) {
            sign[i] = 0, tree[i] = -1;
        } else {
            const int32_t t = r3g_or::top_index(top[c]);
            const int bit = (normals[3 * (int64_t)t + 2] < 0.0f ? 1 : 0) ^ par[t] ^ par[i];     // the top member ends with s n_z >= 0
            sign[i] = bit ? -1 : 1;
            tree[i] = tree_min[c];
            flipped = (unsigned long long)bit;
            trees = c == (int32_t)i;
        }
    }
    trees = wave_sum_u64(trees), flipped = wave_sum_u64(flipped);
    if ((threadIdx.x & 63) == 0 && (trees | flipped)) atomicAdd(&sm->trees, trees), atomicAdd(&sm->flipped, flipped);
}

// every undirected graph edge once: from the lower end, or from the end whose row alone holds it
__global__ __launch_bounds__(kT) void or_frustrated(const int32_t* __restrict__ idx, int k, int64_t n, const int8_t* __restrict__ sign,
                                                    const float* __restrict__ unit, OrientSmall* __restrict__ sm) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long bad = 0;
    if (i < n && sign[i] != 0) {
        r3g_or::each_neighbour(idx + i * (k + 1), k, (int32_t)i, [&](int32_t j) {
            if (!r3g_or::frustrated(sign, unit, (int32_t)i, j)) return;
            if ((int32_t)i < j || !r3g_or::has_neighbour(idx + (int64_t)j * (k + 1), k, j, (int32_t)i)) ++bad;
        });
    }
    bad = wave_sum_u64(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&sm->frustrated, bad);
}

template <class T>
T* at(char* ws, size_t off) {
    return (T*)(ws + off);
}

}  // namespace

size_t orient_workspace_bytes(int64_t n, int k, OrientLayout* lay) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 15) & ~(size_t)15;
        return o;
    };
    const size_t m = (size_t)n;
    lay->off_q = take(12 * m), lay->off_unit = take(12 * m);
    lay->off_d2 = take(4 * m * (k + 1)), lay->off_idx = take(4 * m * (k + 1));
    for (int b = 0; b < 2; ++b) lay->off_comp[b] = take(4 * m), lay->off_par[b] = take(m);
    lay->off_best_w = take(4 * m), lay->off_best_pair = take(8 * m);
    lay->off_tree_min = take(4 * m), lay->off_top = take(8 * m);
    lay->off_small = take(sizeof(OrientSmall));
    return lay->bytes = off;
}

hipError_t orient_prepare(char* ws, const OrientLayout& lay, const float* points, const float* normals, int64_t n, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small, 0, sizeof(OrientSmall), s));
    hipLaunchKernelGGL(or_prepare, dim3(nblocks(n, kT)), dim3(kT), 0, s, points, normals, n, at<float>(ws, lay.off_q),
                       at<float>(ws, lay.off_unit), at<int32_t>(ws, lay.off_comp[0]), at<uint8_t>(ws, lay.off_par[0]),
                       at<OrientSmall>(ws, lay.off_small));
    return hipGetLastError();
}

hipError_t orient_round(char* ws, const OrientLayout& lay, int64_t n, int k, hipStream_t s) {
    const dim3 g(nblocks(n, kT)), b(kT);
    const int32_t* idx = at<int32_t>(ws, lay.off_idx);
    const float* unit = at<float>(ws, lay.off_unit);
    int32_t* comp[2] = {at<int32_t>(ws, lay.off_comp[0]), at<int32_t>(ws, lay.off_comp[1])};
    uint8_t* par[2] = {at<uint8_t>(ws, lay.off_par[0]), at<uint8_t>(ws, lay.off_par[1])};
    uint32_t* best_w = at<uint32_t>(ws, lay.off_best_w);
    unsigned long long* best_pair = at<unsigned long long>(ws, lay.off_best_pair);
    OrientSmall* sm = at<OrientSmall>(ws, lay.off_small);
    R3G_HIP(hipMemsetAsync(&sm->merged, 0, 8, s));
    hipLaunchKernelGGL(or_reset, g, b, 0, s, n, best_w, best_pair);
    hipLaunchKernelGGL((or_offer<false>), g, b, 0, s, idx, k, n, comp[0], unit, best_w, best_pair);
    hipLaunchKernelGGL((or_offer<true>), g, b, 0, s, idx, k, n, comp[0], unit, best_w, best_pair);
    hipLaunchKernelGGL(or_hook, g, b, 0, s, n, comp[0], par[0], best_pair, unit, comp[1], par[1], sm);
    // after the hooks a chain is at most n long: 2^steps >= n doubling steps reach every root; an odd number of them ends in
    // buffer 0, and a step past the end changes nothing
    int steps = 1;
    while (((int64_t)1 << steps) < n) ++steps;
    steps |= 1;
    for (int t = 0, from = 1; t < steps; ++t, from ^= 1)
        hipLaunchKernelGGL(or_jump, g, b, 0, s, n, comp[from], par[from], comp[from ^ 1], par[from ^ 1]);
    return hipGetLastError();
}

hipError_t orient_finish(char* ws, const OrientLayout& lay, const float* normals, int64_t n, int k, int8_t* sign, int32_t* tree,
                         hipStream_t s) {
    const dim3 g(nblocks(n, kT)), b(kT);
    const int32_t* comp = at<int32_t>(ws, lay.off_comp[0]);
    const uint8_t* par = at<uint8_t>(ws, lay.off_par[0]);
    int32_t* tree_min = at<int32_t>(ws, lay.off_tree_min);
    unsigned long long* top = at<unsigned long long>(ws, lay.off_top);
    OrientSmall* sm = at<OrientSmall>(ws, lay.off_small);
    hipLaunchKernelGGL(or_tree_reset, g, b, 0, s, n, tree_min, top);
    hipLaunchKernelGGL(or_tree_reduce, g, b, 0, s, n, comp, at<float>(ws, lay.off_q), tree_min, top);
    hipLaunchKernelGGL(or_sign, g, b, 0, s, n, comp, par, tree_min, top, normals, sign, tree, sm);
    hipLaunchKernelGGL(or_frustrated, g, b, 0, s, at<int32_t>(ws, lay.off_idx), k, n, sign, at<float>(ws, lay.off_unit), sm);
    return hipGetLastError();
}

}  // namespace r3g
