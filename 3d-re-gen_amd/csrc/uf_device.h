// uf_device.h -- the lock-free union-find that the floater cleaner (mesh_kernels.hip) and DBSCAN (dbscan_kernels.hip) share.
// Roots always link to the smaller id, so a set's root is its smallest member, independent of scheduling.  Included by
// those .hip files only; the anonymous namespace gives each its own copy.
#ifndef R3G_UF_DEVICE_H
#define R3G_UF_DEVICE_H
#include <hip/hip_runtime.h>

namespace r3g {
namespace {

__device__ __forceinline__ int uf_find(const int* __restrict__ parent, int x) {
    int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

// find with path halving: a non-root slot is re-pointed at its grandparent (still an ancestor with a smaller id, so
// concurrent finds and links stay correct; a root's slot is only ever changed by the CAS in uf_union)
__device__ __forceinline__ int uf_find_halving(int* __restrict__ parent, int x) {
    int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        const int gp = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gp != p) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void uf_union(int* __restrict__ parent, int a, int b) {
    for (;;) {
        a = uf_find_halving(parent, a);
        b = uf_find_halving(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        // the larger root goes under the smaller one; only a root's own slot is ever CASed
        if (atomicCAS(&parent[hi], hi, lo) == hi) return;
    }
}

}  // namespace
}  // namespace r3g
#endif
