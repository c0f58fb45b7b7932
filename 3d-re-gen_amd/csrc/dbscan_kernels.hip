// dbscan_kernels.hip -- DBSCAN on the point cloud of a context.
//
// One lane per usable point, taken in cell order (a wave's lanes sit in neighbouring cells and gather the same 16-byte
// records), walks the box of cells that can hold a neighbour (dbscan_core.h, radius_walk) three times: to count, to link
// core points by the lock-free union-find of uf_device.h (roots link to the smaller index, so a cluster's root is its
// smallest core index whatever the schedule), and to give every non-core point the smallest root among its core neighbours.
// Roots are numbered by the library's exclusive scan.  Integer atomics only, and their order decides nothing: the sets of a
// union-find do not depend on the order of the unions, the sizes are sums and the arg-max is a max.  The number of launches
// is fixed: no pass is repeated until it converges.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_GRID_HD static __host__ __device__ __forceinline__
#define R3G_MD_HD static __host__ __device__ __forceinline__
#define R3G_CL_HD static __host__ __device__ __forceinline__
#define R3G_CL_HD_MEMBER __host__ __device__ __forceinline__
#define R3G_DB_HD static __host__ __device__ __forceinline__
#define R3G_DB_HD_MEMBER __host__ __device__ __forceinline__
#include "dbscan_kernels.h"
#include "mesh_launch.h"
#include "scan_kernels.h"
#include "uf_device.h"

namespace r3g {
namespace {

using r3g_cl::Grid;
using r3g_cl::Pt;

__global__ __launch_bounds__(kT) void db_begin(int64_t n, int32_t* __restrict__ label, uint32_t* __restrict__ count,
                                               uint8_t* __restrict__ core, int32_t* __restrict__ root, uint32_t* __restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    label[i] = -1;
    if (count) count[i] = 0;
    core[i] = 0, root[i] = -1, size[i] = 0;
}

// FULL: the whole count (the caller wants it); otherwise a lane stops at min_samples
template <bool FULL>
__global__ __launch_bounds__(kT) void db_count(Grid g, const Pt* __restrict__ sorted, const unsigned* __restrict__ starts, int64_t m,
                                               double eps, double eps2, uint32_t min_samples, uint32_t* __restrict__ count,
                                               uint8_t* __restrict__ core, int32_t* __restrict__ root, DbscanSmall* __restrict__ sm) {
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long tests = 0, ncore = 0;
    if (k < m) {
        const Pt p = sorted[k];
        r3g_db::CountVisitor v{0u, FULL ? 0xffffffffu : min_samples};
        tests = r3g_db::radius_walk(g, sorted, starts, p, eps, eps2, v);
        const bool is_core = v.count >= min_samples;
        if (FULL) count[p.index] = v.count;
        if (is_core) core[p.index] = 1, root[p.index] = p.index, ncore = 1;
    }
    tests = wave_sum_u64(tests), ncore = wave_sum_u64(ncore);
    if ((threadIdx.x & 63) == 0 && (tests | ncore)) atomicAdd(&sm->tests, tests), atomicAdd(&sm->n_core, ncore);
}

struct DeviceUnite {
    int* parent;
    __device__ __forceinline__ void operator()(int32_t a, int32_t b) { uf_union(parent, a, b); }
};

__global__ __launch_bounds__(kT) void db_link(Grid g, const Pt* __restrict__ sorted, const unsigned* __restrict__ starts, int64_t m,
                                              double eps, double eps2, const uint8_t* __restrict__ core, int32_t* root,
                                              DbscanSmall* __restrict__ sm) {
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long tests = 0;
    if (k < m) {
        const Pt p = sorted[k];
        if (core[p.index]) {
            DeviceUnite u{root};
            r3g_db::LinkVisitor<DeviceUnite> v{core, p.index, u};
            tests = r3g_db::radius_walk(g, sorted, starts, p, eps, eps2, v);
        }
    }
    tests = wave_sum_u64(tests);
    if ((threadIdx.x & 63) == 0 && tests) atomicAdd(&sm->tests, tests);
}

// roots never change here (nothing links any more), so every chain ends in its final root
__global__ __launch_bounds__(kT) void db_flatten(int64_t n, int32_t* root) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    if (__hip_atomic_load(&root[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
    const int r = uf_find(root, (int)i);
    __hip_atomic_store(&root[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// reads root[] of core points only and writes root[] of non-core points only: no lane reads what another writes
__global__ __launch_bounds__(kT) void db_border(Grid g, const Pt* __restrict__ sorted, const unsigned* __restrict__ starts, int64_t m,
                                                double eps, double eps2, const uint8_t* __restrict__ core, int32_t* root,
                                                DbscanSmall* __restrict__ sm) {
    const int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long tests = 0, nborder = 0;
    if (k < m) {
        const Pt p = sorted[k];
        if (!core[p.index]) {
            r3g_db::BorderVisitor v{core, root, r3g_cl::kNoIndex};
            tests = r3g_db::radius_walk(g, sorted, starts, p, eps, eps2, v);
            if (v.best != r3g_cl::kNoIndex) root[p.index] = v.best, nborder = 1;
        }
    }
    tests = wave_sum_u64(tests), nborder = wave_sum_u64(nborder);
    if ((threadIdx.x & 63) == 0 && (tests | nborder)) atomicAdd(&sm->tests, tests), atomicAdd(&sm->n_border, nborder);
}

__global__ __launch_bounds__(kT) void db_flag(int64_t n, const int32_t* __restrict__ root, uint32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i < n) flag[i] = r3g_db::root_flag(root, i);
}

// Labels and points per cluster.  One dominant cluster is the expected case, and same-address atomics serialise in L2:
// lanes with equal labels are merged first (one atomic per distinct label per wave).
__global__ __launch_bounds__(kT) void db_label(int64_t n, const int32_t* __restrict__ root, const uint32_t* __restrict__ number,
                                               int32_t* __restrict__ label, uint32_t* __restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t l = i < n ? r3g_db::label_of(root, number, i) : -1;
    if (i < n) label[i] = l;
    unsigned long long todo = __ballot(l >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t ll = __shfl(l, leader, 64);
        const unsigned long long same = __ballot(l == ll) & todo;
        if (lane == leader) atomicAdd(&size[ll], (unsigned)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(kT) void db_largest(int64_t n, const uint32_t* __restrict__ size, DbscanSmall* __restrict__ sm) {
    const int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x;
    unsigned long long best = (c < n && c < (int64_t)sm->n_clusters) ? r3g_db::pack_best(size[c], (int32_t)c) : 0ull;
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(&sm->best, best);
}

template <class T>
T* at(char* ws, size_t off) {
    return (T*)(ws + off);
}

}  // namespace

size_t dbscan_workspace_bytes(int64_t n, DbscanLayout* lay) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t m = (size_t)(n < 1 ? 1 : n);
    lay->off_small = take(sizeof(DbscanSmall));
    lay->off_core = take(m), lay->off_root = take(4 * m), lay->off_number = take(4 * m), lay->off_size = take(4 * m);
    lay->off_sums = take(4 * scan_scratch_elems((int64_t)m));
    return lay->bytes = off;
}

hipError_t dbscan_begin(char* ws, const DbscanLayout& lay, int64_t n, int32_t* label, uint32_t* count, hipStream_t s) {
    R3G_HIP(hipMemsetAsync(ws + lay.off_small, 0, sizeof(DbscanSmall), s));
    hipLaunchKernelGGL(db_begin, dim3(nblocks(n, kT)), dim3(kT), 0, s, n, label, count, at<uint8_t>(ws, lay.off_core),
                       at<int32_t>(ws, lay.off_root), at<uint32_t>(ws, lay.off_size));
    return hipGetLastError();
}

hipError_t dbscan_run(char* ws, const DbscanLayout& lay, const Grid& g, const Pt* sorted, const unsigned* starts, int64_t m, int64_t n,
                      double eps, uint32_t min_samples, int32_t* label, uint32_t* count, const Event* ev, int* launches, hipStream_t s) {
    const dim3 gm(nblocks(m, kT)), gn(nblocks(n, kT)), b(kT);
    const double eps2 = eps * eps;
    uint8_t* core = at<uint8_t>(ws, lay.off_core);
    int32_t* root = at<int32_t>(ws, lay.off_root);
    uint32_t* number = at<uint32_t>(ws, lay.off_number);
    uint32_t* size = at<uint32_t>(ws, lay.off_size);
    DbscanSmall* sm = at<DbscanSmall>(ws, lay.off_small);
    int pass = 0;
    auto mark = [&] { return hipEventRecord(ev[pass++], s); };
    R3G_HIP(mark());
    if (count)
        hipLaunchKernelGGL((db_count<true>), gm, b, 0, s, g, sorted, starts, m, eps, eps2, min_samples, count, core, root, sm);
    else
        hipLaunchKernelGGL((db_count<false>), gm, b, 0, s, g, sorted, starts, m, eps, eps2, min_samples, count, core, root, sm);
    R3G_HIP(mark());
    hipLaunchKernelGGL(db_link, gm, b, 0, s, g, sorted, starts, m, eps, eps2, (const uint8_t*)core, root, sm);
    hipLaunchKernelGGL(db_flatten, gn, b, 0, s, n, root);
    R3G_HIP(mark());
    hipLaunchKernelGGL(db_border, gm, b, 0, s, g, sorted, starts, m, eps, eps2, (const uint8_t*)core, root, sm);
    R3G_HIP(mark());
    hipLaunchKernelGGL(db_flag, gn, b, 0, s, n, (const int32_t*)root, number);
    R3G_HIP(exclusive_scan_u32(number, number, n, at<unsigned>(ws, lay.off_sums), &sm->n_clusters, s));
    hipLaunchKernelGGL(db_label, gn, b, 0, s, n, (const int32_t*)root, (const uint32_t*)number, label, size);
    hipLaunchKernelGGL(db_largest, gn, b, 0, s, n, (const uint32_t*)size, sm);
    R3G_HIP(mark());
    *launches = 10;     // count, link, flatten, border, flag, the scan's three, label, largest
    return hipGetLastError();
}

}  // namespace r3g
