// dbscan_kernels.h -- host-side interface of dbscan_kernels.hip (internal to libr3g.so)
#ifndef R3G_DBSCAN_KERNELS_H
#define R3G_DBSCAN_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dbscan_core.h"
#include "events.h"

namespace r3g {

struct DbscanLayout {
    size_t off_small;     // DbscanSmall
    size_t off_core;      // uint8 [n]
    size_t off_root;      // int32 [n]: the union-find's parents, then every point's root (-1: none)
    size_t off_number;    // uint32 [n]: root flags, scanned in place into cluster numbers
    size_t off_size;      // uint32 [n]: points per cluster (there are at most n clusters)
    size_t off_sums;      // uint32 [scan_scratch_elems(n)]
    size_t bytes;
};

// the bytes read back through the context's 64-byte pinned buffer
struct DbscanSmall {
    unsigned long long tests;       // predicate evaluations of the three walks
    unsigned long long n_core;
    unsigned long long n_border;
    unsigned long long best;        // r3g_db::pack_best of the largest cluster
    uint32_t n_clusters;
    uint32_t pad;
};
static_assert(sizeof(DbscanSmall) <= 64, "DbscanSmall travels through the 64-byte pinned buffer");

constexpr int kDbscanPasses = 4;    // count, link (with flatten), border, numbering (with sizes and the arg-max)

size_t dbscan_workspace_bytes(int64_t n, DbscanLayout* lay);
// label[i] = -1, count[i] = 0 (where given), no core, no root; DbscanSmall cleared.  One launch.
hipError_t dbscan_begin(char* ws, const DbscanLayout& lay, int64_t n, int32_t* label, uint32_t* count, hipStream_t s);
// The four passes over the m usable points `sorted` (cell order, grid g, CSR starts).  ev: kDbscanPasses + 1 events recorded
// around the passes.  -> the number of kernels launched through *launches.
hipError_t dbscan_run(char* ws, const DbscanLayout& lay, const r3g_cl::Grid& g, const r3g_cl::Pt* sorted, const unsigned* starts,
                      int64_t m, int64_t n, double eps, uint32_t min_samples, int32_t* label, uint32_t* count, const Event* ev,
                      int* launches, hipStream_t s);

}  // namespace r3g
#endif
