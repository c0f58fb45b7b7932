// grid_csr_kernels.h -- host-side interface of the device build of a grid in CSR form (grid_csr.h; internal to libr3g.so):
// what a build leaves behind, and its workspace layout (grid_csr_kernels.hip).  The kernels that depend on the record type
// are templates (grid_csr_device.h), instantiated by meshdist_kernels.hip, meshinside_kernels.hip and cloud_kernels.hip; the
// scan of the per-cell counts is the library's exclusive_scan_u32 (scan_kernels.h).
#ifndef R3G_GRID_CSR_KERNELS_H
#define R3G_GRID_CSR_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dev_buf.h"
#include "grid_csr.h"

namespace r3g {

// what the build leaves on the device for the query (all inside the user's workspace except the pair list)
struct GridCsrLayout {
    size_t off_small;     // GridCsrSmall
    size_t off_recs;      // the user's 48-byte record [nf]
    size_t off_counts;    // uint32 [cells + 1]: per-cell counts, then the fill cursors
    size_t off_starts;    // uint32 [cells + 1]: CSR row starts
    size_t off_sums;      // uint32 [scan_scratch_elems(cells + 1)]: the scan's tile sums
    size_t total;
};

// the bytes read back through the context's 64-byte pinned buffer
struct GridCsrSmall {
    uint32_t bad_index;             // != 0: a face index outside [0, V)
    uint32_t pad;
    unsigned long long skipped;     // faces with a non-finite vertex
    uint32_t box[6];                // enc_float of lo[D], hi[D] on the grid axes; the first 2 * D entries in use
    unsigned long long pairs;       // (record, cell) pairs at the resolution last counted
    unsigned long long tests;       // point-record tests of the last query
};
static_assert(sizeof(GridCsrSmall) == 56, "GridCsrSmall travels through the 64-byte pinned buffer");

// what a user keeps in the context between its build and its queries
template <int D>
struct GridCsrState {
    DevBuf ws;
    DevBuf pairs;                   // int32 [GridCsrSmall::pairs]: a buffer of its own
    GridCsrLayout lay{};
    r3g_grid::GridN<D> grid{};
    bool built = false;
};

size_t grid_csr_workspace_bytes(int64_t nf, size_t record_bytes, int64_t cells, GridCsrLayout* lay);

}  // namespace r3g
#endif
