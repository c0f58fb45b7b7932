// grid_csr_kernels.hip -- the part of the grid build (grid_csr.h) that does not depend on the record type: the workspace
// layout.  The exclusive scan that turns per-cell counts into CSR row starts is exclusive_scan_u32 (scan_kernels.h).
#include "grid_csr_kernels.h"
#include "scan_kernels.h"

namespace r3g {

size_t grid_csr_workspace_bytes(int64_t nf, size_t record_bytes, int64_t cells, GridCsrLayout* lay) {
    const size_t cells1 = (size_t)cells + 1;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 0;
    lay->off_small = o, o += 256;
    lay->off_recs = o, o += up(record_bytes * (size_t)nf);
    lay->off_counts = o, o += up(4 * cells1);
    lay->off_starts = o, o += up(4 * cells1);
    lay->off_sums = o, o += up(4 * scan_scratch_elems((int64_t)cells1));
    lay->total = o;
    return o;
}

}  // namespace r3g
