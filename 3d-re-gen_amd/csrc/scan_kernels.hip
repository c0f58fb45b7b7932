// scan_kernels.hip -- scan_device.h instantiated for a plain array: the scan behind the mesh cleaners' compactions, the CSR
// row starts of the grid build (meshdist, meshinside, cloud) and the tile offsets of meshfill.  Integers only.
#include "scan_kernels.h"

namespace r3g {

hipError_t exclusive_scan_u32(const unsigned* in, unsigned* out, int64_t n, unsigned* tile_sums, unsigned* d_total, hipStream_t s) {
    return exclusive_scan(ScanLoadU32{in}, n, out, tile_sums, d_total, s);
}

}  // namespace r3g
