// scan_kernels.h -- the device-wide exclusive scan of scan_device.h over a plain uint32 array, exported once for the library
// (internal to libr3g.so).  For the .hip files only: it brings scan_device.h's tile constant and scratch length with it.
#ifndef R3G_SCAN_KERNELS_H
#define R3G_SCAN_KERNELS_H
#include "scan_device.h"

namespace r3g {

// out[i] = in[0] + ... + in[i - 1] (modulo 2^32) for i in [0, n); *d_total = the sum of all, where d_total is not null.
// tile_sums: scan_scratch_elems(n) words of scratch.  in == out is allowed.  Three launches, no capacity.
hipError_t exclusive_scan_u32(const unsigned* in, unsigned* out, int64_t n, unsigned* tile_sums, unsigned* d_total, hipStream_t s);

}  // namespace r3g
#endif
