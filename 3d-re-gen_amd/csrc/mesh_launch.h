// mesh_launch.h -- what the mesh .hip files (mesh, meshdist, meshinside, meshfit, meshtopo, meshfill) share around a launch:
// the block size, grid sizes, the integer wave sum and the early return on a HIP error.  Internal to each translation unit.
// The prefix sums they share live in scan_device.h.
#ifndef R3G_MESH_LAUNCH_H
#define R3G_MESH_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace r3g {
namespace {

constexpr int kT = 256;

inline unsigned nblocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
// blocks of a grid-stride loop over n elements
inline unsigned grid_for(int64_t n) {
    const unsigned b = nblocks(n, kT);
    return b < 1 ? 1 : (b > 4096 ? 4096 : b);
}

// an integer sum: the order of the butterfly decides nothing
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace
}  // namespace r3g

#define R3G_HIP(x)                         \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

#endif
