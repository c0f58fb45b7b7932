// recon_kernels.h -- host-side interface of recon_kernels.hip (internal to libr3g.so)
#ifndef R3G_RECON_KERNELS_H
#define R3G_RECON_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dev_buf.h"
#include "recon_core.h"

namespace r3g {

// what a context keeps of the last r3g_recon_splat: the four int64 channels [4][n^3] followed by ReconSmall, and the float32
// lattices of the solver (per level d = 1 .. depth: x, the second sweep buffer, b).  Both buffers grow only.
struct ReconSmall {
    unsigned long long usable;      // splat: usable points.  sample: points that took part in the sum
    unsigned long long sum;         // sample: the int64 fixed-point sum of the sampled values (two's complement)
};

struct ReconState {
    DevBuf channels, levels;
    r3g_rc::Lattice lat{};
    double side = 0.0;
    bool splatted = false, solved = false;
};

inline int64_t recon_nodes(int d) { return (int64_t)((1 << d) + 1) * ((1 << d) + 1) * ((1 << d) + 1); }
inline size_t recon_channels_bytes(int depth) { return (size_t)recon_nodes(depth) * 8 * r3g_rc::kChannels + sizeof(ReconSmall); }
inline size_t recon_small_offset(int depth) { return (size_t)recon_nodes(depth) * 8 * r3g_rc::kChannels; }
// float offset of buffer `which` (0 x, 1 sweep buffer, 2 b) of level d in `levels` (the finest level first)
inline size_t recon_level_offset(int depth, int d, int which) {
    size_t off = 0;
    for (int e = depth; e > d; --e) off += 3 * (size_t)recon_nodes(e);
    return off + (size_t)which * (size_t)recon_nodes(d);
}
inline size_t recon_levels_bytes(int depth) { return 4 * recon_level_offset(depth, 0, 0); }     // levels depth .. 1

// zero the channels and ReconSmall, then add every usable point's 8 trilinear weights (density) and weighted unit normal
hipError_t recon_splat(ReconState* st, const float* points, const float* normals, int64_t n, hipStream_t s);
// b = div V on the finest level, x = 0, then `cycles` V-cycles; the result is buffer x of level depth
hipError_t recon_solve(ReconState* st, int cycles, hipStream_t s);
// trilinear sample of the density channel (field 0) or of x (field 1) at points [n][3]: values_out float32 [n] (may be null;
// NaN for a point that takes no part) and, into ReconSmall, the fixed-point sum and the count over the points that take
// part: finite coordinates and, where normals is non-null, a usable normal
hipError_t recon_sample(ReconState* st, int field, const float* points, const float* normals, int64_t n, float* values_out,
                        hipStream_t s);

}  // namespace r3g
#endif
