// orient_kernels.h -- host-side interface of orient_kernels.hip (internal to libr3g.so)
#ifndef R3G_ORIENT_KERNELS_H
#define R3G_ORIENT_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "orient_core.h"

namespace r3g {

struct OrientSmall {
    unsigned long long usable, merged, trees, flipped, frustrated;
};

// the workspace of one r3g_cloud_orient over n points with rows of k + 1 entries (byte offsets, each a multiple of 16)
struct OrientLayout {
    size_t off_q, off_unit, off_d2, off_idx, off_comp[2], off_par[2], off_best_w, off_best_pair, off_tree_min, off_top, off_small, bytes;
};
size_t orient_workspace_bytes(int64_t n, int k, OrientLayout* lay);

// q = the usable points (others NaN), unit normals, comp[0] = i / -1, par[0] = 0; OrientSmall zeroed, usable counted
hipError_t orient_prepare(char* ws, const OrientLayout& lay, const float* points, const float* normals, int64_t n, hipStream_t s);
// one Boruvka round over the rows in ws (k + 1 entries each): cheapest leaving edge per component, hooks, pointer jumping with
// parity; comp[0] / par[0] hold roots and parities to them afterwards, OrientSmall.merged the number of roots that hooked
hipError_t orient_round(char* ws, const OrientLayout& lay, int64_t n, int k, hipStream_t s);
// sign int8 [n], tree int32 [n] and the counts of OrientSmall from the finished forest
hipError_t orient_finish(char* ws, const OrientLayout& lay, const float* normals, int64_t n, int k, int8_t* sign, int32_t* tree,
                         hipStream_t s);

}  // namespace r3g
#endif
