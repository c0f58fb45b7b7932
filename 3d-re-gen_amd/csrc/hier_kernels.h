// hier_kernels.h -- planner of the hierarchical volume decoder (hier_kernels.hip): which points of the next finer lattice
// have to be evaluated, as a bit mask over their linear indices, its ascending index list, and the merge of the evaluated
// values with the floor parents of the coarse grid.  The algorithm is defined in DESIGN.md ("Hierarchical volume decoding").
#ifndef R3G_HIER_KERNELS_H
#define R3G_HIER_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace r3g {

// One select's state inside a caller-owned workspace.  nc = points per axis of the coarse grid, nf = 2 nc - 1 of the fine one.
struct HierLayout {
    int nc = 0, nf = 0;
    int64_t coarse_pts = 0, fine_pts = 0, nwords = 0;   // nwords = ceil(fine_pts / 64): bit q & 63 of word q >> 6 is point q
    int nblocks = 0;                                     // tiles of the popcount scan (scan_device.h: 2048 words each)
    size_t off_cand = 0, off_dil = 0, off_words = 0, off_prefix = 0, off_bsum = 0, off_small = 0, total = 0;
};

size_t hier_workspace_bytes(int nc, HierLayout* lay);

// steps 1-5 and the scan: leaves the mask, the exclusive popcount prefix per word and, at ws + off_small, the number of
// active points (uint64).  All counts are integers; the result does not depend on the launch shape.
hipError_t hier_select_launch(const float* coarse, double level, double band, int is_finest, char* ws, const HierLayout& lay,
                              hipStream_t s);
// ascending linear indices of the mask's points (step 6): idx has room for the count hier_select_launch left
hipError_t hier_indices_launch(const char* ws, const HierLayout& lay, int32_t* idx, hipStream_t s);
// step 8: fine[q] = values[rank(q)] for a point of the mask, coarse[q >> 1 per axis] for every other one
hipError_t hier_merge_launch(const char* ws, const HierLayout& lay, const float* coarse, const float* values, float* fine,
                             hipStream_t s);
// number of cells of `fine` whose corners are not all on one side of `level` and not all in the mask: uint64 at ws + off_small + 8
hipError_t hier_unsafe_launch(char* ws, const HierLayout& lay, const float* fine, double level, hipStream_t s);

}  // namespace r3g
#endif
