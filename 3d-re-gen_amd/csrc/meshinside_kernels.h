// meshinside_kernels.h -- host-side interface of meshinside_kernels.hip (internal to libr3g.so)
#ifndef R3G_MESHINSIDE_KERNELS_H
#define R3G_MESHINSIDE_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "meshinside_core.h"

namespace r3g {

// what the build leaves on the device for the query (all inside Ctx::meshinside_ws except the pair list)
struct MeshinsideLayout {
    size_t off_small;     // MeshinsideSmall
    size_t off_recs;      // r3g_mi::Rec [nf]
    size_t off_counts;    // uint32 [columns + 1]: per-column counts, then the fill cursors
    size_t off_starts;    // uint32 [columns + 1]: CSR row starts
    size_t off_sums;      // uint32 [scan tiles]
    size_t total;
};

// the 48 bytes read back through the context's pinned buffer
struct MeshinsideSmall {
    uint32_t bad_index;             // != 0: a face index outside [0, V)
    uint32_t pad;
    unsigned long long skipped;     // faces with a non-finite vertex
    uint32_t box[4];                // enc_float of lo[2], hi[2] of the projected vertices of the finite faces
    unsigned long long pairs;       // (face, column) pairs at the resolution last counted
    unsigned long long tests;       // point-face tests of the last query
};

size_t meshinside_workspace_bytes(int64_t nf, int res_max, MeshinsideLayout* lay);

// validate the indices, project the faces into padded records (unusable ones marked), projected bounding box and
// `skipped` into MeshinsideSmall
hipError_t meshinside_records(char* ws, const MeshinsideLayout& lay, const float* verts, int64_t nv, const int32_t* faces,
                              int64_t nf, int axis, hipStream_t s);
// MeshinsideSmall::pairs for grid g (touches no column)
hipError_t meshinside_count_pairs(char* ws, const MeshinsideLayout& lay, int64_t nf, const r3g_mi::Grid2& g, hipStream_t s);
// per-column counts -> exclusive scan -> fill of pairs [MeshinsideSmall::pairs] with face ids
hipError_t meshinside_fill(char* ws, const MeshinsideLayout& lay, int64_t nf, const r3g_mi::Grid2& g, int32_t* pairs, hipStream_t s);
hipError_t meshinside_query(char* ws, const MeshinsideLayout& lay, const r3g_mi::Grid2& g, int axis, const int32_t* pairs,
                            const float* points, int64_t n, int32_t* count, hipStream_t s);

void meshinside_add_tests(int64_t n);     // r3g_get_counter("meshinside_tests")
int64_t meshinside_tests_total();

}  // namespace r3g
#endif
