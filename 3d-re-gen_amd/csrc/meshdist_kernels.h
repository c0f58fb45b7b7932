// meshdist_kernels.h -- host-side interface of meshdist_kernels.hip (internal to libr3g.so)
#ifndef R3G_MESHDIST_KERNELS_H
#define R3G_MESHDIST_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "meshdist_core.h"

namespace r3g {

// what the build leaves on the device for the query (all inside Ctx::meshdist_ws except the pair list)
struct MeshdistLayout {
    size_t off_small;     // MeshdistSmall
    size_t off_tris;      // r3g_md::Tri [nf]
    size_t off_counts;    // uint32 [cells + 1]: per-cell counts, then the fill cursors
    size_t off_starts;    // uint32 [cells + 1]: CSR row starts
    size_t off_sums;      // uint32 [scan tiles]
    size_t total;
};

// the 64 bytes read back through the context's pinned buffer
struct MeshdistSmall {
    uint32_t bad_index;             // != 0: a face index outside [0, V)
    uint32_t pad;
    unsigned long long skipped;     // faces with a non-finite vertex
    uint32_t box[6];                // enc_float of lo[3], hi[3] over the usable faces
    unsigned long long pairs;       // (face, cell) pairs at the resolution last counted
    unsigned long long tests;       // point-triangle tests of the last query
};

size_t meshdist_workspace_bytes(int64_t nf, int res_max, MeshdistLayout* lay);

// validate the indices, copy the faces into padded records, bounding box and `skipped` into MeshdistSmall
hipError_t meshdist_records(char* ws, const MeshdistLayout& lay, const float* verts, int64_t nv, const int32_t* faces,
                            int64_t nf, hipStream_t s);
// MeshdistSmall::pairs for grid g (touches no cell)
hipError_t meshdist_count_pairs(char* ws, const MeshdistLayout& lay, int64_t nf, const r3g_md::Grid& g, hipStream_t s);
// per-cell counts -> exclusive scan -> fill of pairs [MeshdistSmall::pairs] with face ids
hipError_t meshdist_fill(char* ws, const MeshdistLayout& lay, int64_t nf, const r3g_md::Grid& g, int32_t* pairs, hipStream_t s);
hipError_t meshdist_query(char* ws, const MeshdistLayout& lay, const r3g_md::Grid& g, const int32_t* pairs, const float* points,
                          int64_t n, float* dist2, int32_t* face, hipStream_t s);

void meshdist_add_tests(int64_t n);     // r3g_get_counter("meshdist_tests")
int64_t meshdist_tests_total();

}  // namespace r3g
#endif
