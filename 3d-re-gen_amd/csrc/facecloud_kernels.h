// facecloud_kernels.h -- host-side interface of facecloud_kernels.hip (internal to libr3g.so)
#ifndef R3G_FACECLOUD_KERNELS_H
#define R3G_FACECLOUD_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "facecloud_core.h"

namespace r3g {

struct FacecloudLayout {
    size_t off_small;     // FacecloudSmall
    size_t off_recs;      // r3g_md::Tri [F]
    size_t off_wide;      // int32 [F]: the wide faces, in the order the cursor handed out (no output depends on it)
    size_t total;
};

// the bytes read back through the context's 64-byte pinned buffer
struct FacecloudSmall {
    unsigned long long usable;      // faces with three indices in [0, V) and finite vertices
    unsigned long long tests;       // point-triangle tests
    uint32_t wide;                  // faces walked by a wave
    uint32_t max_ring;              // the largest ring walked
};
static_assert(sizeof(FacecloudSmall) == 24, "FacecloudSmall travels through the 64-byte pinned buffer");

size_t facecloud_workspace_bytes(int64_t n_faces, FacecloudLayout* lay);

// zero the record, then one lane per face: its three vertices as a r3g_md::Tri, usable or not, narrow or wide
hipError_t facecloud_classify(char* ws, const FacecloudLayout& lay, const r3g_fc::Grid& g, const float* verts, int64_t n_verts, const int32_t* tri,
                              int64_t n_faces, hipStream_t s);
// one lane per face: the unusable faces' outputs, and the walk of the narrow ones
hipError_t facecloud_narrow(char* ws, const FacecloudLayout& lay, const r3g_fc::Grid& g, const r3g_fc::Pt* sorted, const unsigned* starts,
                            int64_t n_faces, float* dist2, int32_t* index, float* weights, float* diff, hipStream_t s);
// one wave per wide face
hipError_t facecloud_wide(char* ws, const FacecloudLayout& lay, const r3g_fc::Grid& g, const r3g_fc::Pt* sorted, const unsigned* starts,
                          int64_t n_faces, float* dist2, int32_t* index, float* weights, float* diff, hipStream_t s);
// one lane per vertex over the corner CSR of section 4o: grad_verts [V][3]
hipError_t facecloud_gather(const float* grad_dist2, const int32_t* index, const float* weights, const float* diff, const int32_t* corner_start,
                            const int32_t* corner_ids, int64_t n_verts, int64_t n_faces, float* grad_verts, hipStream_t s);

}  // namespace r3g
#endif
