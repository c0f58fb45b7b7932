// softras_kernels.h -- launchers of the soft silhouette (the definition is softras_core.h)
#ifndef R3G_SOFTRAS_KERNELS_H
#define R3G_SOFTRAS_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#ifndef R3G_SR_HD
#define R3G_SR_HD static inline
#endif
#include "softras_core.h"

namespace r3g {

// what a call reads back: 32 bytes
struct SoftrasSmall {
    unsigned long long pairs;        // (face, tile) pairs of the bin pass, counted in 64 bits
    unsigned long long used;         // faces that are drawn and whose box meets the image
    unsigned long long skipped;      // faces that are not drawn (softras_core.h, face_drawn; an index outside the vertices)
    unsigned long long found;        // backward: (pixel, face) pairs whose fragment was in the pixel's stored list
};

struct SoftrasLayout {
    size_t off_small, off_count, off_start, off_cursor, off_scan, total;
    int64_t tiles;
};

struct SoftrasGeom {
    int height, width, tiles_x, tiles_y, K;
    float sigma, blur_radius, blur_reach;      // blur_reach = sqrtf(blur_radius), rounded once on the host
};

size_t softras_workspace_bytes(int height, int width, SoftrasLayout* lay);

// zeroes the record and the per-tile counts, counts each drawn face into the tiles of its box: a memset and one launch (no launch
// when n_faces == 0), then the exclusive scan of the counts (three launches): start[t], start[tiles] = the pair count modulo 2^32
hipError_t softras_bin_count(char* ws, const SoftrasLayout& lay, const SoftrasGeom& g, const float* pos, int64_t n_verts, const int32_t* tri,
                             int64_t n_faces, hipStream_t s);
// writes each face into its tiles' segments of `pairs` (in the order the atomics fall: the forward does not depend on it)
hipError_t softras_bin_fill(char* ws, const SoftrasLayout& lay, const SoftrasGeom& g, const float* pos, int64_t n_verts, const int32_t* tri,
                            int64_t n_faces, int32_t* pairs, unsigned n_pairs, hipStream_t s);
// one wave per tile: the K smallest keys of every pixel and the blend
hipError_t softras_forward(const char* ws, const SoftrasLayout& lay, const SoftrasGeom& g, const float* pos, int64_t n_verts, const int32_t* tri,
                           int64_t n_faces, const int32_t* pairs, float* alpha, int32_t* face, float* dist, float* zbuf, hipStream_t s);
// one workgroup per face: grad_face float32 [n_faces][3][2] in the order of softras_core.h
hipError_t softras_backward(char* ws, const SoftrasLayout& lay, const SoftrasGeom& g, const float* pos, int64_t n_verts, const int32_t* tri,
                            int64_t n_faces, const int32_t* face, const float* dist, const float* grad_alpha, float* grad_face, hipStream_t s);
// one lane per vertex: grad_pos float32 [n_verts][3] from the corners corner_ids[corner_start[v] .. corner_start[v + 1])
hipError_t softras_gather(const float* grad_face, const int32_t* corner_start, const int32_t* corner_ids, int64_t n_verts, int64_t n_faces,
                          float* grad_pos, hipStream_t s);

}  // namespace r3g
#endif
