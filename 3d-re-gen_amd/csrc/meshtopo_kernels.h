// meshtopo_kernels.h -- host-side interface of meshtopo_kernels.hip (internal to libr3g.so)
#ifndef R3G_MESHTOPO_KERNELS_H
#define R3G_MESHTOPO_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#ifndef R3G_MT_HD
#ifdef __HIPCC__
#define R3G_MT_HD static __host__ __device__ __forceinline__
#else
#define R3G_MT_HD static inline
#endif
#endif
#include "meshtopo_core.h"

namespace r3g {

// everything a build leaves on the device, inside Ctx::meshtopo_ws
struct MeshtopoLayout {
    size_t off_small;     // r3g_mt::Small
    size_t off_label;     // int32 [F]: the labels of the rounds, then (body << 1) | parity
    size_t off_mate;      // int32 [3 F]
    size_t off_hslot;     // uint32 [3 F]: the table slot of every half-edge
    size_t off_hclash;    // uint8 [3 F]: the mate runs in the same direction
    size_t off_body;      // int32 [F]
    size_t off_flip;      // uint8 [F]
    size_t off_unori;     // uint32 [F]: at a body's lowest face, != 0 when the body is unorientable
    size_t off_bodyvol;   // int64 [F]: at a body's lowest face, its quantised six-volume as `flip` would wind it
    size_t off_vmark;     // uint32 [(V + 31) / 32]: referenced-vertex bits
    size_t off_keys;      // uint64 [slots]
    size_t off_counts;    // uint64 [slots]: forward | backward << 32
    size_t off_lo;        // int32 [slots]
    size_t off_hi;        // int32 [slots]
    uint64_t slots;
    size_t total;
};

size_t meshtopo_workspace_bytes(int64_t nv, int64_t nf, MeshtopoLayout* lay);

// index range, usable flags (label = self or -1), referenced vertices, the |coordinate| maximum; verts may be null
hipError_t meshtopo_check(char* ws, const MeshtopoLayout& lay, const float* verts, int64_t nv, const int32_t* faces, int64_t nf,
                          hipStream_t s);
// edge insert and classify: mate, clash bits, class counts
hipError_t meshtopo_edges(char* ws, const MeshtopoLayout& lay, const int32_t* faces, int64_t nf, hipStream_t s);
// one label round; Small::changed says whether anything moved
hipError_t meshtopo_round(char* ws, const MeshtopoLayout& lay, int64_t nf, hipStream_t s);
// after the last round: unorientable marks, body / flip, body and total sums (verts may be null: no sums)
hipError_t meshtopo_finish(char* ws, const MeshtopoLayout& lay, const float* verts, const int32_t* faces, int64_t nf, hipStream_t s);
// reverse in place: flip, then (outward 1) the orientable bodies of negative volume or (outward 2) all of them if the total is
hipError_t meshtopo_apply(char* ws, const MeshtopoLayout& lay, int32_t* faces, int64_t nf, int outward, hipStream_t s);

}  // namespace r3g
#endif
