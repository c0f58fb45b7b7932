// meshfill_kernels.h -- host-side interface of meshfill_kernels.hip (internal to libr3g.so)
#ifndef R3G_MESHFILL_KERNELS_H
#define R3G_MESHFILL_KERNELS_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#ifndef R3G_MF_HD
#ifdef __HIPCC__
#define R3G_MF_HD static __host__ __device__ __forceinline__
#else
#define R3G_MF_HD static inline
#endif
#endif
#include "meshfill_core.h"

namespace r3g {

constexpr int kFillTile = 2048;       // slots per block of the compaction and of the allocation scans

// everything a plan leaves on the device, inside Ctx::meshfill_ws.  B = boundary half-edges (slots), V = vertices.
struct MeshfillLayout {
    size_t off_small;        // r3g_mf::Small
    size_t off_deg;          // uint64 [V]: nout | nin << 32
    size_t off_outc;         // int32 [V]: the slot that leaves the vertex, where nout = 1
    size_t off_tilecnt;      // uint32 [half-edge tiles + 1]: boundary half-edges per tile
    size_t off_tilestart;    // uint32 [half-edge tiles + 1]: their exclusive scan
    size_t off_scratch;      // uint32: the tile sums of exclusive_scan_u32
    size_t off_bh;           // int32 [B]: the half-edge id of every slot, ascending
    size_t off_succ;         // int32 [B]
    size_t off_lead;         // int32 [B]: the leader's slot, -1 for a tangled slot
    size_t off_x[2];         // int32 [B] twice: m of the minimum doubling, then q of the rank doubling
    size_t off_y[2];         // int32 [B] twice: p, then d; off_y[final] holds d after the plan
    size_t off_scan[4];      // uint32 [B] each, read at leaders: loop ordinal, loop start, filled ordinal, face base
    size_t off_tsum[4];      // uint32 [slot tiles + 1] each
    size_t off_lverts;       // int32 [B]: the loop vertices, loop after loop in rank order (the first loop_edges in use)
    size_t off_cent;         // float [3 * (B / 3)]: the centroids of the filled loops (mode 1)
    int64_t n3, he_tiles, slots, slot_tiles;
    int final;
    size_t total;
};

size_t meshfill_workspace_bytes(int64_t nv, int64_t nf, int64_t boundary, MeshfillLayout* lay);

// Everything between the mate table and the counts, without a read-back: compaction, vertex pass, succ, the two doublings of
// `rounds` rounds each, allocation, loop vertices and (mode 1) centroids.  boundary > 0.  lay->final is set.
hipError_t meshfill_plan(char* ws, MeshfillLayout* lay, const int32_t* mate, const float* verts, int64_t nv, const int32_t* faces,
                         int rounds, int64_t max_loop, int mode, hipStream_t s);
// the appended faces [faces_added][3] and (mode 1, new_verts may be null) vertices [filled][3]
hipError_t meshfill_emit(const char* ws, const MeshfillLayout& lay, int64_t nv, int64_t max_loop, int mode, int64_t filled,
                         int64_t faces_added, int32_t* new_faces, float* new_verts, hipStream_t s);
// loop_start int64 [loops + 1], loop_verts int32 [loop_edges], status int32 [loops]
hipError_t meshfill_loops(const char* ws, const MeshfillLayout& lay, int64_t max_loop, int64_t loops, int64_t loop_edges,
                          int64_t* loop_start, int32_t* loop_verts, int32_t* status, hipStream_t s);

}  // namespace r3g
#endif
