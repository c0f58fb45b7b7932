// meshfill_kernels.hip -- boundary loops of a triangle mesh and the faces that close them.
//
// compact (the boundary half-edges of the mate table into B slots by ascending id: tile counts, exclusive_scan_u32 of scan_kernels,
// tile write) -> vertex pass (one 64-bit add per endpoint) -> link (the slot that leaves each vertex of nout = 1) -> succ ->
// minimum / open by pointer doubling -> rank by Wyllie doubling -> allocate (four scans over the leaders) -> loop vertices ->
// centroids -> emit.  Every doubling round reads the previous round's arrays and writes the other pair, so no round races;
// the atomics are integer adds and one maximum, and their order decides nothing.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_MF_HD static __host__ __device__ __forceinline__
#include "mesh_launch.h"
#include "meshfill_kernels.h"
#include "scan_kernels.h"

namespace r3g {
namespace {

using r3g_mf::Small;

constexpr int kItems = kFillTile / kT;      // consecutive slots per thread, so that a tile keeps its order

// WRITE = false: tilecnt[tile] = boundary half-edges of the tile.  WRITE = true: bh[tilestart[tile] + ...] = their ids.
template <bool WRITE>
__global__ __launch_bounds__(kT) void mf_compact(const int32_t* __restrict__ mate, int64_t n3, int64_t tiles, unsigned* __restrict__ tilecnt,
                                                 const unsigned* __restrict__ tilestart, int32_t* __restrict__ bh, int64_t slots) {
    __shared__ unsigned sh[kT / 64];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * kFillTile + (int64_t)threadIdx.x * kItems;
        unsigned bits = 0, cnt = 0;
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const bool b = base + i < n3 && mate[base + i] == -1;
            bits |= (unsigned)b << i;
            cnt += b;
        }
        unsigned total;
        const unsigned off = block_exclusive_scan<kT / 64>(cnt, sh, &total);
        if (!WRITE) {
            if (threadIdx.x == 0) tilecnt[tile] = total;
        } else {
            int64_t pos = (int64_t)tilestart[tile] + off;
#pragma unroll
            for (int i = 0; i < kItems; ++i)
                if ((bits >> i) & 1u) {
                    if (pos < slots) bh[pos] = (int32_t)(base + i);
                    ++pos;
                }
        }
    }
}

__global__ __launch_bounds__(kT) void mf_vertex(const int32_t* __restrict__ bh, const int32_t* __restrict__ faces, int64_t slots,
                                                unsigned long long* __restrict__ deg) {
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        const int64_t h = bh[c];
        atomicAdd(&deg[r3g_mf::he_tail(faces, h)], r3g_mf::kDegOut);
        atomicAdd(&deg[r3g_mf::he_head(faces, h)], r3g_mf::kDegIn);
    }
}

// a vertex of nout = 1 has exactly one writer
__global__ __launch_bounds__(kT) void mf_link(const int32_t* __restrict__ bh, const int32_t* __restrict__ faces, int64_t slots,
                                              const unsigned long long* __restrict__ deg, int32_t* __restrict__ outc) {
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        const int32_t v = r3g_mf::he_tail(faces, bh[c]);
        if (r3g_mf::deg_out(deg[v]) == 1u) outc[v] = (int32_t)c;
    }
}

__global__ __launch_bounds__(kT) void mf_succ(const int32_t* __restrict__ bh, const int32_t* __restrict__ faces, int64_t slots,
                                              const unsigned long long* __restrict__ deg, const int32_t* __restrict__ outc,
                                              int32_t* __restrict__ succ, int32_t* __restrict__ m, int32_t* __restrict__ p) {
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        const int32_t v = r3g_mf::he_head(faces, bh[c]);
        const int32_t sc = r3g_mf::vertex_simple(deg[v]) ? outc[v] : -1;
        succ[c] = sc;
        m[c] = (int32_t)c;
        p[c] = sc;
    }
}

struct Load32 {
    const int32_t* a;
    __device__ int32_t operator()(int32_t i) const { return a[i]; }
};

__global__ __launch_bounds__(kT) void mf_min_round(int64_t slots, const int32_t* __restrict__ mi, const int32_t* __restrict__ pi,
                                                   int32_t* __restrict__ mo, int32_t* __restrict__ po) {
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        int32_t m, p;
        r3g_mf::min_step(Load32{mi}, Load32{pi}, mi[c], pi[c], &m, &p);
        mo[c] = m;
        po[c] = p;
    }
}

__global__ __launch_bounds__(kT) void mf_rank_init(int64_t slots, const int32_t* __restrict__ m, const int32_t* __restrict__ p,
                                                   const int32_t* __restrict__ succ, int32_t* __restrict__ lead,
                                                   int32_t* __restrict__ q, int32_t* __restrict__ d) {
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        const bool open = p[c] < 0;
        const int32_t l = open ? -1 : m[c];
        const bool terminal = open || l == (int32_t)c;
        lead[c] = l;
        q[c] = terminal ? (int32_t)c : succ[c];
        d[c] = terminal ? 0 : 1;
    }
}

__global__ __launch_bounds__(kT) void mf_rank_round(int64_t slots, const int32_t* __restrict__ qi, const int32_t* __restrict__ di,
                                                    int32_t* __restrict__ qo, int32_t* __restrict__ dout) {
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        int32_t q, d;
        r3g_mf::rank_step(Load32{qi}, Load32{di}, qi[c], di[c], &q, &d);
        qo[c] = q;
        dout[c] = d;
    }
}

struct Four {
    unsigned* a[4];
};

// The four numbers a leader adds to the scans: one loop, its length, one filled loop, its faces.
// WRITE = false: the tile's sums, the totals and the longest loop.  WRITE = true: the exclusive scans at every slot.
template <bool WRITE>
__global__ __launch_bounds__(kT) void mf_allocate(int64_t slots, int64_t tiles, const int32_t* __restrict__ lead,
                                                  const int32_t* __restrict__ succ, const int32_t* __restrict__ d, int64_t max_loop,
                                                  int mode, Four tsum, Four scan, Small* __restrict__ sm) {
    __shared__ unsigned sh[kT / 64];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * kFillTile + (int64_t)threadIdx.x * kItems;
        unsigned val[4][kItems], sum[4] = {0, 0, 0, 0}, longest = 0;
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const int64_t c = base + i;
            val[0][i] = val[1][i] = val[2][i] = val[3][i] = 0;
            if (c < slots && lead[c] == (int32_t)c) {
                const int32_t len = r3g_mf::loop_length(d[succ[c]]);
                const bool keep = r3g_mf::loop_kept(len, max_loop);
                val[0][i] = 1;
                val[1][i] = (unsigned)len;
                val[2][i] = keep;
                val[3][i] = keep ? r3g_mf::loop_faces(len, mode) : 0u;
                longest = (unsigned)len > longest ? (unsigned)len : longest;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) sum[k] += val[k][i];
        }
        unsigned off[4], total[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) off[k] = block_exclusive_scan<kT / 64>(sum[k], sh, &total[k]);
        if (!WRITE) {
            if (threadIdx.x == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) tsum.a[k][tile] = total[k];
                if (total[0]) {
                    atomicAdd(&sm->loops, (unsigned long long)total[0]);
                    atomicAdd(&sm->loop_edges, (unsigned long long)total[1]);
                }
                if (total[2]) {
                    atomicAdd(&sm->filled, (unsigned long long)total[2]);
                    atomicAdd(&sm->faces_added, (unsigned long long)total[3]);
                }
            }
            for (int dd = 32; dd >= 1; dd >>= 1) {
                const unsigned o = __shfl_xor(longest, dd, 64);
                longest = o > longest ? o : longest;
            }
            if ((threadIdx.x & 63) == 0 && longest) atomicMax(&sm->longest, longest);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned run = tsum.a[k][tile] + off[k];
#pragma unroll
                for (int i = 0; i < kItems; ++i) {
                    if (base + i < slots) scan.a[k][base + i] = run;
                    run += val[k][i];
                }
            }
        }
    }
}

// what the later passes need of a slot's loop, read at its leader
struct LoopOf {
    int32_t length, rank;
    unsigned ordinal, start, filled_ordinal, face_base;
    bool kept;
};

struct Plan {
    const int32_t *bh, *succ, *lead, *d;
    const unsigned *s_ord, *s_start, *s_fill, *s_face;
    const int32_t* lverts;
};

__device__ __forceinline__ bool loop_of(const Plan& pl, int64_t c, int64_t max_loop, LoopOf* lo) {
    const int32_t l = pl.lead[c];
    if (l < 0) return false;
    lo->length = r3g_mf::loop_length(pl.d[pl.succ[l]]);
    lo->rank = r3g_mf::loop_rank(lo->length, pl.d[c]);
    lo->ordinal = pl.s_ord[l], lo->start = pl.s_start[l], lo->filled_ordinal = pl.s_fill[l], lo->face_base = pl.s_face[l];
    lo->kept = r3g_mf::loop_kept(lo->length, max_loop);
    return true;
}

__global__ __launch_bounds__(kT) void mf_loop_verts(int64_t slots, Plan pl, const int32_t* __restrict__ faces, int64_t max_loop,
                                                    int32_t* __restrict__ lverts) {
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        LoopOf lo;
        if (!loop_of(pl, c, max_loop, &lo)) continue;
        const int64_t at = (int64_t)lo.start + lo.rank;
        if (at < slots) lverts[at] = r3g_mf::he_tail(faces, pl.bh[c]);
    }
}

struct LoopCoord {
    const float* verts;
    const int32_t* a;
    __device__ float operator()(int32_t i, int k) const { return verts[3 * (int64_t)a[i] + k]; }
};

// one lane per filled loop: at most max_loop sequential additions in the fixed order
__global__ __launch_bounds__(kT) void mf_centroids(int64_t slots, Plan pl, const float* __restrict__ verts, int64_t max_loop,
                                                   float* __restrict__ cent) {
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        if (pl.lead[c] != (int32_t)c) continue;
        LoopOf lo;
        loop_of(pl, c, max_loop, &lo);
        if (!lo.kept || 3 * ((int64_t)lo.filled_ordinal + 1) > slots) continue;
        float out[3];
        r3g_mf::loop_centroid(LoopCoord{verts, pl.lverts + lo.start}, lo.length, out);
        cent[3 * (int64_t)lo.filled_ordinal] = out[0];
        cent[3 * (int64_t)lo.filled_ordinal + 1] = out[1];
        cent[3 * (int64_t)lo.filled_ordinal + 2] = out[2];
    }
}

// one lane per slot; a slot of a filled loop writes at most one face
__global__ __launch_bounds__(kT) void mf_emit_faces(int64_t slots, Plan pl, int64_t nv, int64_t max_loop, int mode,
                                                    int64_t faces_added, int32_t* __restrict__ new_faces) {
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        LoopOf lo;
        if (!loop_of(pl, c, max_loop, &lo) || !lo.kept) continue;
        int32_t f[3];
        const int32_t at = r3g_mf::loop_face(Load32{pl.lverts + lo.start}, lo.length, lo.rank, mode, (int32_t)(nv + lo.filled_ordinal), f);
        if (at < 0 || (int64_t)lo.face_base + at >= faces_added) continue;
        int32_t* dst = new_faces + 3 * ((int64_t)lo.face_base + at);
        dst[0] = f[0], dst[1] = f[1], dst[2] = f[2];
    }
}

__global__ __launch_bounds__(kT) void mf_loop_table(int64_t slots, Plan pl, int64_t max_loop, int64_t loops, int64_t loop_edges,
                                                    int64_t* __restrict__ loop_start, int32_t* __restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x == 0) loop_start[loops] = loop_edges;
    for (int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x; c < slots; c += (int64_t)gridDim.x * kT) {
        if (pl.lead[c] != (int32_t)c) continue;
        LoopOf lo;
        loop_of(pl, c, max_loop, &lo);
        if ((int64_t)lo.ordinal >= loops) continue;
        loop_start[lo.ordinal] = (int64_t)lo.start;
        status[lo.ordinal] = lo.kept ? 0 : 1;
    }
}

Plan plan_of(const char* ws, const MeshfillLayout& lay) {
    Plan pl;
    pl.bh = (const int32_t*)(ws + lay.off_bh), pl.succ = (const int32_t*)(ws + lay.off_succ);
    pl.lead = (const int32_t*)(ws + lay.off_lead), pl.d = (const int32_t*)(ws + lay.off_y[lay.final]);
    pl.s_ord = (const unsigned*)(ws + lay.off_scan[0]), pl.s_start = (const unsigned*)(ws + lay.off_scan[1]);
    pl.s_fill = (const unsigned*)(ws + lay.off_scan[2]), pl.s_face = (const unsigned*)(ws + lay.off_scan[3]);
    pl.lverts = (const int32_t*)(ws + lay.off_lverts);
    return pl;
}

unsigned tile_grid(int64_t tiles) { return tiles < 1 ? 1u : (tiles > 4096 ? 4096u : (unsigned)tiles); }

}  // namespace

static_assert(sizeof(Small) == 40, "r3g_mf::Small travels through the context's 64-byte pinned buffer");
static_assert(kItems * kT == kFillTile && kItems <= 32, "a thread keeps one bit per slot of its part of the tile");

size_t meshfill_workspace_bytes(int64_t nv, int64_t nf, int64_t boundary, MeshfillLayout* lay) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t V = (size_t)nv, B = (size_t)boundary;
    lay->n3 = 3 * nf;
    lay->he_tiles = (lay->n3 + kFillTile - 1) / kFillTile;
    lay->slots = boundary;
    lay->slot_tiles = (boundary + kFillTile - 1) / kFillTile;
    lay->final = 0;
    const size_t ht1 = (size_t)lay->he_tiles + 1, st1 = (size_t)lay->slot_tiles + 1;
    size_t o = 0;
    lay->off_small = o, o += 256;
    lay->off_deg = o, o += up(8 * V);
    lay->off_outc = o, o += up(4 * V);
    lay->off_tilecnt = o, o += up(4 * ht1);
    lay->off_tilestart = o, o += up(4 * ht1);
    lay->off_scratch = o, o += up(4 * scan_scratch_elems((int64_t)(ht1 > st1 ? ht1 : st1)));
    lay->off_bh = o, o += up(4 * B);
    lay->off_succ = o, o += up(4 * B);
    lay->off_lead = o, o += up(4 * B);
    for (int k = 0; k < 2; ++k) lay->off_x[k] = o, o += up(4 * B);
    for (int k = 0; k < 2; ++k) lay->off_y[k] = o, o += up(4 * B);
    for (int k = 0; k < 4; ++k) lay->off_scan[k] = o, o += up(4 * B);
    for (int k = 0; k < 4; ++k) lay->off_tsum[k] = o, o += up(4 * st1);
    lay->off_lverts = o, o += up(4 * B);
    lay->off_cent = o, o += up(12 * (B / 3) + 4);
    lay->total = o;
    return o;
}

hipError_t meshfill_plan(char* ws, MeshfillLayout* layp, const int32_t* mate, const float* verts, int64_t nv, const int32_t* faces,
                         int rounds, int64_t max_loop, int mode, hipStream_t s) {
    MeshfillLayout& lay = *layp;
    const int64_t B = lay.slots;
    if (B < 1) return hipErrorInvalidValue;
    unsigned* tilecnt = (unsigned*)(ws + lay.off_tilecnt);
    unsigned* tilestart = (unsigned*)(ws + lay.off_tilestart);
    unsigned* scratch = (unsigned*)(ws + lay.off_scratch);
    int32_t* bh = (int32_t*)(ws + lay.off_bh);
    int32_t* succ = (int32_t*)(ws + lay.off_succ);
    int32_t* lead = (int32_t*)(ws + lay.off_lead);
    int32_t* x[2] = {(int32_t*)(ws + lay.off_x[0]), (int32_t*)(ws + lay.off_x[1])};
    int32_t* y[2] = {(int32_t*)(ws + lay.off_y[0]), (int32_t*)(ws + lay.off_y[1])};
    unsigned long long* deg = (unsigned long long*)(ws + lay.off_deg);
    int32_t* outc = (int32_t*)(ws + lay.off_outc);
    Small* sm = (Small*)(ws + lay.off_small);
    const unsigned gs = grid_for(B);

    R3G_HIP(hipMemsetAsync(sm, 0, sizeof(Small), s));
    R3G_HIP(hipMemsetAsync(deg, 0, 8 * (size_t)nv, s));
    R3G_HIP(hipMemsetAsync(tilecnt + lay.he_tiles, 0, 4, s));
    hipLaunchKernelGGL(mf_compact<false>, dim3(tile_grid(lay.he_tiles)), dim3(kT), 0, s, mate, lay.n3, lay.he_tiles, tilecnt,
                       (const unsigned*)nullptr, (int32_t*)nullptr, B);
    R3G_HIP(exclusive_scan_u32(tilecnt, tilestart, lay.he_tiles + 1, scratch, nullptr, s));
    hipLaunchKernelGGL(mf_compact<true>, dim3(tile_grid(lay.he_tiles)), dim3(kT), 0, s, mate, lay.n3, lay.he_tiles, (unsigned*)nullptr,
                       (const unsigned*)tilestart, bh, B);
    hipLaunchKernelGGL(mf_vertex, dim3(gs), dim3(kT), 0, s, (const int32_t*)bh, faces, B, deg);
    hipLaunchKernelGGL(mf_link, dim3(gs), dim3(kT), 0, s, (const int32_t*)bh, faces, B, (const unsigned long long*)deg, outc);
    hipLaunchKernelGGL(mf_succ, dim3(gs), dim3(kT), 0, s, (const int32_t*)bh, faces, B, (const unsigned long long*)deg,
                       (const int32_t*)outc, succ, x[0], y[0]);
    int cur = 0;
    for (int r = 0; r < rounds; ++r, cur ^= 1)
        hipLaunchKernelGGL(mf_min_round, dim3(gs), dim3(kT), 0, s, B, (const int32_t*)x[cur], (const int32_t*)y[cur], x[cur ^ 1], y[cur ^ 1]);
    hipLaunchKernelGGL(mf_rank_init, dim3(gs), dim3(kT), 0, s, B, (const int32_t*)x[cur], (const int32_t*)y[cur], (const int32_t*)succ,
                       lead, x[cur ^ 1], y[cur ^ 1]);
    cur ^= 1;
    for (int r = 0; r < rounds; ++r, cur ^= 1)
        hipLaunchKernelGGL(mf_rank_round, dim3(gs), dim3(kT), 0, s, B, (const int32_t*)x[cur], (const int32_t*)y[cur], x[cur ^ 1], y[cur ^ 1]);
    lay.final = cur;
    R3G_HIP(hipGetLastError());

    Four tsum, scan;
    for (int k = 0; k < 4; ++k) {
        tsum.a[k] = (unsigned*)(ws + lay.off_tsum[k]);
        scan.a[k] = (unsigned*)(ws + lay.off_scan[k]);
        R3G_HIP(hipMemsetAsync(tsum.a[k] + lay.slot_tiles, 0, 4, s));
    }
    hipLaunchKernelGGL(mf_allocate<false>, dim3(tile_grid(lay.slot_tiles)), dim3(kT), 0, s, B, lay.slot_tiles, (const int32_t*)lead,
                       (const int32_t*)succ, (const int32_t*)y[cur], max_loop, mode, tsum, scan, sm);
    for (int k = 0; k < 4; ++k) R3G_HIP(exclusive_scan_u32(tsum.a[k], tsum.a[k], lay.slot_tiles + 1, scratch, nullptr, s));
    hipLaunchKernelGGL(mf_allocate<true>, dim3(tile_grid(lay.slot_tiles)), dim3(kT), 0, s, B, lay.slot_tiles, (const int32_t*)lead,
                       (const int32_t*)succ, (const int32_t*)y[cur], max_loop, mode, tsum, scan, sm);
    const Plan pl = plan_of(ws, lay);
    hipLaunchKernelGGL(mf_loop_verts, dim3(gs), dim3(kT), 0, s, B, pl, faces, max_loop, (int32_t*)(ws + lay.off_lverts));
    if (mode == r3g_mf::kModeCentroid)
        hipLaunchKernelGGL(mf_centroids, dim3(gs), dim3(kT), 0, s, B, pl, verts, max_loop, (float*)(ws + lay.off_cent));
    return hipGetLastError();
}

hipError_t meshfill_emit(const char* ws, const MeshfillLayout& lay, int64_t nv, int64_t max_loop, int mode, int64_t filled,
                         int64_t faces_added, int32_t* new_faces, float* new_verts, hipStream_t s) {
    if (lay.slots < 1) return hipSuccess;
    if (new_faces && faces_added > 0)
        hipLaunchKernelGGL(mf_emit_faces, dim3(grid_for(lay.slots)), dim3(kT), 0, s, lay.slots, plan_of(ws, lay), nv, max_loop, mode,
                           faces_added, new_faces);
    if (mode == r3g_mf::kModeCentroid && new_verts && filled > 0)
        R3G_HIP(hipMemcpyAsync(new_verts, ws + lay.off_cent, 12 * (size_t)filled, hipMemcpyDeviceToDevice, s));
    return hipGetLastError();
}

hipError_t meshfill_loops(const char* ws, const MeshfillLayout& lay, int64_t max_loop, int64_t loops, int64_t loop_edges,
                          int64_t* loop_start, int32_t* loop_verts, int32_t* status, hipStream_t s) {
    if (lay.slots < 1 || loops < 1) return hipMemsetAsync(loop_start, 0, 8, s);
    hipLaunchKernelGGL(mf_loop_table, dim3(grid_for(lay.slots)), dim3(kT), 0, s, lay.slots, plan_of(ws, lay), max_loop, loops, loop_edges,
                       loop_start, status);
    R3G_HIP(hipMemcpyAsync(loop_verts, ws + lay.off_lverts, 4 * (size_t)loop_edges, hipMemcpyDeviceToDevice, s));
    return hipGetLastError();
}

}  // namespace r3g
