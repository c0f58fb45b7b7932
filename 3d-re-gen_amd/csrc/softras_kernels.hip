// softras_kernels.hip -- the soft silhouette on the device (the definition is softras_core.h).
//
// sr_bin_count / sr_bin_fill: one lane per face.  The face's pixel box (face_box: clamped in float, so a finite coordinate of any
//             size is safe) is cut into 8 x 8 tiles; count[tile] and the cursor of the fill are integer atomics, the starts come
//             from the shared device-wide scan.  The order inside a tile's segment is whatever the atomics gave; the forward keeps
//             a set and sorts it, so nothing downstream depends on it.
// sr_forward: one wave per tile, one lane per pixel.  The tile's faces are walked with wave-uniform (scalar) loads; a lane keeps
//             its K smallest keys (pz, face) with their distances in LDS, element j of lane l at [j][l] (consecutive lanes,
//             consecutive banks), by insertion into the sorted list.  Then the blend and the four outputs.
// sr_backward: one workgroup of four waves per face.  Thread t walks the pixels t, t + 256, ... of the face's box in raster order,
//             recomputes the fragment (the same text as the forward, so the same branch), finds the face in the pixel's stored
//             list and adds its terms to six sums; butterfly per wave, ((w0 + w1) + w2) + w3 through LDS.  No floating-point
//             atomics anywhere.
// sr_gather:  one lane per vertex over its corners in ascending corner index.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define R3G_SR_HD static __host__ __device__ __forceinline__
#include "scan_kernels.h"
#include "softras_kernels.h"

namespace r3g {
namespace {

using r3g_sr::Box;
using r3g_sr::Frag;
using r3g_sr::kBackThreads;
using r3g_sr::kTile;
using r3g_sr::Tri;

constexpr int kBlock = 256;
static_assert(kBackThreads == 256 && kTile == 8, "four waves a face; a tile is one wave");
static_assert(sizeof(SoftrasSmall) == 32, "the record the host reads back");

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// FILL = false: count[tile] += 1 and the record's sums; FILL = true: pairs[start[tile] + cursor[tile]++] = f
template <bool FILL>
__global__ __launch_bounds__(kBlock) void sr_bin(const float* __restrict__ pos, int64_t n_verts, const int32_t* __restrict__ tri, int64_t n_faces,
                                                 SoftrasGeom g, unsigned* __restrict__ count, const unsigned* __restrict__ start,
                                                 int32_t* __restrict__ pairs, unsigned n_pairs, SoftrasSmall* __restrict__ small) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned my_pairs = 0, used = 0, skipped = 0;
    if (f < n_faces) {
        Tri T;
        float area;
        if (!r3g_sr::load_tri(pos, n_verts, tri, f, &T) || !r3g_sr::face_drawn(T, &area)) {
            skipped = 1;
        } else {
            const Box b = r3g_sr::face_box(T, g.blur_reach, g.width, g.height);
            if (!r3g_sr::box_empty(b)) {
                used = 1;
                for (int ty = b.y0 / kTile; ty <= b.y1 / kTile; ++ty)
                    for (int tx = b.x0 / kTile; tx <= b.x1 / kTile; ++tx) {
                        const int64_t t = (int64_t)ty * g.tiles_x + tx;
                        if (FILL) {
                            const unsigned at = start[t] + atomicAdd(&count[t], 1u);
                            if (at < n_pairs) pairs[at] = (int32_t)f;
                        } else {
                            atomicAdd(&count[t], 1u);
                            ++my_pairs;
                        }
                    }
            }
        }
    }
    if (!FILL) {
        my_pairs = wave_sum_u32(my_pairs), used = wave_sum_u32(used), skipped = wave_sum_u32(skipped);
        if ((threadIdx.x & 63) == 0) {
            if (my_pairs) atomicAdd(&small->pairs, (unsigned long long)my_pairs);
            if (used) atomicAdd(&small->used, (unsigned long long)used);
            if (skipped) atomicAdd(&small->skipped, (unsigned long long)skipped);
        }
    }
}

__global__ __launch_bounds__(64) void sr_forward(const float* __restrict__ pos, int64_t n_verts, const int32_t* __restrict__ tri, int64_t n_faces,
                                                 SoftrasGeom g, const unsigned* __restrict__ start, const int32_t* __restrict__ pairs,
                                                 float* __restrict__ alpha, int32_t* __restrict__ face, float* __restrict__ dist,
                                                 float* __restrict__ zbuf) {
    extern __shared__ float lds[];      // [K][64] pz, [K][64] face, [K][64] dist
    const int lane = threadIdx.x, K = g.K;
    const int tx = blockIdx.x % g.tiles_x, ty = blockIdx.x / g.tiles_x;
    const int x = tx * kTile + (lane & 7), y = ty * kTile + (lane >> 3);
    const bool valid = x < g.width && y < g.height;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    float* lpz = lds + lane;
    int32_t* lface = reinterpret_cast<int32_t*>(lds + K * 64) + lane;
    float* ldist = lds + 2 * K * 64 + lane;
    int n = 0;
    const unsigned p0 = start[blockIdx.x], p1 = start[blockIdx.x + 1];
    for (unsigned p = p0; p < p1; ++p) {
        const int32_t f = __builtin_amdgcn_readfirstlane(pairs[p]);      // the same face for the whole wave: its rows come as scalar loads
        Tri T;
        float area;
        if (f < 0 || f >= n_faces || !r3g_sr::load_tri(pos, n_verts, tri, f, &T) || !r3g_sr::face_drawn(T, &area)) continue;
        if (valid) {
            const Frag fr = r3g_sr::fragment(T, area, px, py, g.blur_radius);
            if (fr.kept) r3g_sr::list_insert(lpz, lface, ldist, 64, &n, K, fr.pz, f, fr.dist);
        }
    }
    if (!valid) return;
    const size_t pix = (size_t)y * g.width + x;
    alpha[pix] = r3g_sr::blend(ldist, 64, n, g.sigma);
    for (int k = 0; k < K; ++k) {
        const bool has = k < n;
        face[pix * K + k] = has ? lface[k * 64] : -1;
        dist[pix * K + k] = has ? ldist[k * 64] : -1.0f;
        zbuf[pix * K + k] = has ? lpz[k * 64] : -1.0f;
    }
}

__global__ __launch_bounds__(kBackThreads) void sr_backward(const float* __restrict__ pos, int64_t n_verts, const int32_t* __restrict__ tri,
                                                            SoftrasGeom g, const int32_t* __restrict__ face, const float* __restrict__ dist,
                                                            const float* __restrict__ grad_alpha, float* __restrict__ grad_face,
                                                            SoftrasSmall* __restrict__ small) {
    __shared__ float sh[4][6];
    const int64_t f = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    unsigned found = 0;
    Tri T;
    float area;
    if (r3g_sr::load_tri(pos, n_verts, tri, f, &T) && r3g_sr::face_drawn(T, &area)) {
        const Box b = r3g_sr::face_box(T, g.blur_reach, g.width, g.height);
        if (!r3g_sr::box_empty(b)) {
            const int bw = b.x1 - b.x0 + 1, npix = bw * (b.y1 - b.y0 + 1);      // at most 2^28
            for (int i = threadIdx.x; i < npix; i += kBackThreads) {
                const int y = b.y0 + i / bw, x = b.x0 + i % bw;
                const size_t pix = (size_t)y * g.width + x;
                found += r3g_sr::back_pixel(T, area, (float)x + 0.5f, (float)y + 0.5f, g.blur_radius, g.sigma, grad_alpha[pix], face + pix * g.K,
                                            dist + pix * g.K, g.K, (int32_t)f, acc)
                             ? 1u
                             : 0u;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float v = acc[k];
        for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
        if (lane == 0) sh[wave][k] = v;
    }
    found = wave_sum_u32(found);
    if (lane == 0 && found) atomicAdd(&small->found, (unsigned long long)found);
    __syncthreads();
    if (threadIdx.x < 6) grad_face[f * 6 + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void sr_gather(const float* __restrict__ grad_face, const int32_t* __restrict__ corner_start,
                                                    const int32_t* __restrict__ corner_ids, int64_t n_verts, int64_t n_corners,
                                                    float* __restrict__ grad_pos) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n_verts) return;
    int64_t c0 = corner_start[v], c1 = corner_start[v + 1];
    c0 = c0 < 0 ? 0 : c0, c1 = c1 > n_corners ? n_corners : c1;      // (a list the caller got wrong must not read past the arrays)
    float gx = 0.0f, gy = 0.0f;
    for (int64_t c = c0; c < c1; ++c) {
        const int32_t id = corner_ids[c];
        if (id < 0 || id >= n_corners) continue;
        gx = gx + grad_face[2 * (int64_t)id], gy = gy + grad_face[2 * (int64_t)id + 1];
    }
    grad_pos[3 * v] = gx, grad_pos[3 * v + 1] = gy, grad_pos[3 * v + 2] = 0.0f;
}

}  // namespace

size_t softras_workspace_bytes(int height, int width, SoftrasLayout* lay) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const int64_t tiles = (int64_t)((height + kTile - 1) / kTile) * ((width + kTile - 1) / kTile);
    size_t o = 0;
    lay->tiles = tiles;
    lay->off_small = o, o += up(sizeof(SoftrasSmall));
    lay->off_count = o, o += up(4 * (size_t)(tiles + 1));       // [tiles] stays 0, so that start[tiles] is the pair count
    lay->off_cursor = o, o += up(4 * (size_t)(tiles + 1));
    lay->off_start = o, o += up(4 * (size_t)(tiles + 1));
    lay->off_scan = o, o += up(4 * scan_scratch_elems(tiles + 1));
    lay->total = o;
    return o;
}

hipError_t softras_bin_count(char* ws, const SoftrasLayout& lay, const SoftrasGeom& g, const float* pos, int64_t n_verts, const int32_t* tri,
                             int64_t n_faces, hipStream_t s) {
    // the record, the counts and the cursors lie next to each other
    hipError_t e = hipMemsetAsync(ws + lay.off_small, 0, lay.off_start - lay.off_small, s);
    if (e != hipSuccess) return e;
    unsigned* count = (unsigned*)(ws + lay.off_count);
    if (n_faces) {
        hipLaunchKernelGGL(sr_bin<false>, dim3((unsigned)((n_faces + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, pos, n_verts, tri, n_faces, g, count,
                           (const unsigned*)nullptr, (int32_t*)nullptr, 0u, (SoftrasSmall*)(ws + lay.off_small));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return exclusive_scan_u32(count, (unsigned*)(ws + lay.off_start), lay.tiles + 1, (unsigned*)(ws + lay.off_scan), nullptr, s);
}

hipError_t softras_bin_fill(char* ws, const SoftrasLayout& lay, const SoftrasGeom& g, const float* pos, int64_t n_verts, const int32_t* tri,
                            int64_t n_faces, int32_t* pairs, unsigned n_pairs, hipStream_t s) {
    if (!n_faces || !n_pairs) return hipSuccess;
    hipLaunchKernelGGL(sr_bin<true>, dim3((unsigned)((n_faces + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, pos, n_verts, tri, n_faces, g,
                       (unsigned*)(ws + lay.off_cursor), (const unsigned*)(ws + lay.off_start), pairs, n_pairs, (SoftrasSmall*)nullptr);
    return hipGetLastError();
}

hipError_t softras_forward(const char* ws, const SoftrasLayout& lay, const SoftrasGeom& g, const float* pos, int64_t n_verts, const int32_t* tri,
                           int64_t n_faces, const int32_t* pairs, float* alpha, int32_t* face, float* dist, float* zbuf, hipStream_t s) {
    hipLaunchKernelGGL(sr_forward, dim3((unsigned)lay.tiles), dim3(64), (size_t)12 * 64 * g.K, s, pos, n_verts, tri, n_faces, g,
                       (const unsigned*)(ws + lay.off_start), pairs, alpha, face, dist, zbuf);
    return hipGetLastError();
}

hipError_t softras_backward(char* ws, const SoftrasLayout& lay, const SoftrasGeom& g, const float* pos, int64_t n_verts, const int32_t* tri,
                            int64_t n_faces, const int32_t* face, const float* dist, const float* grad_alpha, float* grad_face, hipStream_t s) {
    hipError_t e = hipMemsetAsync(ws + lay.off_small, 0, sizeof(SoftrasSmall), s);
    if (e != hipSuccess || !n_faces) return e;
    hipLaunchKernelGGL(sr_backward, dim3((unsigned)n_faces), dim3(kBackThreads), 0, s, pos, n_verts, tri, g, face, dist, grad_alpha, grad_face,
                       (SoftrasSmall*)(ws + lay.off_small));
    return hipGetLastError();
}

hipError_t softras_gather(const float* grad_face, const int32_t* corner_start, const int32_t* corner_ids, int64_t n_verts, int64_t n_faces,
                          float* grad_pos, hipStream_t s) {
    if (!n_verts) return hipSuccess;
    hipLaunchKernelGGL(sr_gather, dim3((unsigned)((n_verts + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, grad_face, corner_start, corner_ids, n_verts,
                       3 * n_faces, grad_pos);
    return hipGetLastError();
}

}  // namespace r3g
