// kvsel_kernels.hip -- adaptive top-k selection of the geo decoder's cross-attention keys.
//
//   kvsel_regroup : Q [H][npad][64] of a pass -> [groups][H][G][64], the layout in which the attention kernel takes the groups
//                   as batches with their own K / V^T (16-byte copies: one read and one write of the pass's Q)
//   kvsel_select  : one workgroup per (group, head).  The mean of the logits of the sampled query rows IS the logit of their
//                   mean, so the score of a key is one dot product with q-bar: a [N_lat x 64] matrix-vector product into LDS.
//                   Scores become order-preserving 32-bit keys, the k-th largest is found by radix select (8-bit digits, LDS
//                   histograms), and the selected indices are written ascending through 64-bit ballots and prefix counts.
//                   No global atomics; nothing depends on the order of the workgroups.
//   kvsel_vrows   : the row-major copy of V the gather reads (V^T columns would be 2-byte strided reads)
//   kvsel_gather  : K rows by index; V rows by index, transposed through LDS into the compact V^T in the kernel's key order
#include "kvsel_kernels.h"

#include "kernels.h"
#include "prof.h"

namespace r3g {
namespace {

constexpr int KV_THREADS = 256;
constexpr int KV_SELECT_LDS_EXTRA = (256 + 64 + 256 + 16 + 2) * 4;   // histogram, q-bar, partial sums, wave counts, select state

__device__ inline float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ inline float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// fp32 score -> unsigned key with the same order: a NaN ranks below every number, -0 and +0 are one key
__device__ inline unsigned score_key(float s) {
    if (s != s) return 0u;
    if (s == 0.0f) s = 0.0f;
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(KV_THREADS) void kvsel_regroup_kernel(const uint16_t* __restrict__ q, int heads, int lq_pad, int group,
                                                                  int full, int tail_pad, uint16_t* __restrict__ out) {
    const int64_t rows = (int64_t)full * group + tail_pad;      // output rows per head
    const int64_t t = (int64_t)blockIdx.x * KV_THREADS + threadIdx.x;
    const int part = (int)(t & 7);
    const int64_t ri = t >> 3;
    if (ri >= rows * heads) return;
    const int h = (int)(ri / rows);
    const int64_t r = ri % rows;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < lq_pad) v = *reinterpret_cast<const uint4*>(q + ((int64_t)h * lq_pad + r) * 64 + part * 8);
    const int64_t g = r / group;
    int64_t dst;
    if (g < full) dst = ((g * heads + h) * group + r % group) * 64;
    else dst = ((int64_t)full * heads * group + (int64_t)h * tail_pad + (r - (int64_t)full * group)) * 64;
    *reinterpret_cast<uint4*>(out + dst + part * 8) = v;
}

__global__ __launch_bounds__(KV_THREADS) void kvsel_select_kernel(const uint16_t* __restrict__ q, int lq, int lq_pad,
                                                                 const uint16_t* __restrict__ k, int lk, int lk_pad, int heads,
                                                                 int group, int stride, int topk, int32_t* __restrict__ idx) {
    extern __shared__ unsigned kv_smem[];
    unsigned* keys = kv_smem;                                    // [lk]
    unsigned* hist = keys + lk;                                  // [256]
    float* qbar = reinterpret_cast<float*>(hist + 256);          // [64]
    float* part = qbar + 64;                                     // [4][64]
    unsigned* wc = reinterpret_cast<unsigned*>(part + 256);      // [2][8] counts per wave
    unsigned* st = wc + 16;                                      // [2] digit found, rank left
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int g = blockIdx.x / heads, h = blockIdx.x % heads;
    const int rows = min(group, lq - g * group);
    const int S = (rows + stride - 1) / stride;                  // rows r of the group with r % stride == 0 (one for a short tail)

    // q-bar: mean of the sampled rows, fp32
    {
        const uint16_t* qg = q + ((int64_t)h * lq_pad + (int64_t)g * group) * 64;
        const int d = t & 63, sub = t >> 6;
        float acc = 0.0f;
        for (int si = sub; si < S; si += 4) acc += __uint_as_float((unsigned)qg[(int64_t)si * stride * 64 + d] << 16);
        part[sub * 64 + d] = acc;
        __syncthreads();
        if (t < 64) qbar[t] = (((part[t] + part[64 + t]) + part[128 + t]) + part[192 + t]) / (float)S;
        __syncthreads();
    }
    // score[key] = q-bar . k[key], as an order-preserving key
    for (int key = t; key < lk; key += KV_THREADS) {
        const uint4* kr = reinterpret_cast<const uint4*>(k + ((int64_t)h * lk_pad + key) * 64);
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint4 v = kr[c];
            const float* qb = qbar + c * 8;
            s = fmaf(bf16_lo(v.x), qb[0], s); s = fmaf(bf16_hi(v.x), qb[1], s);
            s = fmaf(bf16_lo(v.y), qb[2], s); s = fmaf(bf16_hi(v.y), qb[3], s);
            s = fmaf(bf16_lo(v.z), qb[4], s); s = fmaf(bf16_hi(v.z), qb[5], s);
            s = fmaf(bf16_lo(v.w), qb[6], s); s = fmaf(bf16_hi(v.w), qb[7], s);
        }
        keys[key] = score_key(s);
    }
    // radix select of the topk-th largest key: after the four digits `prefix` is that key and `need` says how many of the keys
    // equal to it belong to the selection
    unsigned prefix = 0, mask = 0, need = (unsigned)topk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
        for (int key = t; key < lk; key += KV_THREADS) {
            const unsigned u = keys[key];
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        const unsigned c = hist[255 - t];                        // thread t owns digit 255 - t: an inclusive scan from the top
        unsigned incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wc[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += wc[w];
        if (incl >= need && incl - c < need) {                   // exactly one digit holds the rank
            st[0] = (unsigned)(255 - t);
            st[1] = need - (incl - c);
        }
        __syncthreads();
        prefix |= st[0] << shift;
        mask |= 255u << shift;
        need = st[1];
    }
    // the selection in ascending key index: every key above the threshold, and the first `need` keys at it
    int32_t* out = idx + (int64_t)blockIdx.x * topk;
    unsigned run_gt = 0, run_eq = 0;
    for (int base = 0, it = 0; base < lk; base += KV_THREADS, ++it) {
        const int key = base + t;
        const unsigned u = key < lk ? keys[key] : 0u;
        const bool gt = key < lk && u > prefix, eq = key < lk && u == prefix;
        const unsigned long long bg = __ballot(gt), be = __ballot(eq);
        unsigned* w = wc + (it & 1) * 8;
        if (lane == 0) { w[wave] = (unsigned)__popcll(bg); w[4 + wave] = (unsigned)__popcll(be); }
        __syncthreads();
        unsigned gb = run_gt, eb = run_eq;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < wave) { gb += w[i]; eb += w[4 + i]; }
            run_gt += w[i];
            run_eq += w[4 + i];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        gb += (unsigned)__popcll(bg & below);
        eb += (unsigned)__popcll(be & below);
        if (gt || (eq && eb < need)) {
            const unsigned pos = gb + min(eb, need);
            if (pos < (unsigned)topk) out[pos] = key;
        }
    }
}

__global__ __launch_bounds__(KV_THREADS) void kvsel_vrows_kernel(const uint16_t* __restrict__ vt, int lk, int lk_pad, int heads,
                                                                uint16_t* __restrict__ v) {
    const int64_t t = (int64_t)blockIdx.x * KV_THREADS + threadIdx.x;
    if (t >= (int64_t)heads * 8 * lk) return;
    const int key = (int)(t % lk), c = (int)((t / lk) & 7), h = (int)(t / ((int64_t)8 * lk));
    const uint16_t* src = vt + ((int64_t)h * 64 + c * 8) * lk_pad + vt_key_pos(key);
    unsigned w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (unsigned)src[(int64_t)(2 * e) * lk_pad] | ((unsigned)src[(int64_t)(2 * e + 1) * lk_pad] << 16);
    *reinterpret_cast<uint4*>(v + ((int64_t)h * lk + key) * 64 + c * 8) = make_uint4(w[0], w[1], w[2], w[3]);
}

// one workgroup per (64 compact keys, group * H + head)
__global__ __launch_bounds__(KV_THREADS) void kvsel_gather_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, int lk,
                                                                 int lk_pad, int heads, const int32_t* __restrict__ idx, int topk,
                                                                 int kpad, uint16_t* __restrict__ k_out, uint16_t* __restrict__ vt_out) {
    __shared__ unsigned tile[64 * 33];     // V rows of the tile, [key][dim pair], 33 dwords per row
    __shared__ int src[64];
    const int t = threadIdx.x, gh = blockIdx.y, h = gh % heads, j0 = blockIdx.x * 64;
    if (t < 64) {
        const int j = j0 + t;
        int sk = j < topk ? idx[(int64_t)gh * topk + j] : -1;
        if (sk < 0 || sk >= lk) sk = -1;                         // padding (and anything that is not a key): zeros
        src[t] = sk;
    }
    __syncthreads();
#pragma unroll
    for (int c = t; c < 512; c += KV_THREADS) {
        const int row = c >> 3, part = c & 7, sk = src[row];
        uint4 kv = make_uint4(0, 0, 0, 0), vv = kv;
        if (sk >= 0) {
            kv = *reinterpret_cast<const uint4*>(k + ((int64_t)h * lk_pad + sk) * 64 + part * 8);
            vv = *reinterpret_cast<const uint4*>(v + ((int64_t)h * lk + sk) * 64 + part * 8);
        }
        *reinterpret_cast<uint4*>(k_out + ((int64_t)gh * kpad + j0 + row) * 64 + part * 8) = kv;
        unsigned* tr = tile + row * 33 + part * 4;
        tr[0] = vv.x; tr[1] = vv.y; tr[2] = vv.z; tr[3] = vv.w;
    }
    __syncthreads();
#pragma unroll
    for (int c = t; c < 512; c += KV_THREADS) {
        const int d = c >> 3, p0 = (c & 7) * 8;
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // vt_key_pos swaps two blocks: it is its own inverse, position p holds compact key vt_key_pos(p)
            const unsigned a = tile[(int)vt_key_pos(p0 + 2 * e) * 33 + (d >> 1)], b = tile[(int)vt_key_pos(p0 + 2 * e + 1) * 33 + (d >> 1)];
            const unsigned lo = (d & 1) ? a >> 16 : a & 0xffffu, hi = (d & 1) ? b >> 16 : b & 0xffffu;
            w[e] = lo | (hi << 16);
        }
        *reinterpret_cast<uint4*>(vt_out + ((int64_t)gh * 64 + d) * kpad + j0 + p0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace

hipError_t kvsel_regroup_launch(const uint16_t* q, int heads, int lq, int lq_pad, int group, uint16_t* out, hipStream_t s) {
    if (!q || !out || heads < 1 || lq < 1 || lq > lq_pad || group < 256 || group % 256) return hipErrorInvalidValue;
    const KvselCut c = kvsel_cut(lq, group);
    const int64_t chunks = ((int64_t)c.full * group + c.tail_pad) * heads * 8;
    ProfScope prof_scope_(PC_QKV_SPLIT, (double)chunks * 32, s);
    hipLaunchKernelGGL(kvsel_regroup_kernel, dim3((unsigned)((chunks + KV_THREADS - 1) / KV_THREADS)), dim3(KV_THREADS), 0, s, q, heads,
                       lq_pad, group, c.full, c.tail_pad, out);
    return hipGetLastError();
}

hipError_t kvsel_select_launch(const uint16_t* q, int lq, int lq_pad, const uint16_t* k, int lk, int lk_pad, int heads, int group,
                               int stride, int topk, int32_t* idx, hipStream_t s) {
    if (!q || !k || !idx || heads < 1 || lq < 1 || lq > lq_pad || lk < 1 || lk > lk_pad || group < 256 || group % 256 || stride < 1 ||
        topk < 1 || topk > lk)
        return hipErrorInvalidValue;
    const size_t lds = (size_t)lk * 4 + KV_SELECT_LDS_EXTRA;
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const int groups = kvsel_cut(lq, group).groups;
    ProfScope prof_scope_(PC_GEMV, 2.0 * 64 * lk * (double)groups * heads, s);
    hipLaunchKernelGGL(kvsel_select_kernel, dim3((unsigned)(groups * heads)), dim3(KV_THREADS), lds, s, q, lq, lq_pad, k, lk, lk_pad, heads,
                       group, stride, topk, idx);
    return hipGetLastError();
}

hipError_t kvsel_vrows_launch(const uint16_t* vt, int lk, int lk_pad, int heads, uint16_t* v, hipStream_t s) {
    if (!vt || !v || heads < 1 || lk < 1 || lk > lk_pad || lk_pad % 16) return hipErrorInvalidValue;
    const int64_t n = (int64_t)heads * 8 * lk;
    ProfScope prof_scope_(PC_ELEMWISE, (double)n * 32, s);
    hipLaunchKernelGGL(kvsel_vrows_kernel, dim3((unsigned)((n + KV_THREADS - 1) / KV_THREADS)), dim3(KV_THREADS), 0, s, vt, lk, lk_pad, heads, v);
    return hipGetLastError();
}

hipError_t kvsel_gather_launch(const uint16_t* k, const uint16_t* v, int lk, int lk_pad, int heads, const int32_t* idx, int groups,
                               int topk, uint16_t* k_out, uint16_t* vt_out, hipStream_t s) {
    if (!k || !v || !idx || !k_out || !vt_out || heads < 1 || groups < 1 || lk < 1 || lk > lk_pad || topk < 1 || topk > lk ||
        (int64_t)groups * heads > 65535)
        return hipErrorInvalidValue;
    const int kpad = (topk + 63) / 64 * 64;
    ProfScope prof_scope_(PC_ELEMWISE, 4.0 * 128 * kpad * (double)groups * heads, s);
    hipLaunchKernelGGL(kvsel_gather_kernel, dim3((unsigned)(kpad / 64), (unsigned)(groups * heads)), dim3(KV_THREADS), 0, s, k, v, lk, lk_pad,
                       heads, idx, topk, kpad, k_out, vt_out);
    return hipGetLastError();
}

}  // namespace r3g
