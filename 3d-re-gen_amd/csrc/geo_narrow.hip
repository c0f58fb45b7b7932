// geo_narrow.hip -- fused tail of a narrow (width 256) geo decoder for gfx950.
//
//   x1    = x0 + c_proj(cat) + b            fp32 registers
//   xn    = bf16(ln_3(x1))                  statistics and affine in fp32, eps 1e-6
//   h     = bf16(gelu_erf(c_fc(xn) + b))    fp32 accumulator, GELU in fp32
//   x2    = x1 + mlp.c_proj(h) + b          fp32 registers, the hidden taken 32 units at a time
//   logit = output_proj(ln_post(x2))        fp32, eps 1e-5; ln_post optional
//
// The generic path runs this as five launches that move the stream, its normalised copy and the hidden through HBM.  Here a
// workgroup of four waves owns 128 rows, each wave 32 of them (two 16-row MFMA tiles) across all 256 columns, and nothing but
// the logits is stored.
//
// Every product is computed TRANSPOSED on v_mfma_f32_16x16x32_bf16: D = W X^T, the weight fragment as the A operand, the rows'
// activations as the B operand.  A lane (r = lane & 15, q = lane >> 4) then holds, for row r of its tile, the four output
// channels 16 j + 4 q + {0..3} of every 16-channel block j -- and the B operand of the NEXT product wants, for that same row, eight
// values of the summed index per lane.  A sum does not care about the order of its terms: the lane's own eight values of the
// blocks 2 kf and 2 kf + 1 ARE its B fragment kf, provided the weight fragment lists the summed index in the same permuted
// order, k(kf, q, e) = 32 kf + 16 (e >> 2) + 4 q + (e & 3).  So activations never change lanes between the three products: no LDS
// turn, no shuffles; a row's statistics are a sum over the lane's registers and over the four lanes r, r + 16, r + 32, r + 48.
// The permutation lives in the weights: geo_tail_pack lays them out once per grid query as a stream of ready fragments (1 KiB each,
// lane-major) in the order of consumption.  The workgroup copies that stream through LDS in panels of 32 fragments, double
// buffered (2 x 32 KiB): the four waves share every fragment, and the 384 KiB - 1.1 MiB of weights stay L2-resident.
#include "geo_narrow.h"

#include "gemm_common.h"
#include "prof.h"

namespace r3g {
namespace {

constexpr int GT_THREADS = 256;
constexpr int GT_MT = 2;                          // 16-row MFMA tiles per wave
constexpr int GT_ROWS = 4 * 16 * GT_MT;           // rows per workgroup
constexpr int GT_PANEL = 32;                      // fragments per LDS panel
constexpr int GT_PANEL_U4 = GT_PANEL * 64;        // ... in 16-byte units
constexpr int GT_LDS_BYTES = 2 * GT_PANEL_U4 * 16;

union Frag {
    uint4 u;
    bf16x8 v;
};

__device__ __forceinline__ float quad_sum(float v) {      // over the four lanes that share a row: r, r + 16, r + 32, r + 48
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

__global__ __launch_bounds__(GT_THREADS) void geo_tail_pack_kernel(const uint16_t* __restrict__ wp, int64_t ldp,
                                                                   const uint16_t* __restrict__ wfc, int64_t ldfc,
                                                                   const uint16_t* __restrict__ wfp, int64_t ldfp, int frags,
                                                                   uint4* __restrict__ out) {
    const int idx = blockIdx.x * GT_THREADS + threadIdx.x;
    const int f = idx >> 6, lane = idx & 63, r = lane & 15, q = lane >> 4;
    if (f >= frags) return;
    const uint16_t* row;
    int col_lo, col_hi;      // columns of elements 0..3 and 4..7
    if (f < 128) {           // c_proj: output block f >> 3, k-fragment f & 7, the summed index in natural order
        row = wp + (int64_t)(16 * (f >> 3) + r) * ldp;
        col_lo = 32 * (f & 7) + 8 * q;
        col_hi = col_lo + 4;
    } else {
        const int g = f - 128, hp = g >> 5, u = g & 31;
        if (u < 16) {        // mlp.c_fc: hidden block 2 hp + (u >> 3), k-fragment u & 7 over ln_3's output in register order
            row = wfc + (int64_t)(32 * hp + 16 * (u >> 3) + r) * ldfc;
            col_lo = 32 * (u & 7) + 4 * q;
        } else {             // mlp.c_proj: output block u - 16, summed over the 32 hidden units of hp in register order
            row = wfp + (int64_t)(16 * (u - 16) + r) * ldfp;
            col_lo = 32 * hp + 4 * q;
        }
        col_hi = col_lo + 16;
    }
    const uint2 lo = *reinterpret_cast<const uint2*>(row + col_lo), hi = *reinterpret_cast<const uint2*>(row + col_hi);
    out[idx] = make_uint4(lo.x, lo.y, hi.x, hi.y);
}

__global__ __launch_bounds__(GT_THREADS) void geo_tail_kernel(GeoTailArgs p) {
    extern __shared__ uint4 gt_lds[];             // [2][GT_PANEL_U4]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, q = lane >> 4;
    const uint4* __restrict__ packed = reinterpret_cast<const uint4*>(p.packed);
    const int panels = 4 + p.hidden / 32;
    int64_t row[GT_MT];
#pragma unroll
    for (int mt = 0; mt < GT_MT; ++mt) {
        const int64_t m = (int64_t)blockIdx.x * GT_ROWS + wave * (16 * GT_MT) + 16 * mt + r;
        row[mt] = m < p.n ? m : (int64_t)p.n - 1;      // a row past n repeats the last one: read in bounds, never stored
    }
    constexpr int NST = GT_PANEL_U4 / GT_THREADS;
    {   // panel 0 -> LDS
        uint4 st[NST];
#pragma unroll
        for (int i = 0; i < NST; ++i) st[i] = packed[t + GT_THREADS * i];
#pragma unroll
        for (int i = 0; i < NST; ++i) gt_lds[t + GT_THREADS * i] = st[i];
    }

    // the rows' attention output as B fragments, and acc = x0 + b_proj in the accumulator layout
    Frag catf[8][GT_MT];
#pragma unroll
    for (int kf = 0; kf < 8; ++kf)
#pragma unroll
        for (int mt = 0; mt < GT_MT; ++mt)
            catf[kf][mt].u = *reinterpret_cast<const uint4*>(p.cat + row[mt] * p.ld_cat + 32 * kf + 8 * q);
    f32x4 acc[16][GT_MT];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float4 b = *reinterpret_cast<const float4*>(p.b_proj + 16 * j + 4 * q);
#pragma unroll
        for (int mt = 0; mt < GT_MT; ++mt) {
            const uint2 w = *reinterpret_cast<const uint2*>(p.x0 + row[mt] * p.ld_x0 + 16 * j + 4 * q);
            const f32x2 lo = unpack16<false>(w.x), hi = unpack16<false>(w.y);
            acc[j][mt] = (f32x4){lo[0] + b.x, lo[1] + b.y, hi[0] + b.z, hi[1] + b.w};
        }
    }
    __syncthreads();

    // ---- c_proj: panels 0..3, four output blocks each
#pragma unroll
    for (int pi = 0; pi < 4; ++pi) {
        uint4 st[NST];
#pragma unroll
        for (int i = 0; i < NST; ++i) st[i] = packed[(int64_t)(pi + 1) * GT_PANEL_U4 + t + GT_THREADS * i];
        const uint4* buf = gt_lds + (pi & 1) * GT_PANEL_U4;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int kf = 0; kf < 8; ++kf) {
                Frag w;
                w.u = buf[(jj * 8 + kf) * 64 + lane];
#pragma unroll
                for (int mt = 0; mt < GT_MT; ++mt)
                    acc[4 * pi + jj][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w.v, catf[kf][mt].v, acc[4 * pi + jj][mt], 0, 0, 0);
            }
        uint4* nxt = gt_lds + ((pi + 1) & 1) * GT_PANEL_U4;
#pragma unroll
        for (int i = 0; i < NST; ++i) nxt[t + GT_THREADS * i] = st[i];
        __syncthreads();
    }

    // ---- ln_3 of x1 (fp32) -> bf16 B fragments of mlp.c_fc; then acc = x1 + b of mlp.c_proj
    Frag xnf[8][GT_MT];
    {
        float mean[GT_MT], rstd[GT_MT];
#pragma unroll
        for (int mt = 0; mt < GT_MT; ++mt) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) s += (acc[j][mt][0] + acc[j][mt][1]) + (acc[j][mt][2] + acc[j][mt][3]);
            mean[mt] = quad_sum(s) * (1.0f / 256.0f);
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = acc[j][mt][c] - mean[mt];
                    v = fmaf(d, d, v);
                }
            rstd[mt] = 1.0f / sqrtf(quad_sum(v) * (1.0f / 256.0f) + 1e-6f);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float4 g = *reinterpret_cast<const float4*>(p.ln3_w + 16 * j + 4 * q);
            const float4 b = *reinterpret_cast<const float4*>(p.ln3_b + 16 * j + 4 * q);
            const float4 b2 = *reinterpret_cast<const float4*>(p.b_fp + 16 * j + 4 * q);
#pragma unroll
            for (int mt = 0; mt < GT_MT; ++mt) {
                const f32x4 x = acc[j][mt];
                const float y0 = fmaf((x[0] - mean[mt]) * rstd[mt], g.x, b.x), y1 = fmaf((x[1] - mean[mt]) * rstd[mt], g.y, b.y);
                const float y2 = fmaf((x[2] - mean[mt]) * rstd[mt], g.z, b.z), y3 = fmaf((x[3] - mean[mt]) * rstd[mt], g.w, b.w);
                const uint32_t w0 = pack_bf16(y0, y1), w1 = pack_bf16(y2, y3);
                if (j & 1) { xnf[j >> 1][mt].u.z = w0; xnf[j >> 1][mt].u.w = w1; }
                else { xnf[j >> 1][mt].u.x = w0; xnf[j >> 1][mt].u.y = w1; }
                acc[j][mt] = (f32x4){x[0] + b2.x, x[1] + b2.y, x[2] + b2.z, x[3] + b2.w};
            }
        }
    }

    // ---- the MLP, 32 hidden units per panel: 16 fragments of mlp.c_fc, then 16 of mlp.c_proj
    for (int pi = 4; pi < panels; ++pi) {
        // (the last panel fetches itself once more and parks it in the buffer nobody reads again: no branch around the copy)
        const int64_t nxt_panel = pi + 1 < panels ? pi + 1 : pi;
        uint4 st[NST];
#pragma unroll
        for (int i = 0; i < NST; ++i) st[i] = packed[nxt_panel * GT_PANEL_U4 + t + GT_THREADS * i];
        const uint4* buf = gt_lds + (pi & 1) * GT_PANEL_U4;
        const int h0 = 32 * (pi - 4);
        f32x4 h[2][GT_MT];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float4 bb = *reinterpret_cast<const float4*>(p.b_fc + h0 + 16 * b + 4 * q);
#pragma unroll
            for (int mt = 0; mt < GT_MT; ++mt) h[b][mt] = (f32x4){bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int kf = 0; kf < 8; ++kf) {
                Frag w;
                w.u = buf[(b * 8 + kf) * 64 + lane];
#pragma unroll
                for (int mt = 0; mt < GT_MT; ++mt) h[b][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w.v, xnf[kf][mt].v, h[b][mt], 0, 0, 0);
            }
        }
        Frag hf[GT_MT];
#pragma unroll
        for (int mt = 0; mt < GT_MT; ++mt) {
            hf[mt].u.x = pack_bf16(gelu_erf(h[0][mt][0]), gelu_erf(h[0][mt][1]));
            hf[mt].u.y = pack_bf16(gelu_erf(h[0][mt][2]), gelu_erf(h[0][mt][3]));
            hf[mt].u.z = pack_bf16(gelu_erf(h[1][mt][0]), gelu_erf(h[1][mt][1]));
            hf[mt].u.w = pack_bf16(gelu_erf(h[1][mt][2]), gelu_erf(h[1][mt][3]));
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            Frag w;
            w.u = buf[(16 + j) * 64 + lane];
#pragma unroll
            for (int mt = 0; mt < GT_MT; ++mt) acc[j][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w.v, hf[mt].v, acc[j][mt], 0, 0, 0);
        }
        uint4* nxt = gt_lds + ((pi + 1) & 1) * GT_PANEL_U4;
#pragma unroll
        for (int i = 0; i < NST; ++i) nxt[t + GT_THREADS * i] = st[i];
        __syncthreads();
    }

    // ---- ln_post (optional) and output_proj on x2, fp32
    const bool lnp = p.lnp_w != nullptr;
#pragma unroll
    for (int mt = 0; mt < GT_MT; ++mt) {
        float mean = 0.f, rstd = 1.f;
        if (lnp) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) s += (acc[j][mt][0] + acc[j][mt][1]) + (acc[j][mt][2] + acc[j][mt][3]);
            mean = quad_sum(s) * (1.0f / 256.0f);
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = acc[j][mt][c] - mean;
                    v = fmaf(d, d, v);
                }
            rstd = 1.0f / sqrtf(quad_sum(v) * (1.0f / 256.0f) + 1e-5f);
        }
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float4 w = *reinterpret_cast<const float4*>(p.out_w + 16 * j + 4 * q);
            f32x4 y = acc[j][mt];
            if (lnp) {
                const float4 g = *reinterpret_cast<const float4*>(p.lnp_w + 16 * j + 4 * q);
                const float4 b = *reinterpret_cast<const float4*>(p.lnp_b + 16 * j + 4 * q);
                y = (f32x4){fmaf((y[0] - mean) * rstd, g.x, b.x), fmaf((y[1] - mean) * rstd, g.y, b.y),
                            fmaf((y[2] - mean) * rstd, g.z, b.z), fmaf((y[3] - mean) * rstd, g.w, b.w)};
            }
            dot = fmaf(y[0], w.x, dot);
            dot = fmaf(y[1], w.y, dot);
            dot = fmaf(y[2], w.z, dot);
            dot = fmaf(y[3], w.w, dot);
        }
        dot = quad_sum(dot) + p.out_b;
        const int64_t m = (int64_t)blockIdx.x * GT_ROWS + wave * (16 * GT_MT) + 16 * mt + r;
        if (q == 0 && m < p.n) p.out[m] = dot;
    }
}

}  // namespace

hipError_t geo_tail_pack_launch(const uint16_t* w_proj, int64_t ld_proj, const uint16_t* w_fc, int64_t ld_fc, const uint16_t* w_fp,
                                int64_t ld_fp, int hidden, void* packed, hipStream_t s) {
    if (!w_proj || !w_fc || !w_fp || !packed || !geo_tail_supported(GEO_TAIL_WIDTH, hidden)) return hipErrorInvalidValue;
    if (ld_proj < 256 || ld_fc < 256 || ld_fp < hidden || (ld_proj | ld_fc | ld_fp) % 4) return hipErrorInvalidValue;   // 8-byte loads
    if (((uintptr_t)w_proj | (uintptr_t)w_fc | (uintptr_t)w_fp) % 8 || (uintptr_t)packed % 16) return hipErrorInvalidValue;
    const int frags = 128 + hidden;
    ProfScope prof_scope_(PC_ELEMWISE, 2.0 * 1024 * frags, s);
    hipLaunchKernelGGL(geo_tail_pack_kernel, dim3((unsigned)(frags * 64 / GT_THREADS)), dim3(GT_THREADS), 0, s, w_proj, ld_proj, w_fc, ld_fc,
                       w_fp, ld_fp, frags, reinterpret_cast<uint4*>(packed));
    return hipGetLastError();
}

hipError_t geo_tail_launch(const GeoTailArgs& p, hipStream_t s) {
    if (!p.cat || !p.x0 || !p.packed || !p.b_proj || !p.ln3_w || !p.ln3_b || !p.b_fc || !p.b_fp || !p.out_w || !p.out || p.n < 1 ||
        !geo_tail_supported(GEO_TAIL_WIDTH, p.hidden) || (p.lnp_w == nullptr) != (p.lnp_b == nullptr))
        return hipErrorInvalidValue;
    // 16-byte row loads of cat, 8-byte of x0, 16-byte of the vectors
    if (p.ld_cat < 256 || p.ld_cat % 8 || (uintptr_t)p.cat % 16 || p.ld_x0 < 256 || p.ld_x0 % 4 || (uintptr_t)p.x0 % 8 || (uintptr_t)p.packed % 16)
        return hipErrorInvalidValue;
    const uintptr_t vecs = (uintptr_t)p.b_proj | (uintptr_t)p.ln3_w | (uintptr_t)p.ln3_b | (uintptr_t)p.b_fc | (uintptr_t)p.b_fp |
                           (uintptr_t)p.out_w | (uintptr_t)p.lnp_w | (uintptr_t)p.lnp_b;
    if (vecs % 16) return hipErrorInvalidValue;
    const double flops = 2.0 * p.n * (256.0 * 256 + 2.0 * 256 * p.hidden);
    ProfScope prof_scope_(PC_GEMM, flops, s, (double)p.n * (2 * 256 * 2 + 4) + (double)geo_tail_packed_bytes(p.hidden));
    hipLaunchKernelGGL(geo_tail_kernel, dim3((unsigned)((p.n + GT_ROWS - 1) / GT_ROWS)), dim3(GT_THREADS), GT_LDS_BYTES, s, p);
    return hipGetLastError();
}

}  // namespace r3g
