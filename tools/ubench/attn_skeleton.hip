// attn_skeleton.hip -- the instruction mix of attn3_kernel's key loop (64 queries per wave, head dimension 64) on operands that
// never leave registers / LDS, in several PROGRAM ORDERS, to measure what an in-order wave gains when its softmax instructions
// stand between its own MFMAs instead of behind them (profiles/attention_interleave.md).
//   per 32-key block and wave: 16 v_mfma_f32_32x32x16_bf16, 32 v_exp_f32, 16 v_cvt_pk_bf16_f32, the row sums, 8 ds_read_b128;
//   per 64-key tile: 4 LDS-DMA pieces (from a 16 KiB buffer that stays in L2), s_waitcnt vmcnt(0), s_barrier.
// Every instruction of the loop is an asm volatile statement, so the program order below IS the order in the code object.
// The vector instructions work on registers of their own (timing does not depend on their values; no instruction reads a
// transcendental result in the next slot), the MFMAs on random bf16 operands.
//   MODE 0 clustered : 8 QK^T MFMAs | softmax of both query blocks | 8 P V MFMAs          (today's order)
//   MODE 1 skewed    : every MFMA followed by its share of the OTHER query block's softmax (2 exp + cvt + packed add [+1])
//   MODE 2 skewed, the row sum on plain v_add_f32 (two per packed add: the same additions in the same order)
//   MODE 3 sweep     : every MFMA followed by NF vector instructions of which NE are v_exp_f32 (the rest v_cvt_pk / v_add)
// Occupancy: 256-thread workgroups; dynamic LDS of 96 KiB allows one per CU (one wave per SIMD), 64 KiB two.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o attn_skeleton attn_skeleton.hip && ./attn_skeleton
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

#define MFMA(acc, a, b) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b))
#define MFMA_FRESH(d, a, b, c) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c))
#define EXP(x) asm volatile("v_exp_f32 %0, %0" : "+v"(x))
#define CVT(d, x, y) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(y))
#define PKADD(acc, x) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(acc) : "v"(x))
#define ADD(acc, x) asm volatile("v_add_f32 %0, %0, %1" : "+v"(acc) : "v"(x))
#define CMP(x, y) asm volatile("v_cmp_lt_f32 vcc, %0, %1" ::"v"(x), "v"(y) : "vcc")
#define DSREAD(d, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:" #imm : "=v"(d) : "v"(addr))
#define LGKM0() asm volatile("s_waitcnt lgkmcnt(0)")

struct St {
    f32x16 s[2], o[2][2], negm;
    bf16x8 qf[4], kf[4], vf[4], pf[2];
    f32x2 e[2][8];      // the "scores" the exponentials run on, per query block
    f32x2 ps[2];
    float l[2];
    uint32_t pk[2];
    uint32_t lds;       // this lane's LDS read address
};

// one of the eight steps of a query block's softmax: 2 exponentials, and the conversion + row-sum add of the previous pair
template <int J, bool PLAIN>
__device__ __forceinline__ void sm_step(St& z, const int qb) {
    EXP(z.e[qb][J][0]);
    EXP(z.e[qb][J][1]);
    constexpr int P = (J + 7) & 7;
    CVT(z.pk[qb], z.e[qb][P][0], z.e[qb][P][1]);
    if (PLAIN) { ADD(z.ps[qb][0], z.e[qb][P][0]); ADD(z.ps[qb][1], z.e[qb][P][1]); }
    else PKADD(z.ps[qb], z.e[qb][P]);
    if (J == 1) ADD(z.ps[qb][0], z.ps[qb][1]);
    if (J == 2) ADD(z.l[qb], z.ps[qb][0]);
    if (J == 3) CMP(z.ps[qb][0], z.l[qb]);
}
template <bool PLAIN>
__device__ __forceinline__ void sm_all(St& z, const int qb) {
    sm_step<0, PLAIN>(z, qb); sm_step<1, PLAIN>(z, qb); sm_step<2, PLAIN>(z, qb); sm_step<3, PLAIN>(z, qb);
    sm_step<4, PLAIN>(z, qb); sm_step<5, PLAIN>(z, qb); sm_step<6, PLAIN>(z, qb); sm_step<7, PLAIN>(z, qb);
}

template <int NF, int NE>
__device__ __forceinline__ void fillers(St& z, const int g) {
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const int r = (g * NF + i) & 7;
        if (i < NE) EXP(z.e[i & 1][r][0]);
        else if ((i - NE) & 1) CVT(z.pk[i & 1], z.e[0][r][1], z.e[1][r][1]);
        else ADD(z.ps[i & 1][0], z.e[1][r][1]);
    }
}

// one 32-key block (kb = 0 / 1 of the tile at `cur`)
template <int MODE, int NF, int NE, int KB>
__device__ __forceinline__ void block(St& z) {
    constexpr int KO = KB * 4096, VO = 8192 + KB * 64;
    if constexpr (MODE == 0) {
        DSREAD(z.kf[0], z.lds, 0); DSREAD(z.kf[1], z.lds, 32); DSREAD(z.kf[2], z.lds, 64); DSREAD(z.kf[3], z.lds, 96);
        (void)KO;
        LGKM0();
        MFMA_FRESH(z.s[0], z.kf[0], z.qf[0], z.negm);
        MFMA_FRESH(z.s[1], z.kf[0], z.qf[1], z.negm);
        DSREAD(z.vf[0], z.lds, 8192); DSREAD(z.vf[1], z.lds, 8224); DSREAD(z.vf[2], z.lds, 8256); DSREAD(z.vf[3], z.lds, 8288);
        (void)VO;
        MFMA(z.s[0], z.kf[1], z.qf[1]); MFMA(z.s[1], z.kf[1], z.qf[2]);
        MFMA(z.s[0], z.kf[2], z.qf[2]); MFMA(z.s[1], z.kf[2], z.qf[3]);
        MFMA(z.s[0], z.kf[3], z.qf[3]); MFMA(z.s[1], z.kf[3], z.qf[0]);
        sm_all<false>(z, 0);
        sm_all<false>(z, 1);
        LGKM0();
        MFMA(z.o[0][0], z.vf[0], z.pf[0]); MFMA(z.o[1][0], z.vf[0], z.pf[1]);
        MFMA(z.o[0][1], z.vf[1], z.pf[0]); MFMA(z.o[1][1], z.vf[1], z.pf[1]);
        MFMA(z.o[0][0], z.vf[2], z.pf[0]); MFMA(z.o[1][0], z.vf[2], z.pf[1]);
        MFMA(z.o[0][1], z.vf[3], z.pf[0]); MFMA(z.o[1][1], z.vf[3], z.pf[1]);
    } else if constexpr (MODE == 1 || MODE == 2) {
        constexpr bool PL = MODE == 2;
        // the fragments of a group are read one group ahead (the loop enters with kf valid)
        // G1: QK^T(qb0, k+1) || softmax(qb1, k) first half
        LGKM0();
        MFMA_FRESH(z.s[0], z.kf[0], z.qf[0], z.negm); sm_step<0, PL>(z, 1); DSREAD(z.vf[0], z.lds, 8192);
        MFMA(z.s[0], z.kf[1], z.qf[1]);               sm_step<1, PL>(z, 1); DSREAD(z.vf[1], z.lds, 8224);
        MFMA(z.s[0], z.kf[2], z.qf[2]);               sm_step<2, PL>(z, 1); DSREAD(z.vf[2], z.lds, 8256);
        MFMA(z.s[0], z.kf[3], z.qf[3]);               sm_step<3, PL>(z, 1); DSREAD(z.vf[3], z.lds, 8288);
        // G2: P V(qb0, k) || softmax(qb1, k) second half
        LGKM0();
        MFMA(z.o[0][0], z.vf[0], z.pf[0]);            sm_step<4, PL>(z, 1);
        MFMA(z.o[0][1], z.vf[1], z.pf[0]);            sm_step<5, PL>(z, 1);
        MFMA(z.o[0][0], z.vf[2], z.pf[0]);            sm_step<6, PL>(z, 1);
        MFMA(z.o[0][1], z.vf[3], z.pf[0]);            sm_step<7, PL>(z, 1);
        // G3: QK^T(qb1, k+1) || softmax(qb0, k+1) first half   (K and V^T fragments stay live: no second read)
        MFMA_FRESH(z.s[1], z.kf[0], z.qf[1], z.negm); sm_step<0, PL>(z, 0);
        MFMA(z.s[1], z.kf[1], z.qf[2]);               sm_step<1, PL>(z, 0);
        MFMA(z.s[1], z.kf[2], z.qf[3]);               sm_step<2, PL>(z, 0);
        MFMA(z.s[1], z.kf[3], z.qf[0]);               sm_step<3, PL>(z, 0);
        // G4: P V(qb1, k) || softmax(qb0, k+1) second half; the K fragments of the next block are read here
        MFMA(z.o[1][0], z.vf[0], z.pf[1]);            sm_step<4, PL>(z, 0); DSREAD(z.kf[0], z.lds, 0);
        MFMA(z.o[1][1], z.vf[1], z.pf[1]);            sm_step<5, PL>(z, 0); DSREAD(z.kf[1], z.lds, 32);
        MFMA(z.o[1][0], z.vf[2], z.pf[1]);            sm_step<6, PL>(z, 0); DSREAD(z.kf[2], z.lds, 64);
        MFMA(z.o[1][1], z.vf[3], z.pf[1]);            sm_step<7, PL>(z, 0); DSREAD(z.kf[3], z.lds, 96);
    } else {
        LGKM0();
        MFMA_FRESH(z.s[0], z.kf[0], z.qf[0], z.negm); fillers<NF, NE>(z, 0); DSREAD(z.vf[0], z.lds, 8192);
        MFMA(z.s[0], z.kf[1], z.qf[1]);               fillers<NF, NE>(z, 1); DSREAD(z.vf[1], z.lds, 8224);
        MFMA(z.s[0], z.kf[2], z.qf[2]);               fillers<NF, NE>(z, 2); DSREAD(z.vf[2], z.lds, 8256);
        MFMA(z.s[0], z.kf[3], z.qf[3]);               fillers<NF, NE>(z, 3); DSREAD(z.vf[3], z.lds, 8288);
        LGKM0();
        MFMA(z.o[0][0], z.vf[0], z.pf[0]);            fillers<NF, NE>(z, 4);
        MFMA(z.o[0][1], z.vf[1], z.pf[0]);            fillers<NF, NE>(z, 5);
        MFMA(z.o[0][0], z.vf[2], z.pf[0]);            fillers<NF, NE>(z, 6);
        MFMA(z.o[0][1], z.vf[3], z.pf[0]);            fillers<NF, NE>(z, 7);
        MFMA_FRESH(z.s[1], z.kf[0], z.qf[1], z.negm); fillers<NF, NE>(z, 8);
        MFMA(z.s[1], z.kf[1], z.qf[2]);               fillers<NF, NE>(z, 9);
        MFMA(z.s[1], z.kf[2], z.qf[3]);               fillers<NF, NE>(z, 10);
        MFMA(z.s[1], z.kf[3], z.qf[0]);               fillers<NF, NE>(z, 11);
        MFMA(z.o[1][0], z.vf[0], z.pf[1]);            fillers<NF, NE>(z, 12); DSREAD(z.kf[0], z.lds, 0);
        MFMA(z.o[1][1], z.vf[1], z.pf[1]);            fillers<NF, NE>(z, 13); DSREAD(z.kf[1], z.lds, 32);
        MFMA(z.o[1][0], z.vf[2], z.pf[1]);            fillers<NF, NE>(z, 14); DSREAD(z.kf[2], z.lds, 64);
        MFMA(z.o[1][1], z.vf[3], z.pf[1]);            fillers<NF, NE>(z, 15); DSREAD(z.kf[3], z.lds, 96);
    }
}

// stamps[wave][4]: s_memtime and s_memrealtime before and after the loop
template <int MODE, int NF, int NE>
__global__ __launch_bounds__(256, 2) void skel(const uint16_t* __restrict__ src, float* __restrict__ sink,
                                               unsigned long long* __restrict__ stamps, int tiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // fill the 2 x 16 KiB ring from the source (random bf16 in [-1, 1))
    for (int i = tid; i < 2048; i += 256) reinterpret_cast<uint4*>(smem)[i] = reinterpret_cast<const uint4*>(src)[i & 1023];
    __syncthreads();
    St z;
    {
        const int row = lane & 31, hh = lane >> 5;
        z.lds = (uint32_t)(row * 128 + ((hh ^ ((row >> 1) & 7)) << 4));   // attn3_kernel's swizzled fragment address
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            z.qf[k] = *reinterpret_cast<const bf16x8*>(smem + 16384 + z.lds + k * 32);
            z.kf[k] = *reinterpret_cast<const bf16x8*>(smem + z.lds + k * 32);
            z.vf[k] = *reinterpret_cast<const bf16x8*>(smem + 8192 + z.lds + k * 32);
        }
        z.pf[0] = *reinterpret_cast<const bf16x8*>(smem + 24576 + z.lds);
        z.pf[1] = *reinterpret_cast<const bf16x8*>(smem + 24576 + z.lds + 32);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            z.negm[r] = -1.f; z.s[0][r] = 0.f; z.s[1][r] = 0.f;
            z.o[0][0][r] = 0.f; z.o[0][1][r] = 0.f; z.o[1][0][r] = 0.f; z.o[1][1][r] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { z.e[0][j] = (f32x2){-1.f - lane * 1e-3f, -2.f}; z.e[1][j] = (f32x2){-1.5f, -0.5f - j}; }
        z.ps[0] = z.ps[1] = (f32x2){0.f, 0.f};
        z.l[0] = z.l[1] = 0.f;
        z.pk[0] = z.pk[1] = 0;
        asm volatile("" : "+v"(z.negm));     // (a known constant would be re-materialised from scalar registers inside the loop)
    }
    uint32_t goff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) goff[i] = (uint32_t)(((wid * 2 + i) * 64 + lane) * 16);   // 8 pieces of 1 KiB per 8 KiB half
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int t = 0; t < tiles; ++t) {
        char* nxt = smem + ((t + 1) & 1) * 16384;
        const char* g = reinterpret_cast<const char*>(src);
#pragma unroll
        for (int i = 0; i < 2; ++i) {     // K piece and V^T piece: 4 LDS-DMA instructions per wave and tile
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + goff[i]),
                                             (__attribute__((address_space(3))) void*)(nxt + (wid * 2 + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + 8192 + goff[i]),
                                             (__attribute__((address_space(3))) void*)(nxt + 8192 + (wid * 2 + i) * 1024), 16, 0, 0);
        }
        block<MODE, NF, NE, 0>(z);
        block<MODE, NF, NE, 1>(z);
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) {
        unsigned long long* st = stamps + ((size_t)blockIdx.x * 4 + wid) * 2;
        st[0] = t1 - t0;
        st[1] = r1 - r0;
    }
    float acc = z.l[0] + z.l[1] + z.ps[0][0] + z.ps[1][1] + __uint_as_float(z.pk[0] ^ z.pk[1]);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc += z.s[0][r] + z.s[1][r] + z.o[0][0][r] + z.o[0][1][r] + z.o[1][0][r] + z.o[1][1][r];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += z.e[0][j][0] + z.e[1][j][1];
    if (acc == 12345.678f) sink[0] = acc;     // (never true: keeps the results alive)
}

struct Res { double ms_per_launch, cyc_per_mfma_simd_wall, ticks_per_mfma_wave, mhz_memtime; };

static uint16_t* d_src; static float* d_sink; static unsigned long long* d_st;
static int g_cus = 256;

template <int MODE, int NF, int NE>
Res run(int wg_per_cu, double seconds, int tiles) {
    auto k = skel<MODE, NF, NE>;
    const int lds = wg_per_cu == 1 ? 96 * 1024 : 64 * 1024;
    CK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    const int nwg = g_cus * wg_per_cu;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k, dim3(nwg), dim3(256), lds, 0, d_src, d_sink, d_st, tiles);   // warm-up
    CK(hipDeviceSynchronize());
    double total_ms = 0; int launches = 0;
    while (total_ms < seconds * 1e3) {
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < 4; ++i) hipLaunchKernelGGL(k, dim3(nwg), dim3(256), lds, 0, d_src, d_sink, d_st, tiles);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        total_ms += ms; launches += 4;
    }
    CK(hipGetLastError());
    std::vector<unsigned long long> h((size_t)nwg * 8);
    CK(hipMemcpy(h.data(), d_st, h.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> ticks, ratio;
    for (size_t w = 0; w < (size_t)nwg * 4; ++w) { ticks.push_back((double)h[2 * w]); ratio.push_back((double)h[2 * w] / (double)h[2 * w + 1]); }
    std::nth_element(ticks.begin(), ticks.begin() + ticks.size() / 2, ticks.end());
    std::nth_element(ratio.begin(), ratio.begin() + ratio.size() / 2, ratio.end());
    const double mfma_per_wave = 32.0 * tiles;
    Res r;
    r.ms_per_launch = total_ms / launches;
    r.ticks_per_mfma_wave = ticks[ticks.size() / 2] / mfma_per_wave;
    r.mhz_memtime = ratio[ratio.size() / 2] * 100.0;    // s_memrealtime counts at 100 MHz
    // wall time per MFMA and SIMD, in s_memtime ticks at the measured tick rate
    r.cyc_per_mfma_simd_wall = r.ms_per_launch * 1e-3 * r.mhz_memtime * 1e6 / (mfma_per_wave * wg_per_cu);
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return r;
}

static void show(const char* name, int wg, const Res& r) {
    printf("%-34s %d wave/SIMD  %8.3f ms/launch  %6.2f ticks/MFMA/SIMD (wall)  %6.2f ticks/MFMA/wave (stamps)  s_memtime %7.1f MHz  matrix duty at 32 ticks %5.1f %%\n",
           name, wg, r.ms_per_launch, r.cyc_per_mfma_simd_wall, r.ticks_per_mfma_wave, r.mhz_memtime, 3200.0 / r.cyc_per_mfma_simd_wall);
    fflush(stdout);
}

template <int NF, int NE>
void sweep_one(int tiles) {
    char name[64];
    snprintf(name, sizeof name, "sweep %d per gap, %d of them exp", NF, NE);
    for (int wg : {1, 2}) show(name, wg, run<3, NF, NE>(wg, 0.25, tiles));
}

int main(int argc, char** argv) {
    const double secs = argc > 1 ? atof(argv[1]) : 1.0;
    const int tiles = 6000;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    g_cus = prop.multiProcessorCount;
    printf("%s, %d CUs, clockRate %d kHz\n", prop.name, g_cus, prop.clockRate);
    std::vector<uint16_t> h(16384);
    uint32_t x = 12345u;
    for (auto& v : h) {     // random bf16 in [-1, 1)
        x = x * 1664525u + 1013904223u;
        const float f = (float)(int)(x >> 8) / 8388608.f - 1.f;
        uint32_t u; memcpy(&u, &f, 4);
        v = (uint16_t)(u >> 16);
    }
    CK(hipMalloc((void**)&d_src, 32768)); CK(hipMalloc((void**)&d_sink, 4)); CK(hipMalloc((void**)&d_st, (size_t)g_cus * 2 * 4 * 2 * 8));
    CK(hipMemcpy(d_src, h.data(), 32768, hipMemcpyHostToDevice));
    for (int rep = 0; rep < 2; ++rep)
        for (int wg : {1, 2}) {     // A / B / (C) / A / B / (C)
            show("clustered", wg, run<0, 0, 0>(wg, secs, tiles));
            show("skewed, packed row sum", wg, run<1, 0, 0>(wg, secs, tiles));
            show("skewed, plain-add row sum", wg, run<2, 0, 0>(wg, secs, tiles));
        }
    sweep_one<0, 0>(tiles);
    sweep_one<1, 0>(tiles); sweep_one<1, 1>(tiles);
    sweep_one<2, 0>(tiles); sweep_one<2, 1>(tiles); sweep_one<2, 2>(tiles);
    sweep_one<3, 0>(tiles); sweep_one<3, 1>(tiles); sweep_one<3, 2>(tiles);
    sweep_one<4, 0>(tiles); sweep_one<4, 1>(tiles); sweep_one<4, 2>(tiles);
    sweep_one<5, 0>(tiles); sweep_one<5, 1>(tiles); sweep_one<5, 2>(tiles);
    sweep_one<6, 0>(tiles); sweep_one<6, 1>(tiles); sweep_one<6, 2>(tiles);
    return 0;
}
