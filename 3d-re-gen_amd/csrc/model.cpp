// model.cpp -- host-side orchestration of the Hunyuan3D-2 shape model on one MI355X (compiled by hipcc).
//
// Mirrors, kernel launch by kernel launch, what the reference obtains from `hy3dgen`
// (src/2d_to_3d_models/run.py:77-84 -> Hunyuan3DDiTFlowMatchingPipeline.__call__):
//   cond_encode  : conditioner.DinoImageEncoder (transformers Dinov2Model) -> cond tokens
//   dit_forward  : denoisers/hunyuan3ddit.py Hunyuan3DDiT.forward
//   flow_sample  : pipelines.py denoising loop (CFG batch 2) + schedulers.FlowMatchEulerDiscreteScheduler.step
//   vae_decode   : autoencoders/model.py ShapeVAE.forward (post_kl + Transformer) + geo-decoder K/V (once)
//   grid_query   : volume_decoders.VanillaVolumeDecoder + attention_blocks.CrossAttentionDecoder
// Weights are registered by their upstream state-dict names; all dimensions come from r3g_model_config.
//
// Token layout (differs from upstream on purpose): softmax attention has no positional term on this
// path, so the joint sequence is stored [latent | cond | pad] (upstream: cat(cond, latent)); latent rows
// start at 0 (tile aligned), cond rows at num_latents, padded keys are masked inside the kernel.
// The residual stream is fp32 in HBM; GEMM operands are bf16; accumulation fp32.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/r3g.h"
#include "geo_narrow.h"
#include "kernels.h"
#include "kvsel_kernels.h"
#include "mesh_kernels.h"
#include "prof.h"
#include "r3g_ctx.h"

namespace r3g {

struct Tensor {
    const void* p;
    int dtype;  // 0 f32, 1 bf16
    int64_t rows, cols;
};

struct Lin {
    const uint16_t* w = nullptr;
    const float* b = nullptr;
    int N = 0, K = 0;
    int64_t ldw = 0;
};

static inline int64_t rup(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// single blocks: MLP-in GEMM on a second stream beside the attention kernel.  Off since the GEMM became a persistent grid of
// one 160 KiB-LDS workgroup per CU: the two kernels can no longer share a CU and take turns (measured 1.4 % slower with it)
static int g_overlap_mlp = 0;
static int g_group_streams = 1;   // img + txt GEMMs of a double block in one launch
static int g_fuse_qkv = 1;    // QKV split + q/k norm + V transpose in the projection's epilogue
static int g_batch_mods = 1;  // one GEMV launch for all modulations of a DiT forward
static int g_geo_fp8 = 0;   // BASELINE.json configs[3]: geo decoder GEMMs on fp8 (e4m3) operands: 0 off (default) | 1 c_q + MLP | 2 MLP only | 3 c_q only
constexpr float kGeoHiddenScale = 1.0f / 16.0f;   // static scale of the fp8 MLP hidden: |GELU| up to 28 representable
static int g_geo_resid_bf16 = 1;   // geo decoder block: 16-bit residual stream (the reference's is fp16)
static int g_cfg_dedup = 1;   // carry the (uniform) unconditional context as one weighted token
static unsigned g_option_epoch = 0;   // bumped by every r3g_set_option: cached intermediate results (Model::GeoCache) are tied to it
static int g_geo_q_cache_gb = -1;   // budget of that cache in GiB (option "geo_q_cache_gb"); < 0: 30 % of the device's memory
static int g_geo_q_cache = 1;   // keep the object-independent query side of the geo decoder resident in HBM (Model::GeoCache)
static int g_dit_f16_guard = 1;    // option "dit_f16_guard": check the latents of an fp16-stream group, fall back to fp32 on overflow
static int g_geo_ln3_fold = 1;    // option "geo_ln3_fold" (round 6): the geo decoder's ln_3 folded into c_proj's epilogue (statistics) and c_fc (W' = W gamma, rstd (acc - mean c1) + c2)
static int g_geo_lnd_fused = 1;   // option "geo_lnd_fused" (round 6): ln_post + output_proj folded into the geo decoder's last residual GEMM
static int g_dit_resid_f16 = 1;   // the DiT's residual stream of the de-duplicated CFG path in fp16 (the reference's activation type) instead of fp32
static int g_skip_zero_step = 1;   // skip the DiT evaluation of a step whose d_sigma is 0 (upstream's last step)
// r3g_flow_sample runs steps [g_flow_first_step, g_flow_last_step) of its schedule (options "flow_first_step" / "flow_last_step";
// default: all of them, a last step of -1 standing for "to the end").  Consecutive segments of one schedule, each continuing on the
// previous one's latents, are the same launches as the whole schedule in one call: tests read the latents after 10, 20, ... of 50 steps this way.
static int g_flow_first_step = 0, g_flow_last_step = -1;
static int flow_last_step(int steps) { return g_flow_last_step < 0 ? steps : std::min(steps, g_flow_last_step); }
// adaptive top-k selection of the geo decoder's cross-attention keys (options "geo_kv_topk" / "geo_kv_group" /
// "geo_kv_stride"): 0 exact (default) | k > 0 keys kept per (group, head), clamped to num_latents | -1 upstream's rule
static int g_geo_kv_topk = 0, g_geo_kv_group = 8192, g_geo_kv_stride = 64;
// narrow geo decoder: option "geo_narrow_fused" -- everything behind the cross-attention of a decoder of width
// 256 in one launch per pass (geo_narrow.hip) instead of the generic five
static int g_geo_narrow_fused = 0;

static const Option g_model_options[] = {
    {"fuse_qkv", &g_fuse_qkv},
    {"batch_mods", &g_batch_mods},
    {"cfg_dedup", &g_cfg_dedup},
    {"skip_zero_step", &g_skip_zero_step},
    {"geo_q_cache", &g_geo_q_cache},
    {"geo_q_cache_gb", &g_geo_q_cache_gb, OPT_ELSE, [](int v) { return v >= 0; }, -1},
    {"geo_resid_bf16", &g_geo_resid_bf16},
    {"dit_resid_f16", &g_dit_resid_f16},
    {"dit_f16_guard", &g_dit_f16_guard},
    {"geo_fp8", &g_geo_fp8, OPT_ELSE, [](int v) { return v >= 0 && v <= 3; }, 0},
    {"group_streams", &g_group_streams},
    {"overlap_mlp", &g_overlap_mlp},
    {"geo_lnd_fused", &g_geo_lnd_fused},
    {"geo_ln3_fold", &g_geo_ln3_fold},
    {"flow_first_step", &g_flow_first_step, OPT_ANY},
    {"flow_last_step", &g_flow_last_step, OPT_ELSE, [](int v) { return v >= 0 && v < (1 << 30); }, -1},
    // the "geo_kv_*" options: nothing cached depends on them, no new epoch
    {"geo_kv_topk", &g_geo_kv_topk, OPT_REFUSE, [](int v) { return v >= -1; }, 0,
     "r3g_set_option: geo_kv_topk is 0 (exact), a key count, or -1 (upstream's rule)", false},
    {"geo_kv_group", &g_geo_kv_group, OPT_REFUSE, [](int v) { return v >= 256 && v % 256 == 0; }, 0,
     "r3g_set_option: geo_kv_group must be a multiple of 256, at least 256", false},
    {"geo_kv_stride", &g_geo_kv_stride, OPT_REFUSE, [](int v) { return v >= 1; }, 0, "r3g_set_option: geo_kv_stride must be at least 1", false},
    {"geo_narrow_fused", &g_geo_narrow_fused, OPT_FLAG, nullptr, 0, nullptr, false},     // behind the cached query side: no new epoch
    // = r3g_set_staging: the GEMMs' and the attention's staging path are set together and read back as 1 while both are LDS-DMA
    {"lds_dma", &g_gemm_glds, OPT_FLAG, nullptr, 0, nullptr, true, &g_attn_glds},
    {}};

// every switch of the library: the rows of the files that own some, in one list
static const std::vector<const Option*>& options() {
    static const std::vector<const Option*> all = [] {
        std::vector<const Option*> v;
        for (const Option* t : {g_model_options, g_gemm_options, g_attn_options, g_ln_options, g_mc_options, g_mesh_options})
            for (; t->name; ++t) v.push_back(t);
        return v;
    }();
    return all;
}

static const Option* find_option(const char* name) {
    for (const Option* o : options())
        if (!strcmp(name, o->name)) return o;
    return nullptr;
}

// the rules of options.h, once each
static int store(const Option* o, const char* name, int value) {
    if (!o) return fail(R3G_ERR_INVALID, "r3g_set_option: unknown option '%s'", name);
    switch (o->rule) {
        case OPT_FLAG: value = value != 0; break;
        case OPT_ANY: break;
        case OPT_KEEP: if (!o->ok(value)) return R3G_OK; break;
        case OPT_ELSE: if (!o->ok(value)) value = o->other; break;
        case OPT_MASK: value &= o->other; break;
        case OPT_REFUSE: if (!o->ok(value)) return fail(R3G_ERR_INVALID, "%s", o->refusal); break;
    }
    *o->slot = value;
    if (o->slot2) *o->slot2 = value;
    return R3G_OK;
}

int option_store(const char* name, int value) { return store(find_option(name), name, value); }

struct Model {
    r3g_model_config c{};
    std::unordered_map<std::string, Tensor> w;
    std::unordered_map<std::string, float> scalars;
    // derived
    int T = 0, Tpad = 0, Lc = 0, Lcpad = 0, H = 0, Hd = 0, W = 0, Wh = 0, Hc = 0, Hch = 0, Fc = 0;
    int cin_pad = 0, qc = 0;
    // the geo decoder's own width and head count: W / Wh unless the checkpoint carries a narrow decoder; read off
    // vae.geo_decoder.query_proj.weight by geo_dims() at the start of every r3g_vae_decode / grid query
    int Wg = 0, Hg = 0;
    DevBuf geo_tail_packed;               // geo_tail_pack_launch's fragment stream (fused tail of a narrow decoder)
    // device buffers (every DevBuf below goes with the model)
    DevBuf arena;
    float* f32a = nullptr;      // residual stream
    uint16_t* xn = nullptr;     // normalised / modulated operand
    uint16_t* qkv = nullptr;    // fused projection output
    uint16_t *Q = nullptr, *K = nullptr, *Vt = nullptr;
    uint16_t* cat = nullptr;    // [attn | mlp hidden] operand of the closing projection
    uint16_t* hid = nullptr;    // wide hidden (VAE / geo / DINO MLP)
    uint16_t* inb = nullptr;    // bf16 copy of small inputs (latents, Fourier features, patches)
    float* small = nullptr;     // temb[B][256] | th[B][H] | vec[B][H] | mods[B][12H] | v2[2][N][Cin] ...
    float *temb = nullptr, *th = nullptr, *vec = nullptr, *mods = nullptr, *v2 = nullptr;
    // guidance-distilled checkpoints: timestep_embedding(g) [256] | guidance_in's hidden [H] | guidance_in(emb(g)) [H], per call
    float *gemb = nullptr, *gth = nullptr, *gvec = nullptr;
    // persistent results
    float* z = nullptr;         // VAE-decoded latents f32 [Nlat][W]
    uint16_t *geoK = nullptr, *geoVt = nullptr;
    bool have_z = false;
    // all adaLN modulation GEMVs of one DiT forward, batched into one launch
    DevBuf mod_jobs;                    // GemvJob [n_mod_jobs]
    int n_mod_jobs = 0;
    DevBuf mod_all;                     // f32 [job][B][N]
    std::vector<int64_t> mod_off;       // per job offset into mod_all
    // second stream: the MLP half of a single block's linear1 runs beside the attention kernel (see dit_forward_grouped, which makes
    // the three on first use: all of them or none)
    Stream aux;
    Event ev_fork, ev_join;
    // fp8 mode of the geo decoder (option geo_fp8): e4m3 copies of its weights with one scale per output row, made on
    // first use; per-row scales of the activations LayerNorm quantises; the constant scale vector of the MLP hidden
    struct W8 { DevBuf w8, sw; };                    // e4m3 [N][K], f32 [N rounded up to 64]
    std::unordered_map<const void*, W8> w8;
    DevBuf fp8_sa, fp8_sconst;                       // f32 [qc] each
    // The folds' buffers are grown to the decoder at hand by size alone: lnf_w, lnf_c and lnd_gw are rewritten by every grid query
    // (the weights may have been re-registered), lnd_part and lnf_stats are written before they are read within a pass.
    DevBuf lnf_w;                                    // ln_3 fold: bf16(c_fc.weight * ln_3.weight) [N][W]
    DevBuf lnf_c, lnf_stats;                         //   f32 c1 | c2 [2 N], (mean, rstd) per row of a pass [qc][2]
    DevBuf lnd_gw, lnd_part;                         // EPI_RESID_BF16_LND: f32 gamma * w [W] + 2 constants, chunk statistics [qc][W / 64][4]
    // activation arena of the grouped DiT engine for `cap_obj` objects and `cap_lat` latent blocks (= attention entries) per
    // launch (allocated on first use), and the segment tables of its fused QKV epilogues for `nb` objects of `epo` entries each
    // (2: classifier-free guidance with the de-duplicated unconditional entry | 1: a guidance-distilled model, no CFG batch)
    struct DitBatch {
        int cap_obj = 0, cap_lat = 0, nb = 0, epo = 0;
        DevBuf base;
        float *f32a = nullptr, *v2 = nullptr, *lat0 = nullptr;   // lat0: the group's initial latents (fp16-stream overflow guard)
        int* bad = nullptr;                                        // device flag of that guard
        uint16_t *xn = nullptr, *Q = nullptr, *K = nullptr, *Vt = nullptr, *cat = nullptr, *inb = nullptr, *ctx = nullptr;
        int *seg_txt = nullptr, *seg_all = nullptr;
        std::vector<int> h_seg_txt, h_seg_all;
    } db;
    // Query-side cache of the geo decoder (option geo_q_cache).  Everything a grid point contributes BEFORE it meets an
    // object's latents -- Fourier features, query_proj (the start of its residual stream), ln_1, c_q, q-norm, the scaled Q rows
    // -- is a function of the point's index and the WEIGHTS only, identical for every object.  With 288 GB of HBM the two
    // results (x0 and Q, bf16, 2 x 34.8 GB at 257^3) stay resident: a pass that has been through once reads them instead of
    // recomputing them (bit-identical by construction; -4 launches and ~36 TFLOP per object).  Built lazily pass by pass;
    // dropped when a weight is (re)registered, the grid changes, or the memory is not there (513^3 would need 557 GB).
    struct GeoCache {
        int R = -1, W = 0;                      // W: the decoder width the rows were laid out for
        double bound = 0.0;
        int64_t passes = 0;
        DevBuf x0;                              // bf16 [passes][qc][W], and behind it ...
        uint16_t* Q = nullptr;                  // ... [passes][qc][W] in the same allocation
        std::vector<char> built;
        unsigned epoch = 0;                     // option epoch the built passes belong to (kernel generations change what Q holds)
        bool refused = false;                   // allocation failed for this (R, bound): do not try again
    } gq;
    // hierarchical volume decoder (r3g_grid_query_hier): the grids of the levels below the finest, the active list of the level
    // being built and its logits; grown on demand, released with the model
    DevBuf hier_grids, hier_idx, hier_val;
    // top-k KV selection (kvsel_kernels.h), grown on demand: the grouped Q of a pass, the compact K / V^T and the index table of its
    // (group, head) pairs, and the row-major copy of the object's V (made by the first top-k pass after r3g_vae_decode)
    DevBuf kv_q, kv_k, kv_vt, kv_idx, kv_v;
    bool kv_v_valid = false;
    int kv_last_groups = 0, kv_last_k = 0;      // shape of the table the last top-k pass left in kv_idx (0: none yet)
    const uint16_t* kv_last_q = nullptr;        // ... and the Q rows it was made from: [H][kv_last_npad][64], kv_last_n of them valid
    int kv_last_n = 0, kv_last_npad = 0;
    std::string err;

    const Tensor* find(const std::string& name) const {
        auto it = w.find(name);
        return it == w.end() ? nullptr : &it->second;
    }
};

static std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

#define R3G_TRY(expr)                                          \
    do {                                                       \
        hipError_t e__ = (expr);                               \
        if (e__ != hipSuccess) return hip_fail(e__, #expr);    \
    } while (0)
#define R3G_RC(expr)                \
    do {                            \
        int rc__ = (expr);          \
        if (rc__) return rc__;      \
    } while (0)

// ---- weight lookup ---------------------------------------------------------------------------------
static int get_lin(const Model& m, const std::string& base, bool need_bias, Lin* out) {
    const Tensor* w = m.find(base + ".weight");
    if (!w || w->dtype != 1) return fail(R3G_ERR_STATE, "missing bf16 weight '%s.weight'", base.c_str());
    out->w = (const uint16_t*)w->p;
    out->N = (int)w->rows;
    out->K = (int)w->cols;
    out->ldw = w->cols;
    if (out->K % 64) return fail(R3G_ERR_INVALID, "'%s.weight' K=%d is not padded to a multiple of 64", base.c_str(), out->K);
    const Tensor* b = m.find(base + ".bias");
    out->b = b ? (const float*)b->p : nullptr;
    if (b && b->dtype != 0) return fail(R3G_ERR_INVALID, "'%s.bias' must be f32", base.c_str());
    if (need_bias && !b) return fail(R3G_ERR_STATE, "missing '%s.bias'", base.c_str());
    return R3G_OK;
}

static int get_vec(const Model& m, const std::string& name, int64_t n, const float** out) {
    const Tensor* t = m.find(name);
    if (!t || t->dtype != 0) return fail(R3G_ERR_STATE, "missing f32 tensor '%s'", name.c_str());
    if (n > 0 && t->rows * t->cols != n) return fail(R3G_ERR_INVALID, "'%s' has %lld elements, expected %lld", name.c_str(),
                                                     (long long)(t->rows * t->cols), (long long)n);
    *out = (const float*)t->p;
    return R3G_OK;
}

// ---- thin launch helpers -----------------------------------------------------------------------------
static GemmArgs gemm_args(const uint16_t* A, int64_t lda, int64_t strideA, const Lin& l, int n_off, int N, void* C,
                          int64_t ldc, int64_t strideC, int M, int K, int epi, const float* gate, int64_t strideGate) {
    GemmArgs p{};
    p.A = A; p.lda = lda; p.strideA = strideA;
    p.W = l.w + (int64_t)n_off * l.ldw; p.ldw = l.ldw;
    p.bias = l.b ? l.b + n_off : nullptr;
    p.C = C; p.ldc = ldc; p.strideC = strideC;
    p.gate = gate; p.strideGate = strideGate;
    p.M = M; p.N = N; p.K = K; p.epi = epi;
    return p;
}

// the same layer of the two streams of a double block: one launch (or two, with group_streams = 0)
static int gemm_pair(const GemmArgs& a, int batch_a, const GemmArgs& b, int batch_b, hipStream_t s) {
    hipError_t e;
    if (g_group_streams) {
        e = gemm_launch2(a, batch_a, &b, batch_b, s);
    } else {
        e = gemm_launch(a, batch_a, s);
        if (e == hipSuccess) e = gemm_launch(b, batch_b, s);
    }
    if (e != hipSuccess) return hip_fail(e, "gemm_launch(pair)");
    return R3G_OK;
}

static int gemm(const uint16_t* A, int64_t lda, int64_t strideA, const Lin& l, int n_off, int N, void* C, int64_t ldc,
                int64_t strideC, int M, int K, int epi, const float* gate, int64_t strideGate, int batch, hipStream_t s) {
    if (K > l.K) return fail(R3G_ERR_INVALID, "gemm: K=%d exceeds weight K=%d", K, l.K);
    const GemmArgs p = gemm_args(A, lda, strideA, l, n_off, N, C, ldc, strideC, M, K, epi, gate, strideGate);
    hipError_t e = gemm_launch(p, batch, s);
    if (e != hipSuccess) return hip_fail(e, "gemm_launch");
    return R3G_OK;
}

// projection whose output goes straight to the attention operand layout (EPI_QKV), or the unfused pair
static int gemm_qkv(Model& m, const uint16_t* A, int64_t lda, int64_t strideA, const Lin& l, int n_off, int N, int M,
                    int K, int batch, const QkvSplitArgs& q, int layout, hipStream_t s) {
    if (g_fuse_qkv) {
        GemmArgs p{};
        p.A = A; p.lda = lda; p.strideA = strideA;
        p.W = l.w + (int64_t)n_off * l.ldw; p.ldw = l.ldw;
        p.bias = l.b ? l.b + n_off : nullptr;
        p.M = M; p.N = N; p.K = K; p.epi = EPI_QKV;
        p.qkv.Q = q.Q; p.qkv.K = q.K; p.qkv.Vt = q.Vt; p.qkv.Lq_pad = q.Lq_pad; p.qkv.Lk_pad = q.Lk_pad;
        p.qkv.dst_row0 = q.dst_row0; p.qkv.heads = q.H; p.qkv.layout = layout; p.qkv.norm = q.norm;
        p.qkv.qw = q.qw; p.qkv.qb = q.qb; p.qkv.kw = q.kw; p.qkv.kb = q.kb; p.qkv.eps = q.eps;
        p.qkv.q_scale = q.q_scale;
        hipError_t e = gemm_launch(p, batch, s);
        if (e != hipSuccess) return hip_fail(e, "gemm_launch(qkv)");
        return R3G_OK;
    }
    int rc = gemm(A, lda, strideA, l, n_off, N, const_cast<uint16_t*>(q.src), q.ld, q.src_batch_stride, M, K, EPI_BF16,
                  nullptr, 0, batch, s);
    if (rc) return rc;
    hipError_t e = qkv_split_launch(q, s);
    if (e != hipSuccess) return hip_fail(e, "qkv_split_launch");
    return R3G_OK;
}

static int layernorm(const float* x, int64_t ldx, int64_t xbs, uint16_t* y, int64_t ldy, int64_t ybs, int rows_per_batch,
                     int batch, int C, const float* w, const float* b, const float* scale, const float* shift,
                     int64_t mod_stride, float eps, hipStream_t s, int x_bf16 = 0) {
    LnArgs p{};
    p.x = x; p.ldx = ldx; p.x_batch_stride = xbs; p.x_bf16 = x_bf16;
    p.y = y; p.ldy = ldy; p.y_batch_stride = ybs;
    p.w = w; p.b = b; p.scale = scale; p.shift = shift; p.mod_stride = mod_stride;
    p.rows = rows_per_batch * batch; p.C = C; p.rows_per_batch = rows_per_batch; p.eps = eps;
    hipError_t e = layernorm_launch(p, s);
    if (e != hipSuccess) return hip_fail(e, "layernorm_launch");
    return R3G_OK;
}

static int attention(const Model& m, int B, int heads, int Lq, int Lq_pad, int Lk, int Lk_pad, uint16_t* O, int64_t ldo,
                     int64_t strideO, const uint16_t* Kp, const uint16_t* Vtp, bool shared_kv, hipStream_t s,
                     const uint16_t* Qp = nullptr) {
    AttnArgs p{};
    p.Q = Qp ? Qp : m.Q; p.K = Kp; p.Vt = Vtp; p.O = O; p.ldo = ldo; p.strideO = strideO;
    p.B = B; p.H = heads; p.Lq = Lq; p.Lq_pad = Lq_pad; p.Lk = Lk; p.Lk_pad = Lk_pad;
    p.kv_batch_stride_zero = shared_kv ? 1 : 0;
    p.scale = 0.125f;
    p.q_prescaled = attn_q_scale(0.125f) != 1.0f;
    hipError_t e = attention_launch(p, s);
    if (e != hipSuccess) return hip_fail(e, "attention_launch");
    return R3G_OK;
}

// ---- DiT -------------------------------------------------------------------------------------------
// Modulation.forward: lin(silu(vec)) -> dst f32 [B][mult*H]
static int dit_modulation(Model& m, const std::string& base, int B, int mult, float* dst, hipStream_t s) {
    Lin l;
    R3G_RC(get_lin(m, base, true, &l));
    if (l.N != mult * m.H) return fail(R3G_ERR_INVALID, "'%s' has N=%d, expected %d", base.c_str(), l.N, mult * m.H);
    R3G_TRY(gemv_launch(m.vec, B, m.H, l.w, l.ldw, l.b, dst, l.N, 1, 0, s));
    return R3G_OK;
}

// One-time table of every modulation layer (double img/txt, single, final) for gemv_multi_launch.
static int build_mod_jobs(Model& m) {
    if (m.mod_jobs) return R3G_OK;
    const r3g_model_config& c = m.c;
    std::vector<GemvJob> jobs;
    m.mod_off.clear();
    int64_t off = 0;
    auto add = [&](const std::string& base, int mult) -> int {
        Lin l;
        int rc = get_lin(m, base, true, &l);
        if (rc) return rc;
        if (l.N != mult * m.H) return fail(R3G_ERR_INVALID, "'%s' has N=%d, expected %d", base.c_str(), l.N, mult * m.H);
        // gemv_multi_kernel reads 16 bytes of w per lane; the table lives on the device, where gemv_multi_launch cannot look
        if ((l.ldw & 7) || (reinterpret_cast<uintptr_t>(l.w) & 15))
            return fail(R3G_ERR_INVALID, "'%s': the modulation GEMV needs ldw %% 8 == 0 and a 16-byte aligned matrix", base.c_str());
        jobs.push_back(GemvJob{l.w, l.b, l.ldw, l.N, off});
        m.mod_off.push_back(off);
        off += 2LL * l.N;  // [B<=2][N]
        return R3G_OK;
    };
    for (int i = 0; i < c.dit_depth_double; ++i) {
        R3G_RC(add(fmt("model.double_blocks.%d.img_mod.lin", i), 6));
        R3G_RC(add(fmt("model.double_blocks.%d.txt_mod.lin", i), 6));
    }
    for (int i = 0; i < c.dit_depth_single; ++i) R3G_RC(add(fmt("model.single_blocks.%d.modulation.lin", i), 3));
    R3G_RC(add("model.final_layer.adaLN_modulation.1", 2));
    R3G_RC(m.mod_all.grow((size_t)off * sizeof(float), nullptr, "modulation outputs"));
    R3G_RC(m.mod_jobs.grow(jobs.size() * sizeof(GemvJob), nullptr, "modulation jobs"));      // (last: its presence marks the table as built)
    R3G_TRY(hipMemcpy(m.mod_jobs.p, jobs.data(), jobs.size() * sizeof(GemvJob), hipMemcpyHostToDevice));
    m.n_mod_jobs = (int)jobs.size();
    return R3G_OK;
}

// The joint sequence keeps the cond rows behind the latent rows: the DiT needs num_latents tile aligned.  (The VAE and the geo
// decoder do not -- their padded keys are masked -- so the model itself is created for any count.)
static int dit_latents_aligned(const Model& m) {
    if (m.c.vae_num_latents % 64) return fail(R3G_ERR_INVALID, "the DiT needs num_latents to be a multiple of 64 (got %d)", m.c.vae_num_latents);
    return R3G_OK;
}

static int dit_forward(Model& m, const float* x_in, const float* t_dev, float t_scalar, const uint16_t* cond, float* out,
                       int B, int n_double, int n_single, hipStream_t s) {
    const r3g_model_config& c = m.c;
    const int H = m.H, Nl = c.vae_num_latents, Lc = m.Lc, T = m.T, Tpad = m.Tpad, heads = m.Hd;
    const int64_t xs = (int64_t)Tpad * H;  // batch stride of the residual stream
    if (B < 1 || B > 2) return fail(R3G_ERR_INVALID, "dit_forward: batch %d not in [1,2]", B);
    R3G_RC(dit_latents_aligned(m));
    Lin l;
    // latent_in / cond_in -> joint residual stream [latent | cond]
    R3G_TRY(cast_pad_launch(x_in, c.dit_in_channels, m.inb, m.cin_pad, B * Nl, c.dit_in_channels, m.cin_pad, 1.0f, s));
    R3G_RC(get_lin(m, "model.latent_in", true, &l));
    R3G_RC(gemm(m.inb, m.cin_pad, (int64_t)Nl * m.cin_pad, l, 0, H, m.f32a, H, xs, Nl, m.cin_pad, EPI_F32, nullptr, 0, B, s));
    R3G_RC(get_lin(m, "model.cond_in", true, &l));
    R3G_RC(gemm(cond, c.dit_context_dim, (int64_t)Lc * c.dit_context_dim, l, 0, H, m.f32a + (int64_t)Nl * H, H, xs, Lc,
                c.dit_context_dim, EPI_F32, nullptr, 0, B, s));
    // vec = time_in(timestep_embedding(t))
    R3G_TRY(timestep_embedding_launch(t_dev, t_scalar, B, c.dit_time_factor, m.temb, s));
    R3G_RC(get_lin(m, "model.time_in.in_layer", true, &l));
    R3G_TRY(gemv_launch(m.temb, B, 256, l.w, l.ldw, l.b, m.th, H, 0, 1, s));
    R3G_RC(get_lin(m, "model.time_in.out_layer", true, &l));
    R3G_TRY(gemv_launch(m.th, B, H, l.w, l.ldw, l.b, m.vec, H, 0, 0, s));

    if (g_batch_mods) {
        R3G_RC(build_mod_jobs(m));
        R3G_TRY(gemv_multi_launch(m.vec, B, H, m.mod_jobs.as<GemvJob>(), m.n_mod_jobs, m.mod_all.as<float>(), 1, s));
    }
    const int nd = n_double < 0 ? c.dit_depth_double : n_double;
    const int ns = n_single < 0 ? c.dit_depth_single : n_single;
    const int64_t catld = 5 * (int64_t)H, cats = (int64_t)Tpad * catld;
    const int64_t qkvld = 3 * (int64_t)H, qkvs = (int64_t)Tpad * qkvld;
    const int mh = c.dit_mlp_hidden;
    if (mh != 4 * H) return fail(R3G_ERR_INVALID, "dit mlp_hidden must be 4*hidden");

    for (int i = 0; i < nd; ++i) {
        // stream 0 = img (latent rows [0,Nl)), stream 1 = txt (cond rows [Nl, Nl+Lc))
        for (int st = 0; st < 2; ++st) {
            const char* nm = st == 0 ? "img" : "txt";
            const int row0 = st == 0 ? 0 : Nl, rows = st == 0 ? Nl : Lc;
            const std::string blk = fmt("model.double_blocks.%d.%s", i, nm);
            // mods: [stream][B][6H] = shift1 scale1 gate1 shift2 scale2 gate2
            float* mm = m.mods + (int64_t)st * 2 * 6 * H;
            if (g_batch_mods) mm = m.mod_all.as<float>() + m.mod_off[2 * i + st];
            else R3G_RC(dit_modulation(m, blk + "_mod.lin", B, 6, mm, s));
            R3G_RC(layernorm(m.f32a + (int64_t)row0 * H, H, xs, m.xn + (int64_t)row0 * H, H, xs, rows, B, H, nullptr, nullptr,
                             mm + H, mm, 6 * H, 1e-6f, s));
            R3G_RC(get_lin(m, blk + "_attn.qkv", c.dit_qkv_bias != 0, &l));
            QkvSplitArgs q{};
            q.src = m.qkv + (int64_t)row0 * qkvld; q.ld = qkvld; q.src_batch_stride = qkvs;
            q.q_off = 0; q.k_off = H; q.v_off = 2 * H; q.head_stride = 64;
            q.Q = m.Q; q.K = m.K; q.Vt = m.Vt; q.Lq_pad = Tpad; q.Lk_pad = Tpad; q.dst_row0 = row0;
            q.B = B; q.H = heads; q.L = rows; q.norm = QKN_RMS; q.eps = 1e-6f; q.q_scale = attn_q_scale(0.125f);
            R3G_RC(get_vec(m, blk + "_attn.norm.query_norm.scale", 64, &q.qw));
            R3G_RC(get_vec(m, blk + "_attn.norm.key_norm.scale", 64, &q.kw));
            R3G_RC(gemm_qkv(m, m.xn + (int64_t)row0 * H, H, xs, l, 0, 3 * H, rows, H, B, q, QKV_KHD, s));
        }
        R3G_RC(attention(m, B, heads, T, Tpad, T, Tpad, m.cat, catld, cats, m.K, m.Vt, false, s));
        for (int st = 0; st < 2; ++st) {
            const char* nm = st == 0 ? "img" : "txt";
            const int row0 = st == 0 ? 0 : Nl, rows = st == 0 ? Nl : Lc;
            const std::string blk = fmt("model.double_blocks.%d.%s", i, nm);
            float* mm = g_batch_mods ? m.mod_all.as<float>() + m.mod_off[2 * i + st] : m.mods + (st == 0 ? 0 : (int64_t)2 * 6 * H);
            float* xr = m.f32a + (int64_t)row0 * H;
            R3G_RC(get_lin(m, blk + "_attn.proj", true, &l));
            R3G_RC(gemm(m.cat + (int64_t)row0 * catld, catld, cats, l, 0, H, xr, H, xs, rows, H, EPI_RESID_F32, mm + 2 * H,
                        6 * H, B, s));
            R3G_RC(layernorm(xr, H, xs, m.xn + (int64_t)row0 * H, H, xs, rows, B, H, nullptr, nullptr, mm + 4 * H, mm + 3 * H,
                             6 * H, 1e-6f, s));
            R3G_RC(get_lin(m, blk + "_mlp.0", true, &l));
            R3G_RC(gemm(m.xn + (int64_t)row0 * H, H, xs, l, 0, mh, m.cat + (int64_t)row0 * catld + H, catld, cats, rows, H,
                        EPI_BF16_GELU_TANH, nullptr, 0, B, s));
            R3G_RC(get_lin(m, blk + "_mlp.2", true, &l));
            R3G_RC(gemm(m.cat + (int64_t)row0 * catld + H, catld, cats, l, 0, H, xr, H, xs, rows, mh, EPI_RESID_F32,
                        mm + 5 * H, 6 * H, B, s));
        }
    }
    for (int i = 0; i < ns; ++i) {
        const std::string blk = fmt("model.single_blocks.%d", i);
        float* mm = m.mods;  // [B][3H]: shift scale gate
        if (g_batch_mods) mm = m.mod_all.as<float>() + m.mod_off[2 * c.dit_depth_double + i];
        else R3G_RC(dit_modulation(m, blk + ".modulation.lin", B, 3, mm, s));
        R3G_RC(layernorm(m.f32a, H, xs, m.xn, H, xs, T, B, H, nullptr, nullptr, mm + H, mm, 3 * H, 1e-6f, s));
        R3G_RC(get_lin(m, blk + ".linear1", true, &l));
        if (l.N != 3 * H + mh) return fail(R3G_ERR_INVALID, "linear1 N mismatch");
        R3G_RC(gemm(m.xn, H, xs, l, 3 * H, mh, m.cat + H, catld, cats, T, H, EPI_BF16_GELU_TANH, nullptr, 0, B, s));
        QkvSplitArgs q{};
        q.src = m.qkv; q.ld = qkvld; q.src_batch_stride = qkvs;
        q.q_off = 0; q.k_off = H; q.v_off = 2 * H; q.head_stride = 64;
        q.Q = m.Q; q.K = m.K; q.Vt = m.Vt; q.Lq_pad = Tpad; q.Lk_pad = Tpad; q.dst_row0 = 0;
        q.B = B; q.H = heads; q.L = T; q.norm = QKN_RMS; q.eps = 1e-6f; q.q_scale = attn_q_scale(0.125f);
        R3G_RC(get_vec(m, blk + ".norm.query_norm.scale", 64, &q.qw));
        R3G_RC(get_vec(m, blk + ".norm.key_norm.scale", 64, &q.kw));
        R3G_RC(gemm_qkv(m, m.xn, H, xs, l, 0, 3 * H, T, H, B, q, QKV_KHD, s));
        R3G_RC(attention(m, B, heads, T, Tpad, T, Tpad, m.cat, catld, cats, m.K, m.Vt, false, s));
        R3G_RC(get_lin(m, blk + ".linear2", true, &l));
        R3G_RC(gemm(m.cat, catld, cats, l, 0, H, m.f32a, H, xs, T, H + mh, EPI_RESID_F32, mm + 2 * H, 3 * H, B, s));
    }
    // final layer on the latent rows
    float* fm = m.mods;
    if (g_batch_mods) {
        fm = m.mod_all.as<float>() + m.mod_off[2 * c.dit_depth_double + c.dit_depth_single];
    } else {
        R3G_RC(get_lin(m, "model.final_layer.adaLN_modulation.1", true, &l));
        R3G_TRY(gemv_launch(m.vec, B, H, l.w, l.ldw, l.b, fm, 2 * H, 1, 0, s));
    }
    R3G_RC(layernorm(m.f32a, H, xs, m.xn, H, xs, Nl, B, H, nullptr, nullptr, fm + H, fm, 2 * H, 1e-6f, s));
    R3G_RC(get_lin(m, "model.final_layer.linear", true, &l));
    R3G_RC(gemm(m.xn, H, xs, l, 0, c.dit_in_channels, out, c.dit_in_channels, (int64_t)Nl * c.dit_in_channels, Nl, H, EPI_F32,
                nullptr, 0, B, s));
    return R3G_OK;
}

// ---- the grouped DiT engine: NB objects at once, under classifier-free guidance with a de-duplicated unconditional context
// ---- (2 entries per object, described first) or, for a guidance-distilled model, without the CFG batch (1 entry per object) ----
// The unconditional context is `zeros_like(cond)` (upstream conditioner.unconditional_embedding): after cond_in its
// Lc tokens are identical, and every layer keeps them identical (same input, same per-token ops, same attention
// row).  They are therefore carried as ONE token whose key counts Lc times in the softmax (score + log2(Lc) in the
// log2 domain) -- exactly the same function, 3073 instead of 4442 tokens for that batch entry.
// Objects are independent and share the timestep (hence modulation and gates), so NB of them go through every layer in ONE
// launch (upstream: the pipeline's batch dimension when `image` is a list; the reference's object-level parallelism is the
// pool at src/2d_to_3d_models/run.py:176-193).  A GEMM row does not know which object it belongs to: per-object results are
// bit-identical to NB = 1.  Global row layout of all row-indexed buffers (CFG entry e = 2*object + {0 cond, 1 uncond}):
//   [e*Nl, (e+1)*Nl)  latent rows of entry e          (2*NB blocks, E*NB in general; the img stream of the double blocks)
//   TX0 = 2*NB*Nl;  [TX0 + o*Ltp, +Lc) cond tokens of object o | row TX0 + o*Ltp + Lc: its unconditional token | pad to Ltp
// (Ltp = dit_txt_rows(): Lc + 1 rounded up to whole 16-token groups of V^T, at least 128).  The txt-stream GEMMs see NB*Ltp contiguous rows, the
// single blocks all Rall = TX0 + NB*Ltp rows.
static constexpr int kMaxObjects = kAttnMaxEntries / 2;
// Guidance-distilled checkpoints (model.guidance_in.*: the guidance scale is an embedded input, upstream's "fast" / "turbo"
// subfolders) run WITHOUT the CFG batch: one entry per object, no unconditional token.  The same engine carries them with
// E = 1 entries per object instead of 2 -- E*NB latent blocks, TX0 = E*NB*Nl, per object Lc cond tokens padded to Ltp, E*NB
// ragged attention entries of lq = lk = T without a weighted key -- and a launch group then takes kAttnMaxEntries objects.
static constexpr int kMaxObjectsDistilled = kAttnMaxEntries;
// rows per object in the txt block: Lc cond tokens + 1 unconditional token, padded so that 16-token groups of V^T stay whole
// and (>= 128) no 128-row window of a GEMM meets more than three row segments (QkvEpi::seg_tab)
static int dit_txt_rows(const Model& m) { return (int)std::max<int64_t>(128, rup(m.Lc + 1, 16)); }

static const char* const kGuidanceKeys[4] = {"model.guidance_in.in_layer.weight", "model.guidance_in.in_layer.bias",
                                             "model.guidance_in.out_layer.weight", "model.guidance_in.out_layer.bias"};
// A model is guidance-distilled if and only if the four model.guidance_in.* tensors are registered; a partial set is an error
// that names the first missing key.
static int model_distilled(const Model& m, bool* distilled) {
    int have = 0;
    const char* missing = nullptr;
    for (const char* k : kGuidanceKeys) {
        if (m.find(k)) ++have;
        else if (!missing) missing = k;
    }
    *distilled = have == 4;
    if (have != 0 && have != 4)
        return fail(R3G_ERR_STATE, "guidance-distilled checkpoint is incomplete: missing '%s' (all four model.guidance_in.* tensors or none)",
                    missing);
    return R3G_OK;
}

// E = entries per object: 2 (CFG: conditional + de-duplicated unconditional) or 1 (guidance-distilled)
static int ensure_dit_batch(Model& m, int NB, int E) {
    Model::DitBatch& d = m.db;
    const r3g_model_config& c = m.c;
    const int H = m.H, Nl = c.vae_num_latents, Lc = m.Lc;
    const int Ltp = dit_txt_rows(m);
    if (d.cap_obj < NB || d.cap_lat < E * NB) {
        // the whole device, not a stream: m.aux, the second stream of dit_forward_grouped, works in this arena too
        if (d.base) R3G_TRY(hipDeviceSynchronize());
        d.base.release();
        const int co = std::max(d.cap_obj, NB), cl = std::max(d.cap_lat, E * NB);
        d.cap_obj = d.cap_lat = 0;
        const int64_t rows = rup((int64_t)cl * Nl + (int64_t)co * Ltp, 256);
        const int64_t n_attn = (int64_t)cl * m.Hd * m.Tpad * 64;
        size_t off = 0;
        auto carve = [&](int64_t bytes) { size_t o = off; off += (size_t)rup(bytes, 256); return o; };
        const size_t o_f = carve(rows * H * 4), o_xn = carve(rows * H * 2), o_q = carve(n_attn * 2), o_k = carve(n_attn * 2),
                     o_v = carve(n_attn * 2), o_cat = carve(rows * 5 * H * 2), o_inb = carve((int64_t)co * Nl * m.cin_pad * 2),
                     o_ctx = carve((int64_t)co * Ltp * c.dit_context_dim * 2), o_v2 = carve((int64_t)cl * Nl * c.dit_in_channels * 4),
                     o_seg = carve(2 * 64 * 16), o_lat0 = carve((int64_t)co * Nl * c.dit_in_channels * 4), o_bad = carve(256);
        R3G_RC(d.base.grow(off, nullptr, "dit batch arena"));
        const hipError_t e = hipMemset(d.base.p, 0, off);   // padded rows / columns must start finite
        if (e != hipSuccess) {
            d.base.release();      // (capacities are 0: the next call starts over)
            return hip_fail(e, "hipMemset(dit batch arena)");
        }
        char* a = d.base.p;
        d.f32a = (float*)(a + o_f); d.xn = (uint16_t*)(a + o_xn); d.Q = (uint16_t*)(a + o_q); d.K = (uint16_t*)(a + o_k);
        d.Vt = (uint16_t*)(a + o_v); d.cat = (uint16_t*)(a + o_cat); d.inb = (uint16_t*)(a + o_inb);
        d.ctx = (uint16_t*)(a + o_ctx); d.v2 = (float*)(a + o_v2); d.seg_txt = (int*)(a + o_seg); d.seg_all = d.seg_txt + 64 * 4;
        d.lat0 = (float*)(a + o_lat0); d.bad = (int*)(a + o_bad);
        d.cap_obj = co; d.cap_lat = cl;
        d.nb = 0; d.epo = 0;
    }
    if (d.nb != NB || d.epo != E) {
        // segment tables of the EPI_QKV epilogue: {first row, end row, attention batch slot, destination row}
        const int TX0 = E * NB * Nl;
        d.h_seg_txt.clear(); d.h_seg_all.clear();
        for (int e = 0; e < E * NB; ++e) { const int v[4] = {e * Nl, (e + 1) * Nl, e, 0}; d.h_seg_all.insert(d.h_seg_all.end(), v, v + 4); }
        for (int o = 0; o < NB; ++o) {
            const int c0[4] = {o * Ltp, o * Ltp + Lc, E * o, Nl};
            const int c1[4] = {TX0 + c0[0], TX0 + c0[1], c0[2], c0[3]};
            d.h_seg_txt.insert(d.h_seg_txt.end(), c0, c0 + 4);
            d.h_seg_all.insert(d.h_seg_all.end(), c1, c1 + 4);
            if (E == 2) {   // CFG: the object's single unconditional token, attention slot 2o + 1
                const int u0[4] = {o * Ltp + Lc, o * Ltp + Lc + 1, 2 * o + 1, Nl};
                const int u1[4] = {TX0 + u0[0], TX0 + u0[1], u0[2], u0[3]};
                d.h_seg_txt.insert(d.h_seg_txt.end(), u0, u0 + 4);
                d.h_seg_all.insert(d.h_seg_all.end(), u1, u1 + 4);
            }
        }
        R3G_TRY(hipDeviceSynchronize());   // a previous launch may still read the tables
        R3G_TRY(hipMemcpy(d.seg_txt, d.h_seg_txt.data(), d.h_seg_txt.size() * 4, hipMemcpyHostToDevice));
        R3G_TRY(hipMemcpy(d.seg_all, d.h_seg_all.data(), d.h_seg_all.size() * 4, hipMemcpyHostToDevice));
        d.nb = NB; d.epo = E;
    }
    return R3G_OK;
}

// x_lat f32 [NB][Nl][Cin]; the context rows (m.db.ctx) are filled by the caller; out2 f32 [E*NB][Nl][Cin] (entry order).
// E = m.db.epo entries per object.  gvec (E == 1 only): guidance_in(timestep_embedding(g)) [H], added to vec.
static int dit_forward_grouped(Model& m, const float* x_lat, float t_scalar, float* out2, int NB, hipStream_t s,
                                 bool allow_f16 = true, const float* gvec = nullptr) {
    const r3g_model_config& c = m.c;
    Model::DitBatch& d = m.db;
    const int E = d.epo;
    const int H = m.H, Nl = c.vae_num_latents, Lc = m.Lc, T = m.T, Tpad = m.Tpad, heads = m.Hd;
    const int Ltp = dit_txt_rows(m), TX0 = E * NB * Nl, Mtxt = NB * Ltp, Rall = TX0 + Mtxt;
    const int64_t catld = 5 * (int64_t)H;
    const int mh = c.dit_mlp_hidden;
    if (d.nb != NB || (E != 1 && E != 2)) return fail(R3G_ERR_STATE, "dit batch arena not prepared for %d objects", NB);
    counter_add(LC_DIT_EVALS);
    // The residual stream: fp32, or (option "dit_resid_f16") fp16 -- the reference's own activation type (its pipelines run in
    // fp16) -- in the same buffer: the read-modify-write epilogues of the N = 1024 projections and the LayerNorm reads move
    // half the bytes.  `xrow(r)` = the stream from row r on, in either format.
    const bool xh = g_dit_resid_f16 && allow_f16 && H % 256 == 0;     // (the 16-bit LayerNorm input exists for whole 256-column rows: not CI dims)
    const int xfmt = xh ? 2 : 0, epi_res = xh ? EPI_RESID_F16 : EPI_RESID_F32;
    auto xrow = [&](int64_t r) -> void* {
        return xh ? (void*)(reinterpret_cast<uint16_t*>(d.f32a) + r * H) : (void*)(d.f32a + r * H);
    };
    Lin l;
    // inputs: every object's latents feed both of its CFG entries; cond rows + the single unconditional row per object
    R3G_TRY(cast_pad_launch(x_lat, c.dit_in_channels, d.inb, m.cin_pad, NB * Nl, c.dit_in_channels, m.cin_pad, 1.0f, s));
    R3G_RC(get_lin(m, "model.latent_in", true, &l));
    // (fp16 stream: the stream starts as zeros and the two input projections ADD to it -- 0 + (acc + bias), rounded once)
    if (xh) R3G_TRY(hipMemsetAsync(d.f32a, 0, (size_t)Rall * H * 2, s));
    const int epi_in = xh ? EPI_RESID_F16 : EPI_F32;
    for (int j = 0; j < E; ++j)
        R3G_RC(gemm(d.inb, m.cin_pad, (int64_t)Nl * m.cin_pad, l, 0, H, xrow((int64_t)j * Nl), H, (int64_t)E * Nl * H, Nl, m.cin_pad,
                    epi_in, nullptr, 0, NB, s));
    R3G_RC(get_lin(m, "model.cond_in", true, &l));
    R3G_RC(gemm(d.ctx, c.dit_context_dim, 0, l, 0, H, xrow(TX0), H, 0, Mtxt, c.dit_context_dim, epi_in, nullptr, 0, 1, s));
    R3G_TRY(timestep_embedding_launch(nullptr, t_scalar, 1, c.dit_time_factor, m.temb, s));
    R3G_RC(get_lin(m, "model.time_in.in_layer", true, &l));
    R3G_TRY(gemv_launch(m.temb, 1, 256, l.w, l.ldw, l.b, m.th, H, 0, 1, s));
    R3G_RC(get_lin(m, "model.time_in.out_layer", true, &l));
    R3G_TRY(gemv_launch(m.th, 1, H, l.w, l.ldw, l.b, m.vec, H, 0, 0, s));
    if (gvec) R3G_TRY(vec_add_launch(m.vec, gvec, H, s));   // vec = time_in(emb(t)) + guidance_in(emb(g))
    R3G_RC(build_mod_jobs(m));
    R3G_TRY(gemv_multi_launch(m.vec, 1, H, m.mod_jobs.as<GemvJob>(), m.n_mod_jobs, m.mod_all.as<float>(), 1, s));

    AttnArgs at{};
    at.Q = d.Q; at.K = d.K; at.Vt = d.Vt; at.O = d.cat; at.ldo = catld; at.strideO = 0;
    at.B = E * NB; at.H = heads; at.Lq = T; at.Lq_pad = Tpad; at.Lk = T; at.Lk_pad = Tpad; at.scale = 0.125f;
    at.q_prescaled = attn_q_scale(0.125f) != 1.0f;
    at.ragged = 1;
    for (int o = 0; o < NB; ++o) {   // work order: the long (conditional) entries first
        AttnEntry& ec = at.ent[o];
        ec.lq = T; ec.lk = T; ec.buf = E * o; ec.o_row0 = (int64_t)(E * o) * Nl; ec.o_split = Nl;
        ec.o_row_split = (int64_t)TX0 + (int64_t)o * Ltp; ec.bias_key = -1; ec.bias_log2 = 0.f;
        if (E == 1) continue;
        AttnEntry& eu = at.ent[NB + o];
        eu.lq = Nl + 1; eu.lk = Nl + 1; eu.buf = 2 * o + 1; eu.o_row0 = (int64_t)(2 * o + 1) * Nl; eu.o_split = Nl;
        eu.o_row_split = (int64_t)TX0 + (int64_t)o * Ltp + Lc; eu.bias_key = Nl; eu.bias_log2 = log2f((float)Lc);
    }

    auto qkv_args = [&](const std::string& qn, const std::string& kn, QkvSplitArgs* q) -> int {
        *q = QkvSplitArgs{};
        q->q_off = 0; q->k_off = H; q->v_off = 2 * H; q->head_stride = 64;
        q->Q = d.Q; q->K = d.K; q->Vt = d.Vt; q->Lq_pad = Tpad; q->Lk_pad = Tpad;
        q->H = heads; q->norm = QKN_RMS; q->eps = 1e-6f; q->q_scale = attn_q_scale(0.125f);
        R3G_RC(get_vec(m, qn, 64, &q->qw));
        R3G_RC(get_vec(m, kn, 64, &q->kw));
        return R3G_OK;
    };
    // nseg == 0: attention batch slot = GEMM batch index, destination row = GEMM row
    auto qkv_gemm_args = [&](const uint16_t* A, int64_t strideA, const Lin& lin, int M, const QkvSplitArgs& q, int nseg,
                             const int* seg_dev, const std::vector<int>* seg_host) {
        GemmArgs p{};
        p.A = A; p.lda = H; p.strideA = strideA; p.W = lin.w; p.ldw = lin.ldw; p.bias = lin.b;
        p.M = M; p.N = 3 * H; p.K = H; p.epi = EPI_QKV;
        p.qkv.Q = q.Q; p.qkv.K = q.K; p.qkv.Vt = q.Vt; p.qkv.Lq_pad = q.Lq_pad; p.qkv.Lk_pad = q.Lk_pad;
        p.qkv.dst_row0 = 0; p.qkv.heads = heads; p.qkv.layout = QKV_KHD; p.qkv.norm = q.norm;
        p.qkv.qw = q.qw; p.qkv.kw = q.kw; p.qkv.eps = q.eps; p.qkv.q_scale = q.q_scale; p.qkv.nseg = nseg;
        if (nseg > 3) {
            p.qkv.seg_tab = seg_dev; p.qkv.seg_tab_host = seg_host->data();
        } else {
            for (int i = 0; i < nseg; ++i) {
                p.qkv.seg_m0[i] = (*seg_host)[4 * i]; p.qkv.seg_m1[i] = (*seg_host)[4 * i + 1];
                p.qkv.seg_batch[i] = (*seg_host)[4 * i + 2]; p.qkv.seg_dst[i] = (*seg_host)[4 * i + 3];
            }
        }
        return p;
    };

    void* const xt = xrow(TX0);
    uint16_t* xnt = d.xn + (int64_t)TX0 * H;
    uint16_t* catt = d.cat + (int64_t)TX0 * catld;
    // LayerNorm + modulation of both streams: one launch over all rows (the txt rows take their own scale / shift; pad
    // rows are normalised too and never read), or one launch per stream
    auto ln_streams = [&](const float* sc_i, const float* sh_i, const float* sc_t, const float* sh_t) -> int {
        if (!g_group_streams) {
            R3G_RC(layernorm(d.f32a, H, 0, d.xn, H, 0, TX0, 1, H, nullptr, nullptr, sc_i, sh_i, 0, 1e-6f, s, xfmt));
            return layernorm((const float*)xt, H, 0, xnt, H, 0, Mtxt, 1, H, nullptr, nullptr, sc_t, sh_t, 0, 1e-6f, s, xfmt);
        }
        LnArgs p{};
        p.x = d.f32a; p.ldx = H; p.x_batch_stride = 0; p.x_bf16 = xfmt;
        p.y = d.xn; p.ldy = H; p.y_batch_stride = 0;
        p.scale = sc_i; p.shift = sh_i; p.mod_stride = 0;
        p.seg2_row0 = TX0; p.seg2_row1 = Rall; p.scale2 = sc_t; p.shift2 = sh_t;
        p.rows = Rall; p.C = H; p.rows_per_batch = Rall; p.eps = 1e-6f;
        hipError_t e = layernorm_launch(p, s);
        if (e != hipSuccess) return hip_fail(e, "layernorm_launch(streams)");
        return R3G_OK;
    };
    for (int i = 0; i < c.dit_depth_double; ++i) {
        const std::string bi = fmt("model.double_blocks.%d.img", i), bt = fmt("model.double_blocks.%d.txt", i);
        const float* mi = m.mod_all.as<float>() + m.mod_off[2 * i];
        const float* mt = m.mod_all.as<float>() + m.mod_off[2 * i + 1];
        QkvSplitArgs qi, qt;
        Lin li, lt;
        // img stream: the E*NB latent blocks (one GEMM batch entry = one attention batch slot); txt stream: per object Lc
        // cond tokens (slot E*o) and, under CFG (E == 2), 1 unconditional token (slot 2o+1).  Each layer of the two streams is one grouped launch.
        R3G_RC(ln_streams(mi + H, mi, mt + H, mt));
        R3G_RC(get_lin(m, bi + "_attn.qkv", c.dit_qkv_bias != 0, &li));
        R3G_RC(get_lin(m, bt + "_attn.qkv", c.dit_qkv_bias != 0, &lt));
        R3G_RC(qkv_args(bi + "_attn.norm.query_norm.scale", bi + "_attn.norm.key_norm.scale", &qi));
        R3G_RC(qkv_args(bt + "_attn.norm.query_norm.scale", bt + "_attn.norm.key_norm.scale", &qt));
        R3G_RC(gemm_pair(qkv_gemm_args(d.xn, (int64_t)Nl * H, li, Nl, qi, 0, nullptr, nullptr), E * NB,
                         qkv_gemm_args(xnt, 0, lt, Mtxt, qt, E * NB, d.seg_txt, &d.h_seg_txt), 1, s));
        hipError_t e = attention_launch(at, s);
        if (e != hipSuccess) return hip_fail(e, "attention_launch(dedup)");
        // attention projection
        R3G_RC(get_lin(m, bi + "_attn.proj", true, &li));
        R3G_RC(get_lin(m, bt + "_attn.proj", true, &lt));
        R3G_RC(gemm_pair(gemm_args(d.cat, catld, 0, li, 0, H, d.f32a, H, 0, TX0, H, epi_res, mi + 2 * H, 0), 1,
                         gemm_args(catt, catld, 0, lt, 0, H, xt, H, 0, Mtxt, H, epi_res, mt + 2 * H, 0), 1, s));
        // MLP
        R3G_RC(ln_streams(mi + 4 * H, mi + 3 * H, mt + 4 * H, mt + 3 * H));
        R3G_RC(get_lin(m, bi + "_mlp.0", true, &li));
        R3G_RC(get_lin(m, bt + "_mlp.0", true, &lt));
        R3G_RC(gemm_pair(gemm_args(d.xn, H, 0, li, 0, mh, d.cat + H, catld, 0, TX0, H, EPI_BF16_GELU_TANH, nullptr, 0), 1,
                         gemm_args(xnt, H, 0, lt, 0, mh, catt + H, catld, 0, Mtxt, H, EPI_BF16_GELU_TANH, nullptr, 0), 1, s));
        R3G_RC(get_lin(m, bi + "_mlp.2", true, &li));
        R3G_RC(get_lin(m, bt + "_mlp.2", true, &lt));
        R3G_RC(gemm_pair(gemm_args(d.cat + H, catld, 0, li, 0, H, d.f32a, H, 0, TX0, mh, epi_res, mi + 5 * H, 0), 1,
                         gemm_args(catt + H, catld, 0, lt, 0, H, xt, H, 0, Mtxt, mh, epi_res, mt + 5 * H, 0), 1, s));
    }
    // Single blocks: linear1 = [qkv | mlp-in] over all rows.  The attention grid leaves part of the machine idle in its
    // last dispatch round; the MLP half of linear1 does not depend on the attention, so it CAN be issued on a second stream
    // (fork after the LayerNorm, join before linear2; option overlap_mlp).  Same kernels, same operands: the result does not
    // change.  It paid (-1.1 %) while that GEMM ran 64 KiB workgroups that fit beside attention workgroups; the persistent
    // 256x256 kernel owns a whole CU's LDS.
    const bool overlap = g_overlap_mlp && c.dit_depth_single > 0;
    if (overlap && !m.aux) {      // into locals first: a failure leaves the model without any of the three, and the next forward tries again
        Stream aux;
        Event fork, join;
        R3G_TRY(aux.create(hipStreamNonBlocking));
        R3G_TRY(fork.create(hipEventDisableTiming));
        R3G_TRY(join.create(hipEventDisableTiming));
        m.aux = std::move(aux), m.ev_fork = std::move(fork), m.ev_join = std::move(join);
    }
    for (int i = 0; i < c.dit_depth_single; ++i) {
        const std::string blk = fmt("model.single_blocks.%d", i);
        const float* mm = m.mod_all.as<float>() + m.mod_off[2 * c.dit_depth_double + i];
        R3G_RC(layernorm(d.f32a, H, 0, d.xn, H, 0, Rall, 1, H, nullptr, nullptr, mm + H, mm, 0, 1e-6f, s, xfmt));
        R3G_RC(get_lin(m, blk + ".linear1", true, &l));
        QkvSplitArgs q;
        R3G_RC(qkv_args(blk + ".norm.query_norm.scale", blk + ".norm.key_norm.scale", &q));
        const GemmArgs pq = qkv_gemm_args(d.xn, 0, l, Rall, q, 2 * E * NB, d.seg_all, &d.h_seg_all);
        auto launch_qkv = [&]() -> int {
            hipError_t e = gemm_launch(pq, 1, s);
            if (e != hipSuccess) return hip_fail(e, "gemm_launch(qkv dedup)");
            return R3G_OK;
        };
        hipStream_t sm = s;
        if (overlap) {   // fork after the QKV projection: the MLP-in GEMM starts together with the attention kernel
            R3G_RC(launch_qkv());
            R3G_TRY(hipEventRecord(m.ev_fork, s));
            R3G_TRY(hipStreamWaitEvent(m.aux, m.ev_fork, 0));
            sm = m.aux;
        }
        if (overlap) {
            R3G_RC(gemm(d.xn, H, 0, l, 3 * H, mh, d.cat + H, catld, 0, Rall, H, EPI_BF16_GELU_TANH, nullptr, 0, 1, sm));
            R3G_TRY(hipEventRecord(m.ev_join, m.aux));
        } else {
            // linear1 as upstream has it -- one projection over [q k v | mlp-in] -- where the combined grid fills the machine
            // (round 6, gemm_launch_qkv_mlp); otherwise the two launches of rounds 1-5
            const GemmArgs pm = gemm_args(d.xn, H, 0, l, 3 * H, mh, d.cat + H, catld, 0, Rall, H, EPI_BF16_GELU_TANH, nullptr, 0);
            hipError_t e1 = gemm_launch_qkv_mlp(pq, pm, s);
            if (e1 != hipSuccess) return hip_fail(e1, "gemm_launch_qkv_mlp");
        }
        hipError_t e = attention_launch(at, s);
        if (e != hipSuccess) return hip_fail(e, "attention_launch(dedup)");
        if (overlap) R3G_TRY(hipStreamWaitEvent(s, m.ev_join, 0));
        R3G_RC(get_lin(m, blk + ".linear2", true, &l));
        R3G_RC(gemm(d.cat, catld, 0, l, 0, H, d.f32a, H, 0, Rall, H + mh, epi_res, mm + 2 * H, 0, 1, s));
    }
    const float* fm = m.mod_all.as<float>() + m.mod_off[2 * c.dit_depth_double + c.dit_depth_single];
    R3G_RC(layernorm(d.f32a, H, 0, d.xn, H, 0, TX0, 1, H, nullptr, nullptr, fm + H, fm, 0, 1e-6f, s, xfmt));
    R3G_RC(get_lin(m, "model.final_layer.linear", true, &l));
    R3G_RC(gemm(d.xn, H, 0, l, 0, c.dit_in_channels, out2, c.dit_in_channels, 0, TX0, H, EPI_F32, nullptr, 0, 1, s));
    return R3G_OK;
}

// ---- the geo decoder's dimensions ------------------------------------------------------------------
// r3g_model_config has no field for them: as with guidance_in, the tensors decide.  width_g = rows of query_proj.weight, heads_g =
// width_g / 64; a decoder narrower than the VAE transformer needs latents_proj (width -> width_g) in front of its ln_2.
static int geo_dims(Model& m) {
    const char* name = "vae.geo_decoder.query_proj.weight";
    const Tensor* t = m.find(name);
    if (!t || t->dtype != 1) return fail(R3G_ERR_STATE, "missing bf16 weight '%s'", name);
    const int64_t wg = t->rows;
    if (wg < 64 || wg % 64) return fail(R3G_ERR_INVALID, "'%s' has %lld rows: the geo decoder's width must be a multiple of 64", name, (long long)wg);
    if (wg > m.W) return fail(R3G_ERR_INVALID, "'%s' has %lld rows: the geo decoder cannot be wider than the VAE (width %d)", name, (long long)wg, m.W);
    m.Wg = (int)wg;
    m.Hg = (int)(wg / 64);
    if (m.Wg != m.W) {
        Lin l;
        R3G_RC(get_lin(m, "vae.geo_decoder.latents_proj", true, &l));
        if (l.N != m.Wg || l.K != m.W)
            return fail(R3G_ERR_INVALID, "'vae.geo_decoder.latents_proj.weight' is [%d][%d], expected [%d][%d]", l.N, l.K, m.Wg, m.W);
    }
    return R3G_OK;
}

// ---- VAE transformer + geo-decoder K/V -------------------------------------------------------------
static int vae_decode(Model& m, const float* latents, hipStream_t s) {
    const r3g_model_config& c = m.c;
    const int W = m.W, Nl = c.vae_num_latents, heads = m.Wh;
    R3G_RC(geo_dims(m));
    Lin l;
    R3G_TRY(cast_pad_launch(latents, c.vae_embed_dim, m.inb, m.cin_pad, Nl, c.vae_embed_dim, m.cin_pad,
                            1.0f / c.vae_scale_factor, s));
    R3G_RC(get_lin(m, "vae.post_kl", true, &l));
    R3G_RC(gemm(m.inb, m.cin_pad, 0, l, 0, W, m.z, W, 0, Nl, m.cin_pad, EPI_F32, nullptr, 0, 1, s));
    const float *lw, *lb;
    for (int i = 0; i < c.vae_layers; ++i) {
        const std::string blk = fmt("vae.transformer.resblocks.%d", i);
        R3G_RC(get_vec(m, blk + ".ln_1.weight", W, &lw));
        R3G_RC(get_vec(m, blk + ".ln_1.bias", W, &lb));
        R3G_RC(layernorm(m.z, W, 0, m.xn, W, 0, Nl, 1, W, lw, lb, nullptr, nullptr, 0, 1e-6f, s));
        R3G_RC(get_lin(m, blk + ".attn.c_qkv", c.vae_qkv_bias != 0, &l));
        QkvSplitArgs q{};
        q.src = m.qkv; q.ld = 3 * W; q.src_batch_stride = 0;
        q.q_off = 0; q.k_off = 64; q.v_off = 128; q.head_stride = 192;  // per-head interleaved (q,k,v)
        q.Q = m.Q; q.K = m.K; q.Vt = m.Vt; q.Lq_pad = (int)rup(Nl, 128); q.Lk_pad = (int)rup(Nl, 128); q.dst_row0 = 0;
        q.B = 1; q.H = heads; q.L = Nl; q.eps = 1e-6f; q.q_scale = attn_q_scale(0.125f);
        q.norm = c.vae_qk_norm ? QKN_LAYERNORM : QKN_NONE;
        if (c.vae_qk_norm) {
            R3G_RC(get_vec(m, blk + ".attn.attention.q_norm.weight", 64, &q.qw));
            R3G_RC(get_vec(m, blk + ".attn.attention.q_norm.bias", 64, &q.qb));
            R3G_RC(get_vec(m, blk + ".attn.attention.k_norm.weight", 64, &q.kw));
            R3G_RC(get_vec(m, blk + ".attn.attention.k_norm.bias", 64, &q.kb));
        }
        R3G_RC(gemm_qkv(m, m.xn, W, 0, l, 0, 3 * W, Nl, W, 1, q, QKV_HEAD_QKV, s));
        R3G_RC(attention(m, 1, heads, Nl, q.Lq_pad, Nl, q.Lk_pad, m.cat, W, 0, m.K, m.Vt, false, s));
        R3G_RC(get_lin(m, blk + ".attn.c_proj", true, &l));
        R3G_RC(gemm(m.cat, W, 0, l, 0, W, m.z, W, 0, Nl, W, EPI_RESID_F32, nullptr, 0, 1, s));
        R3G_RC(get_vec(m, blk + ".ln_2.weight", W, &lw));
        R3G_RC(get_vec(m, blk + ".ln_2.bias", W, &lb));
        R3G_RC(layernorm(m.z, W, 0, m.xn, W, 0, Nl, 1, W, lw, lb, nullptr, nullptr, 0, 1e-6f, s));
        R3G_RC(get_lin(m, blk + ".mlp.c_fc", true, &l));
        R3G_RC(gemm(m.xn, W, 0, l, 0, 4 * W, m.hid, 4 * W, 0, Nl, W, EPI_BF16_GELU_ERF, nullptr, 0, 1, s));
        R3G_RC(get_lin(m, blk + ".mlp.c_proj", true, &l));
        R3G_RC(gemm(m.hid, 4 * W, 0, l, 0, W, m.z, W, 0, Nl, 4 * W, EPI_RESID_F32, nullptr, 0, 1, s));
    }
    // geo decoder: K / V^T of the latents, computed ONCE (upstream recomputes c_kv for every query chunk)
    const std::string g = "vae.geo_decoder.cross_attn_decoder";
    const int Wg = m.Wg;
    const float* zg = m.z;
    if (Wg != W) {
        // a narrow decoder: latents_proj (width -> width_g, with bias) on the transformer's output, BEFORE ln_2.  The bf16 operand
        // goes through m.xn, the fp32 result lives in m.hid (idle between the transformer and the grid query)
        R3G_RC(get_lin(m, "vae.geo_decoder.latents_proj", true, &l));
        R3G_TRY(cast_pad_launch(m.z, W, m.xn, W, Nl, W, W, 1.0f, s));
        R3G_RC(gemm(m.xn, W, 0, l, 0, Wg, m.hid, Wg, 0, Nl, W, EPI_F32, nullptr, 0, 1, s));
        zg = reinterpret_cast<const float*>(m.hid);
    }
    R3G_RC(get_vec(m, g + ".ln_2.weight", Wg, &lw));
    R3G_RC(get_vec(m, g + ".ln_2.bias", Wg, &lb));
    R3G_RC(layernorm(zg, Wg, 0, m.xn, Wg, 0, Nl, 1, Wg, lw, lb, nullptr, nullptr, 0, 1e-6f, s));
    R3G_RC(get_lin(m, g + ".attn.c_kv", c.vae_qkv_bias != 0, &l));
    QkvSplitArgs q{};
    q.src = m.qkv; q.ld = 2 * Wg; q.src_batch_stride = 0;
    q.q_off = -1; q.k_off = 0; q.v_off = 64; q.head_stride = 128;  // per-head interleaved (k,v)
    q.Q = nullptr; q.K = m.geoK; q.Vt = m.geoVt; q.Lq_pad = 0; q.Lk_pad = (int)rup(Nl, 64); q.dst_row0 = 0;
    q.B = 1; q.H = m.Hg; q.L = Nl; q.eps = 1e-6f; q.q_scale = attn_q_scale(0.125f);
    const bool qkn = c.vae_qk_norm && c.vae_ln_post;
    q.norm = qkn ? QKN_LAYERNORM : QKN_NONE;
    if (qkn) {
        R3G_RC(get_vec(m, g + ".attn.attention.k_norm.weight", 64, &q.kw));
        R3G_RC(get_vec(m, g + ".attn.attention.k_norm.bias", 64, &q.kb));
    }
    R3G_RC(gemm_qkv(m, m.xn, Wg, 0, l, 0, 2 * Wg, Nl, Wg, 1, q, QKV_HEAD_KV, s));
    m.have_z = true;
    m.kv_v_valid = false;
    return R3G_OK;
}

// ---- fp8 mode helpers ------------------------------------------------------------------------------------------
static int fill_f32(float* dst, int n, float v, hipStream_t s) {
    std::vector<float> h((size_t)n, v);
    R3G_TRY(hipMemcpyAsync(dst, h.data(), 4 * (size_t)n, hipMemcpyHostToDevice, s));
    R3G_TRY(hipStreamSynchronize(s));
    return R3G_OK;
}

static int lin_fp8(Model& m, const Lin& l, const Model::W8** out, hipStream_t s) {
    auto it = m.w8.find(l.w);
    if (it == m.w8.end()) {
        Model::W8 q;
        R3G_RC(q.w8.grow((size_t)l.N * l.K, s, "fp8 weight"));
        R3G_RC(q.sw.grow(4 * (size_t)rup(l.N, 64), s, "fp8 weight scales"));
        R3G_TRY(quant_fp8_rows_launch(l.w, l.ldw, l.N, l.K, q.w8.as<uint8_t>(), l.K, q.sw.as<float>(), s));
        it = m.w8.emplace(l.w, std::move(q)).first;
    }
    *out = &it->second;
    return R3G_OK;
}

// C = epi(A8 W8^T): A8 [M][K] e4m3 with row scales sa, weights quantised on first use
static int gemm_fp8(Model& m, const uint8_t* A8, const float* sa, const Lin& l, void* C, int64_t ldc, int M, int epi,
                    const QkvSplitArgs* q, int qkv_layout, hipStream_t s) {
    const Model::W8* w;
    R3G_RC(lin_fp8(m, l, &w, s));
    GemmArgs p{};
    p.A = reinterpret_cast<const uint16_t*>(A8); p.lda = l.K;
    p.W = w->w8.as<const uint16_t>(); p.ldw = l.K;
    p.bias = l.b; p.C = C; p.ldc = ldc;
    p.M = M; p.N = l.N; p.K = l.K; p.epi = epi;
    p.out_inv_scale = 1.0f / kGeoHiddenScale;
    if (q) {
        p.qkv.Q = q->Q; p.qkv.K = q->K; p.qkv.Vt = q->Vt; p.qkv.Lq_pad = q->Lq_pad; p.qkv.Lk_pad = q->Lk_pad;
        p.qkv.dst_row0 = q->dst_row0; p.qkv.heads = q->H; p.qkv.layout = qkv_layout; p.qkv.norm = q->norm;
        p.qkv.qw = q->qw; p.qkv.qb = q->qb; p.qkv.kw = q->kw; p.qkv.kb = q->kb; p.qkv.eps = q->eps;
        p.qkv.q_scale = q->q_scale;
    }
    hipError_t e = gemm_fp8_launch(p, sa, w->sw.as<const float>(), s);
    if (e != hipSuccess) return hip_fail(e, "gemm_fp8_launch");
    return R3G_OK;
}

static int layernorm_fp8(const float* x, int64_t ldx, uint8_t* y8, int64_t ldy8, float* scale, int rows, int C, const float* w,
                         const float* b, float eps, hipStream_t s, int x_bf16) {
    LnArgs p{};
    p.x = x; p.ldx = ldx; p.x_bf16 = x_bf16;
    p.y8 = y8; p.ldy8 = ldy8; p.y_scale = scale;
    p.w = w; p.b = b;
    p.rows = rows; p.C = C; p.rows_per_batch = rows; p.eps = eps;
    hipError_t e = layernorm_launch(p, s);
    if (e != hipSuccess) return hip_fail(e, "layernorm_launch(fp8)");
    return R3G_OK;
}

// ---- top-k KV selection ---------------------------------------------------------------------
// the keys kept per (group, head) under the current options: 0 = exact attention
static int kv_topk_for(int num_latents) {
    if (g_geo_kv_topk == 0) return 0;
    const int k = g_geo_kv_topk < 0 ? kvsel_upstream_topk(num_latents) : g_geo_kv_topk;
    return std::max(1, std::min(k, num_latents));
}

// The attention of one pass in top-k mode: Q [H][npad][64] (the pass's rows, as the exact path holds them) is cut into groups of
// g_geo_kv_group rows; per (group, head) the k best keys are selected and gathered, and the groups run as the batches of one
// attention launch with their own K / V^T (a shorter tail group as a second launch).  Output rows land in m.cat as in the exact path.
static int kv_attention(Model& m, const uint16_t* Qp, int n, int npad, int k, hipStream_t s) {
    const int W = m.Wg, Nl = m.c.vae_num_latents, heads = m.Hg, G = g_geo_kv_group, Lkp = (int)rup(Nl, 64), kpad = (int)rup(k, 64);
    const KvselCut cut = kvsel_cut(n, G);
    R3G_RC(m.kv_q.grow(2 * (size_t)kvsel_grouped_elems(n, G, heads), s, "grouped Q"));
    R3G_RC(m.kv_k.grow(2 * (size_t)cut.groups * heads * kpad * 64, s, "compact K"));
    R3G_RC(m.kv_vt.grow(2 * (size_t)cut.groups * heads * kpad * 64, s, "compact V^T"));
    R3G_RC(m.kv_idx.grow(4 * (size_t)cut.groups * heads * k, s, "selection indices"));
    R3G_RC(m.kv_v.grow(2 * (size_t)heads * Nl * 64, s, "row-major V"));
    uint16_t *gq = m.kv_q.as<uint16_t>(), *kc = m.kv_k.as<uint16_t>(), *vtc = m.kv_vt.as<uint16_t>();
    uint16_t* vrows = m.kv_v.as<uint16_t>();
    int32_t* idx = m.kv_idx.as<int32_t>();
    if (!m.kv_v_valid) {
        R3G_TRY(kvsel_vrows_launch(m.geoVt, Nl, Lkp, heads, vrows, s));
        m.kv_v_valid = true;
    }
    m.kv_last_groups = 0;
    R3G_TRY(kvsel_regroup_launch(Qp, heads, n, npad, G, gq, s));
    R3G_TRY(kvsel_select_launch(Qp, n, npad, m.geoK, Nl, Lkp, heads, G, g_geo_kv_stride, k, idx, s));
    R3G_TRY(kvsel_gather_launch(m.geoK, vrows, Nl, Lkp, heads, idx, cut.groups, k, kc, vtc, s));
    if (cut.full) R3G_RC(attention(m, cut.full, heads, G, G, k, kpad, m.cat, W, (int64_t)G * W, kc, vtc, false, s, gq));
    if (cut.tail) {
        const int64_t kv_off = (int64_t)cut.full * heads * kpad * 64;
        R3G_RC(attention(m, 1, heads, cut.tail, cut.tail_pad, k, kpad, m.cat + (int64_t)cut.full * G * W, W, 0, kc + kv_off, vtc + kv_off,
                         false, s, gq + (int64_t)cut.full * heads * G * 64));
    }
    m.kv_last_groups = cut.groups;
    m.kv_last_k = k;
    m.kv_last_q = Qp; m.kv_last_n = n; m.kv_last_npad = npad;
    counter_add(LC_GEO_KV_GROUPS, (int64_t)cut.groups * heads);
    return R3G_OK;
}

// A pass takes its points either from the contiguous range [start, start + count) of the (R+1)^3 grid and writes their logits
// to grid[start ...] (list == nullptr: the dense decoder), or from list[0 .. count) and writes them to grid[0 .. count) (the
// hierarchical decoder's listed points; start is 0).  Everything between the Fourier features and the logits is the same
// sequence of launches.  `cache` = false keeps the call away from the query-side cache: it neither reads nor builds it and does
// not touch its (R, bound) key (listed points and the coarse levels of a hierarchical decode).
static int grid_query(Model& m, double bound, int R, float* grid, int64_t start, int64_t count, hipStream_t s,
                      const int32_t* list = nullptr, bool cache = true) {
    const r3g_model_config& c = m.c;
    if (!m.have_z) return fail(R3G_ERR_STATE, "r3g_grid_query: r3g_vae_decode has not run");
    R3G_RC(geo_dims(m));
    const int W = m.Wg, Nl = c.vae_num_latents, heads = m.Hg;      // the decoder's own width and heads from here on
    const bool narrow = W != m.W;
    if (narrow && g_geo_fp8) return fail(R3G_ERR_INVALID, "grid_query: option geo_fp8 is not available with a narrow geo decoder (width %d of %d)", W, m.W);
    const int64_t total = (int64_t)(R + 1) * (R + 1) * (R + 1);
    if (start < 0 || count < 0 || start + count > total) return fail(R3G_ERR_INVALID, "grid_query: range outside the grid");
    if (list && start != 0) return fail(R3G_ERR_INVALID, "grid_query: listed points start at 0");
    const int kv_k = kv_topk_for(Nl);
    m.kv_last_q = nullptr;      // (r3g_kv_selection_operands: the rows it points to are about to be overwritten, or freed with the cache)
    if (kv_k && g_geo_fp8) return fail(R3G_ERR_INVALID, "grid_query: top-k KV selection (option geo_kv_topk) is not available with option geo_fp8");
    const std::string g = "vae.geo_decoder";
    Lin lq, lcq, lproj, lfc, lfp;
    R3G_RC(get_lin(m, g + ".query_proj", true, &lq));
    R3G_RC(get_lin(m, g + ".cross_attn_decoder.attn.c_q", c.vae_qkv_bias != 0, &lcq));
    R3G_RC(get_lin(m, g + ".cross_attn_decoder.attn.c_proj", true, &lproj));
    R3G_RC(get_lin(m, g + ".cross_attn_decoder.mlp.c_fc", true, &lfc));
    R3G_RC(get_lin(m, g + ".cross_attn_decoder.mlp.c_proj", true, &lfp));
    const float *l1w, *l1b, *l3w, *l3b, *lpw = nullptr, *lpb = nullptr, *ow;
    R3G_RC(get_vec(m, g + ".cross_attn_decoder.ln_1.weight", W, &l1w));
    R3G_RC(get_vec(m, g + ".cross_attn_decoder.ln_1.bias", W, &l1b));
    R3G_RC(get_vec(m, g + ".cross_attn_decoder.ln_3.weight", W, &l3w));
    R3G_RC(get_vec(m, g + ".cross_attn_decoder.ln_3.bias", W, &l3b));
    if (c.vae_ln_post) {
        R3G_RC(get_vec(m, g + ".ln_post.weight", W, &lpw));
        R3G_RC(get_vec(m, g + ".ln_post.bias", W, &lpb));
    }
    R3G_RC(get_vec(m, g + ".output_proj.weight", W, &ow));
    auto obi = m.scalars.find(g + ".output_proj.bias");
    if (obi == m.scalars.end()) return fail(R3G_ERR_STATE, "missing scalar '%s.output_proj.bias'", g.c_str());
    const float ob = obi->second;
    const bool qkn = c.vae_qk_norm && c.vae_ln_post;
    const int Lkp = (int)rup(Nl, 64);
    // residual stream of the decoder block: fp32 (round 1) or, by default, bf16 -- the reference keeps it in fp16; it is
    // read / written 7 times per point, 0.9 TB per object in fp32.  The bf16 stream lives in the same buffer (m.f32a).
    const int xb = g_geo_resid_bf16 && W % 256 == 0 ? 1 : 0;
    const int epi_x0 = xb ? EPI_BF16 : EPI_F32, epi_res = xb ? EPI_RESID_BF16 : EPI_RESID_F32;
    // fp8 mode (option geo_fp8, BASELINE.json configs[3]): LayerNorm writes e4m3 + row scales, c_q / c_fc / mlp.c_proj run
    // on fp8 operands; the attention, its output projection and the residual stream stay bf16
    const bool f8 = g_geo_fp8 != 0 && xb && W % 256 == 0 && lfc.N % 256 == 0;
    const bool f8q = f8 && g_geo_fp8 != 2, f8m = f8 && g_geo_fp8 != 3;
    // the query-side cache (Model::GeoCache): bf16 stream, bf16 c_q, and room for 2 x passes x qc x W bf16 in HBM
    Model::GeoCache& gq = m.gq;
    const int64_t passes_all = (total + m.qc - 1) / m.qc;
    bool use_cache = g_geo_q_cache && xb && !f8q && cache && !list;
    if (use_cache && (gq.R != R || gq.bound != bound || gq.W != W)) {
        if (gq.x0) R3G_TRY(hipStreamSynchronize(s));
        gq.x0.release();
        gq.Q = nullptr;
        gq.R = R; gq.bound = bound; gq.W = W; gq.passes = 0; gq.built.clear(); gq.refused = false;
    }
    // (no allocation for a call that contains no canonical pass, e.g. a test's 3 000-point slice of the grid)
    const bool has_canon = start % m.qc == 0 && count >= std::min<int64_t>(m.qc, total - start);
    if (use_cache && !gq.x0 && !gq.refused && has_canon) {
        // The cache lives outside torch's allocator and stays until the model goes (or "geo_q_cache_release"): it takes at most
        // its budget (option "geo_q_cache_gb"; default 30 % of the device's memory: 86 GB of 288, the whole 257^3 grid needs
        // 68) and never the last 16 GB that are free now.  A grid that does not fit (380^3: 227 GB, 513^3: 557 GB) gets a
        // PREFIX of its passes cached; the passes behind it are recomputed per object, as before.
        const size_t per_pass = (size_t)m.qc * W * 2 * 2;
        size_t free_b = 0, total_b = 0;
        hipError_t e = hipMemGetInfo(&free_b, &total_b);
        size_t budget = g_geo_q_cache_gb >= 0 ? (size_t)g_geo_q_cache_gb << 30 : (size_t)(0.30 * (double)total_b);
        if (e == hipSuccess && free_b > ((size_t)16 << 30)) budget = std::min(budget, free_b - ((size_t)16 << 30));
        else budget = 0;
        const int64_t n_cached = std::min<int64_t>(passes_all, (int64_t)(budget / per_pass));
        if (n_cached < 1 || gq.x0.alloc((size_t)n_cached * per_pass) != hipSuccess) {
            (void)hipGetLastError();
            gq.refused = true;            // every pass is recomputed, as before
        } else {
            gq.Q = gq.x0.as<uint16_t>() + n_cached * (int64_t)m.qc * W;
            counter_add(LC_GEO_Q_CACHE_BUILDS);
            gq.passes = n_cached;
            gq.built.assign((size_t)n_cached, 0);
        }
    }
    use_cache = use_cache && gq.x0;
    if (use_cache && gq.epoch != g_option_epoch) {      // an option changed since these passes were built: build them again
        std::fill(gq.built.begin(), gq.built.end(), 0);
        gq.epoch = g_option_epoch;
    }
    // a narrow decoder of width 256: everything behind the attention in one launch per pass (geo_narrow.hip, option "geo_narrow_fused")
    const bool tail = narrow && g_geo_narrow_fused && xb && !f8 && geo_tail_supported(W, lfc.N) && lproj.N == W && lproj.K == W &&
                      lfc.K == W && lfp.N == W && lfp.K == lfc.N;
    // Round 6: ln_post + output_proj inside the last residual GEMM (EPI_RESID_BF16_LND): the final stream x2 is never written or
    // read again (2 x 268 MB per pass) and the ln_dot launch becomes a 33 MB merge of per-chunk statistics.  bf16 stream, bf16 MLP.
    // (both folds only where gemm_launch2 serves their epilogues under the current staging / epilogue switches: otherwise round 5's sequence)
    const bool lnd = g_geo_lnd_fused && xb && !f8m && c.vae_ln_post && W % 256 == 0 && W <= 4096 && lfc.N % 128 == 0 && lfc.N >= 256 &&
                     gemm_fold_supported(EPI_RESID_BF16_LND, m.qc, W, lfc.N);
    // ... and ln_3 the same way, its weights being static: c_proj's epilogue also writes the row statistics of the stream it stores
    // (EPI_RESID_BF16_ST), a small kernel merges them into (mean, rstd), and c_fc runs on the RAW stream with W' = bf16(W gamma) and the
    // epilogue rstd (acc - mean c1) + c2 in front of its GELU (EPI_BF16_GELU_ERF_LNF) -- no LayerNorm launch, no normalised copy of the
    // stream (2 x 268 MB per pass).
    const bool lnf = g_geo_ln3_fold && xb && !f8m && W % 256 == 0 && W <= 4096 && lfc.N % 256 == 0 &&
                     gemm_fold_supported(EPI_RESID_BF16_ST, m.qc, W, W) && gemm_fold_supported(EPI_BF16_GELU_ERF_LNF, m.qc, lfc.N, W);
    if ((lnd || lnf) && !tail) R3G_RC(m.lnd_part.grow(16 * (size_t)m.qc * (size_t)(W / 64), s, "ln fold chunk statistics"));
    if (lnd && !tail) {
        R3G_RC(m.lnd_gw.grow(4 * (size_t)(W + 64), s, "ln_post fold weights"));
        float* gw = m.lnd_gw.as<float>();
        R3G_TRY(lnd_prepare_launch(lpw, lpb, ow, ob, W, gw, gw + W, s));      // (per call: the weights may have been re-registered)
    }
    if (tail) {
        R3G_RC(m.geo_tail_packed.grow(geo_tail_packed_bytes(lfc.N), s, "narrow tail fragments"));
        // (per call: the weights may have been re-registered)
        R3G_TRY(geo_tail_pack_launch(lproj.w, lproj.ldw, lfc.w, lfc.ldw, lfp.w, lfp.ldw, lfc.N, m.geo_tail_packed.p, s));
    }
    Lin lfc2 = lfc;
    if (lnf && !tail) {      // each buffer on its own: a call after a failed allocation makes up what is missing
        R3G_RC(m.lnf_w.grow(2 * (size_t)lfc.N * (size_t)W, s, "ln_3 fold weights"));
        R3G_RC(m.lnf_c.grow(4 * 2 * (size_t)lfc.N, s, "ln_3 fold constants"));
        R3G_RC(m.lnf_stats.grow(8 * (size_t)m.qc, s, "ln_3 fold row statistics"));
        float* c1 = m.lnf_c.as<float>();
        R3G_TRY(lnf_prepare_launch(lfc.w, lfc.ldw, lfc.b, l3w, l3b, lfc.N, W, m.lnf_w.as<uint16_t>(), c1, c1 + lfc.N, s));
        lfc2.w = m.lnf_w.as<uint16_t>(); lfc2.ldw = W; lfc2.K = W; lfc2.b = c1 + lfc.N;
    }
    if (f8) {
        R3G_RC(m.fp8_sa.grow(4 * (size_t)m.qc, s, "fp8 activation scales"));
        if (!m.fp8_sconst) {
            R3G_RC(m.fp8_sconst.grow(4 * (size_t)m.qc, s, "fp8 hidden scales"));
            if (const int rc = fill_f32(m.fp8_sconst.as<float>(), m.qc, kGeoHiddenScale, s)) {
                m.fp8_sconst.release();      // held means filled
                return rc;
            }
        }
    }
    float *const lnd_part = m.lnd_part.as<float>(), *const lnd_gw = m.lnd_gw.as<float>();
    float *const fp8_sa = m.fp8_sa.as<float>(), *const fp8_sconst = m.fp8_sconst.as<float>();
    for (int64_t off = 0; off < count; off += m.qc) {
        const int n = (int)std::min<int64_t>(m.qc, count - off);
        const int npad = (int)rup(n, 128);
        // a pass is served from / stored into the cache when it is one of the grid's canonical passes: it starts at a
        // multiple of the pass size and covers the pass completely (sub-range queries are computed the old way)
        const int64_t p0 = start + off;
        const int64_t pidx = p0 / m.qc;
        const bool canon = use_cache && pidx < gq.passes && p0 % m.qc == 0 && n == (int)std::min<int64_t>(m.qc, total - p0);
        const bool hit = canon && gq.built[(size_t)pidx];
        uint16_t* x0 = canon ? gq.x0.as<uint16_t>() + pidx * (int64_t)m.qc * W : reinterpret_cast<uint16_t*>(m.f32a);
        uint16_t* Qp = canon ? gq.Q + pidx * (int64_t)m.qc * W : m.Q;
        uint8_t* xn8 = reinterpret_cast<uint8_t*>(m.xn);
        uint8_t* hid8 = reinterpret_cast<uint8_t*>(m.hid);
        if (!hit) {
            if (list) R3G_TRY(fourier_points_launch(m.inb, list + off, n, npad, R, bound, c.vae_num_freqs, c.vae_include_pi, s));
            else R3G_TRY(fourier_grid_launch(m.inb, p0, npad, R, bound, c.vae_num_freqs, c.vae_include_pi, s));
            R3G_RC(gemm(m.inb, 64, 0, lq, 0, W, xb ? (void*)x0 : (void*)m.f32a, W, 0, n, 64, epi_x0, nullptr, 0, 1, s));
            const float* xin = xb ? reinterpret_cast<const float*>(x0) : m.f32a;
            if (f8q) R3G_RC(layernorm_fp8(xin, W, xn8, W, fp8_sa, n, W, l1w, l1b, 1e-6f, s, xb));
            else R3G_RC(layernorm(xin, W, 0, m.xn, W, 0, n, 1, W, l1w, l1b, nullptr, nullptr, 0, 1e-6f, s, xb));
            QkvSplitArgs q{};
            q.src = m.qkv; q.ld = W; q.src_batch_stride = 0;
            q.q_off = 0; q.k_off = -1; q.v_off = -1; q.head_stride = 64;
            q.Q = Qp; q.K = nullptr; q.Vt = nullptr; q.Lq_pad = npad; q.Lk_pad = 0; q.dst_row0 = 0;
            q.B = 1; q.H = heads; q.L = n; q.eps = 1e-6f; q.q_scale = attn_q_scale(0.125f);
            q.norm = qkn ? QKN_LAYERNORM : QKN_NONE;
            if (qkn) {
                R3G_RC(get_vec(m, g + ".cross_attn_decoder.attn.attention.q_norm.weight", 64, &q.qw));
                R3G_RC(get_vec(m, g + ".cross_attn_decoder.attn.attention.q_norm.bias", 64, &q.qb));
            }
            if (f8q) R3G_RC(gemm_fp8(m, xn8, fp8_sa, lcq, nullptr, 0, n, EPI_QKV, &q, QKV_Q_ONLY, s));
            else R3G_RC(gemm_qkv(m, m.xn, W, 0, lcq, 0, W, n, W, 1, q, QKV_Q_ONLY, s));
            if (canon) gq.built[(size_t)pidx] = 1;
        }
        if (kv_k) R3G_RC(kv_attention(m, Qp, n, npad, kv_k, s));
        else R3G_RC(attention(m, 1, heads, n, npad, Nl, Lkp, m.cat, W, 0, m.geoK, m.geoVt, true, s, Qp));
        if (tail) {
            GeoTailArgs ta{};
            ta.cat = m.cat; ta.ld_cat = W;
            ta.x0 = canon ? x0 : reinterpret_cast<const uint16_t*>(m.f32a); ta.ld_x0 = W;
            ta.packed = m.geo_tail_packed.p;
            ta.b_proj = lproj.b; ta.ln3_w = l3w; ta.ln3_b = l3b; ta.b_fc = lfc.b; ta.b_fp = lfp.b;
            ta.lnp_w = lpw; ta.lnp_b = lpb; ta.out_w = ow; ta.out_b = ob;
            ta.hidden = lfc.N; ta.n = n; ta.out = grid + start + off;
            R3G_TRY(geo_tail_launch(ta, s));
            counter_add(LC_GEO_NARROW_PASSES);
            continue;
        }
        {   // x1 = x0 + c_proj(attention): the old values come from the cached x0 where there is one
            GemmArgs pr = gemm_args(m.cat, W, 0, lproj, 0, W, m.f32a, W, 0, n, W, lnf ? (int)EPI_RESID_BF16_ST : epi_res, nullptr, 0);
            pr.lnd_part = lnd_part;
            if (canon) pr.resid_src = x0;
            hipError_t e = gemm_launch(pr, 1, s);
            if (e != hipSuccess) return hip_fail(e, "gemm_launch(geo c_proj)");
        }
        if (f8m) {
            R3G_RC(layernorm_fp8(m.f32a, W, xn8, W, fp8_sa, n, W, l3w, l3b, 1e-6f, s, xb));
            R3G_RC(gemm_fp8(m, xn8, fp8_sa, lfc, hid8, lfc.N, n, EPI_FP8_GELU_ERF, nullptr, 0, s));
            R3G_RC(gemm_fp8(m, hid8, fp8_sconst, lfp, m.f32a, W, n, epi_res, nullptr, 0, s));
        } else {
            if (lnf) {
                R3G_TRY(lnf_stats_launch(lnd_part, n, W / 64, 1e-6f, m.lnf_stats.as<float>(), s));
                GemmArgs pf = gemm_args(reinterpret_cast<const uint16_t*>(m.f32a), W, 0, lfc2, 0, lfc.N, m.hid, lfc.N, 0, n, W,
                                        EPI_BF16_GELU_ERF_LNF, nullptr, 0);
                pf.lnf_c1 = m.lnf_c.as<float>();
                pf.lnf_stats = m.lnf_stats.as<float>();
                hipError_t e = gemm_launch(pf, 1, s);
                if (e != hipSuccess) return hip_fail(e, "gemm_launch(geo ln_3 + mlp.c_fc)");
                counter_add(LC_GEO_LNF_PASSES);
            } else {
                R3G_RC(layernorm(m.f32a, W, 0, m.xn, W, 0, n, 1, W, l3w, l3b, nullptr, nullptr, 0, 1e-6f, s, xb));
                R3G_RC(gemm(m.xn, W, 0, lfc, 0, lfc.N, m.hid, lfc.N, 0, n, W, EPI_BF16_GELU_ERF, nullptr, 0, 1, s));
            }
            if (lnd) {
                GemmArgs pl = gemm_args(m.hid, lfc.N, 0, lfp, 0, W, m.f32a, W, 0, n, lfc.N, EPI_RESID_BF16_LND, nullptr, 0);
                pl.lnd_gw = lnd_gw;
                pl.lnd_part = lnd_part;
                hipError_t e = gemm_launch(pl, 1, s);
                if (e != hipSuccess) return hip_fail(e, "gemm_launch(geo mlp.c_proj + ln_post + output_proj)");
                R3G_TRY(lnd_finalize_launch(lnd_part, n, W / 64, 1e-5f, lnd_gw + W, grid + start + off, s));
                counter_add(LC_GEO_LND_PASSES);
                continue;
            }
            R3G_RC(gemm(m.hid, lfc.N, 0, lfp, 0, W, m.f32a, W, 0, n, lfc.N, epi_res, nullptr, 0, 1, s));
        }
        R3G_TRY(ln_dot_launch(m.f32a, W, n, W, c.vae_ln_post, lpw, lpb, 1e-5f, ow, ob, grid + start + off, s, xb));
    }
    return R3G_OK;
}

// ---- conditioner (Dinov2) ----------------------------------------------------------------------------
static int cond_encode(Model& m, const float* img, uint16_t* out, hipStream_t s) {
    const r3g_model_config& c = m.c;
    const int Hc = m.Hc, heads = m.Hch, S = c.cond_image_size, ps = c.cond_patch, P = S / ps, L = m.Lc, Lp = m.Lcpad;
    const std::string e = "conditioner.main_image_encoder.model";
    Lin l;
    R3G_RC(get_lin(m, e + ".embeddings.patch_embeddings.projection", true, &l));
    R3G_TRY(im2col_launch(img, S, ps, m.inb, l.K, s));
    R3G_RC(gemm(m.inb, l.K, 0, l, 0, Hc, m.f32a + Hc, Hc, 0, P * P, l.K, EPI_F32, nullptr, 0, 1, s));
    const float *cls, *pos;
    R3G_RC(get_vec(m, e + ".embeddings.cls_token", Hc, &cls));
    R3G_RC(get_vec(m, e + ".embeddings.position_embeddings", (int64_t)L * Hc, &pos));
    R3G_TRY(fill_rows_launch(m.f32a, Hc, 1, Hc, cls, s));
    R3G_TRY(add_rows_launch(m.f32a, Hc, pos, Hc, L, Hc, s));
    const float *w, *b, *ls;
    for (int i = 0; i < c.cond_layers; ++i) {
        const std::string blk = fmt("%s.encoder.layer.%d", e.c_str(), i);
        R3G_RC(get_vec(m, blk + ".norm1.weight", Hc, &w));
        R3G_RC(get_vec(m, blk + ".norm1.bias", Hc, &b));
        R3G_RC(layernorm(m.f32a, Hc, 0, m.xn, Hc, 0, L, 1, Hc, w, b, nullptr, nullptr, 0, c.cond_ln_eps, s));
        R3G_RC(get_lin(m, blk + ".attention.attention.qkv", true, &l));
        QkvSplitArgs q{};
        q.src = m.qkv; q.ld = 3 * Hc; q.src_batch_stride = 0;
        q.q_off = 0; q.k_off = Hc; q.v_off = 2 * Hc; q.head_stride = 64;
        q.Q = m.Q; q.K = m.K; q.Vt = m.Vt; q.Lq_pad = Lp; q.Lk_pad = Lp; q.dst_row0 = 0;
        q.B = 1; q.H = heads; q.L = L; q.norm = QKN_NONE; q.eps = 0.f; q.q_scale = attn_q_scale(0.125f);
        R3G_RC(gemm_qkv(m, m.xn, Hc, 0, l, 0, 3 * Hc, L, Hc, 1, q, QKV_KHD, s));
        R3G_RC(attention(m, 1, heads, L, Lp, L, Lp, m.cat, Hc, 0, m.K, m.Vt, false, s));
        R3G_RC(get_lin(m, blk + ".attention.output.dense", true, &l));
        R3G_RC(get_vec(m, blk + ".layer_scale1.lambda1", Hc, &ls));
        R3G_RC(gemm(m.cat, Hc, 0, l, 0, Hc, m.f32a, Hc, 0, L, Hc, EPI_RESID_F32, ls, 0, 1, s));
        R3G_RC(get_vec(m, blk + ".norm2.weight", Hc, &w));
        R3G_RC(get_vec(m, blk + ".norm2.bias", Hc, &b));
        R3G_RC(layernorm(m.f32a, Hc, 0, m.xn, Hc, 0, L, 1, Hc, w, b, nullptr, nullptr, 0, c.cond_ln_eps, s));
        R3G_RC(get_lin(m, blk + ".mlp.weights_in", true, &l));
        if (l.N != 2 * m.Fc) return fail(R3G_ERR_INVALID, "Dinov2 SwiGLU weights_in N=%d, expected %d", l.N, 2 * m.Fc);
        R3G_RC(gemm(m.xn, Hc, 0, l, 0, 2 * m.Fc, m.hid, 2 * m.Fc, 0, L, Hc, EPI_BF16, nullptr, 0, 1, s));
        uint16_t* h2 = m.hid + (int64_t)Lp * 2 * m.Fc;
        R3G_TRY(swiglu_launch(m.hid, 2 * m.Fc, h2, m.Fc, L, m.Fc, s));
        R3G_RC(get_lin(m, blk + ".mlp.weights_out", true, &l));
        R3G_RC(get_vec(m, blk + ".layer_scale2.lambda1", Hc, &ls));
        R3G_RC(gemm(h2, m.Fc, 0, l, 0, Hc, m.f32a, Hc, 0, L, m.Fc, EPI_RESID_F32, ls, 0, 1, s));
    }
    R3G_RC(get_vec(m, e + ".layernorm.weight", Hc, &w));
    R3G_RC(get_vec(m, e + ".layernorm.bias", Hc, &b));
    R3G_RC(layernorm(m.f32a, Hc, 0, out, Hc, 0, L, 1, Hc, w, b, nullptr, nullptr, 0, c.cond_ln_eps, s));
    return R3G_OK;
}

// ---- lifetime ----------------------------------------------------------------------------------------
static void model_free(Model* m) { delete m; }      // the buffers, the stream and the events go with their members

static int model_create(Ctx* ctx, const r3g_model_config* cfg) {
    if (ctx->model) { model_free((Model*)ctx->model); ctx->model = nullptr; }
    Model* m = new Model();
    m->c = *cfg;
    const r3g_model_config& c = m->c;
    m->H = c.dit_hidden; m->Hd = c.dit_heads; m->W = c.vae_width; m->Wh = c.vae_heads;
    m->Hc = c.cond_hidden; m->Hch = c.cond_heads; m->Fc = c.cond_ffn_hidden;
    const int P = c.cond_image_size / c.cond_patch;
    m->Lc = P * P + 1;
    m->Lcpad = (int)rup(m->Lc, 128);
    m->T = c.vae_num_latents + m->Lc;
    m->Tpad = (int)rup(m->T, 128);
    m->cin_pad = (int)rup(std::max(c.dit_in_channels, c.vae_embed_dim), 64);
    m->qc = c.grid_chunk > 0 ? (int)rup(c.grid_chunk, 128) : 131072;
    auto bad = [&](const char* what) { model_free(m); return fail(R3G_ERR_INVALID, "r3g_model_create: %s", what); };
    if (m->H != 64 * m->Hd || m->W != 64 * m->Wh || m->Hc != 64 * m->Hch) return bad("every attention here needs head_dim == 64");
    if (m->H % 64 || m->W % 64 || m->Hc % 64 || m->Fc % 64 || c.dit_context_dim % 64) return bad("hidden sizes must be multiples of 64");
    if (c.vae_num_latents < 1) return bad("num_latents must be positive");
    if (c.dit_context_dim != m->Hc) return bad("dit_context_dim must equal the conditioner hidden size");
    if (c.dit_in_channels != c.vae_embed_dim) return bad("dit_in_channels must equal vae_embed_dim");
    if (c.dit_in_channels % 4) return bad("in_channels must be a multiple of 4");
    const int H = m->H, W = m->W, Hc = m->Hc, Nl = c.vae_num_latents, Tp = m->Tpad, Lp = m->Lcpad, qc = m->qc;
    const int Nlp = (int)rup(Nl, 128);
    const int64_t Kpatch = rup(3 * c.cond_patch * c.cond_patch, 64);
    auto mx = [](std::initializer_list<int64_t> v) { int64_t r = 0; for (auto x : v) r = std::max(r, x); return r; };
    const int64_t n_f32a = mx({2LL * Tp * H, (int64_t)Lp * Hc, (int64_t)qc * W});
    const int64_t n_xn = n_f32a;
    const int64_t n_qkv = mx({2LL * Tp * 3 * H, (int64_t)Nlp * 3 * W, (int64_t)Lp * 3 * Hc, (int64_t)qc * W});
    const int64_t n_q = mx({2LL * Tp * H, (int64_t)Nlp * W, (int64_t)Lp * Hc, (int64_t)qc * W});
    const int64_t n_kv = mx({2LL * Tp * H, (int64_t)Nlp * W, (int64_t)Lp * Hc});
    const int64_t n_cat = mx({2LL * Tp * 5 * H, (int64_t)Nlp * W, (int64_t)Lp * Hc, (int64_t)qc * W});
    const int64_t n_hid = mx({(int64_t)Nlp * 4 * W, (int64_t)Lp * 3 * m->Fc, (int64_t)qc * c.vae_mlp_ratio * W});
    const int64_t n_inb = mx({2LL * Nl * m->cin_pad, (int64_t)(qc + 128) * 64, (int64_t)P * P * Kpatch});
    const int64_t n_small = 2 * 256 + 2 * H + 2 * H + 2 * 12 * H + 4LL * Nl * c.dit_in_channels + (256 + 2 * H) + 1024;
    const int64_t n_z = (int64_t)Nl * W;
    const int64_t n_geo = (int64_t)rup(Nl, 64) * W;
    size_t off = 0;
    auto carve = [&](int64_t bytes) { size_t o = off; off += (size_t)rup(bytes, 256); return o; };
    const size_t o_f32a = carve(n_f32a * 4), o_xn = carve(n_xn * 2), o_qkv = carve(n_qkv * 2), o_q = carve(n_q * 2),
                 o_k = carve(n_kv * 2), o_vt = carve(n_kv * 2), o_cat = carve(n_cat * 2), o_hid = carve(n_hid * 2),
                 o_inb = carve(n_inb * 2), o_small = carve(n_small * 4), o_z = carve(n_z * 4), o_gk = carve(n_geo * 2),
                 o_gv = carve(n_geo * 2);
    if (const int rc = m->arena.grow(off, nullptr, "model arena")) { model_free(m); return rc; }
    const hipError_t e = hipMemset(m->arena.p, 0, off);  // padded rows / columns must start finite
    if (e != hipSuccess) { model_free(m); return hip_fail(e, "hipMemset(model arena)"); }
    char* a = m->arena.p;
    m->f32a = (float*)(a + o_f32a); m->xn = (uint16_t*)(a + o_xn); m->qkv = (uint16_t*)(a + o_qkv);
    m->Q = (uint16_t*)(a + o_q); m->K = (uint16_t*)(a + o_k); m->Vt = (uint16_t*)(a + o_vt);
    m->cat = (uint16_t*)(a + o_cat); m->hid = (uint16_t*)(a + o_hid); m->inb = (uint16_t*)(a + o_inb);
    m->small = (float*)(a + o_small); m->z = (float*)(a + o_z); m->geoK = (uint16_t*)(a + o_gk); m->geoVt = (uint16_t*)(a + o_gv);
    m->temb = m->small; m->th = m->temb + 2 * 256; m->vec = m->th + 2 * H; m->mods = m->vec + 2 * H;
    m->v2 = m->mods + 2 * 12 * H;
    m->gemb = m->v2 + 4LL * Nl * c.dit_in_channels; m->gth = m->gemb + 256; m->gvec = m->gth + H;
    ctx->model = m;
    return R3G_OK;
}

}  // namespace r3g

using namespace r3g;

void r3g::Ctx::release_model() {
    if (model) model_free((Model*)model);
    model = nullptr;
}

static Model* model_of(r3g_ctx* ctx) { return ctx ? (Model*)reinterpret_cast<Ctx*>(ctx)->model : nullptr; }
#define NEED_MODEL(fn)                                                                       \
    Model* m = model_of(ctx);                                                                \
    if (!m) return fail(R3G_ERR_STATE, fn ": r3g_model_create has not been called");

extern "C" {

int r3g_model_create(r3g_ctx* ctx, const r3g_model_config* cfg) {
    if (!ctx || !cfg) return fail(R3G_ERR_INVALID, "r3g_model_create: null argument");
    return model_create(reinterpret_cast<Ctx*>(ctx), cfg);
}

int r3g_model_set_tensor(r3g_ctx* ctx, const char* name, const void* d_ptr, int dtype, int64_t rows, int64_t cols) {
    NEED_MODEL("r3g_model_set_tensor");
    if (!name || !d_ptr || (dtype != 0 && dtype != 1) || rows <= 0 || cols <= 0)
        return fail(R3G_ERR_INVALID, "r3g_model_set_tensor: bad argument for '%s'", name ? name : "?");
    m->w[name] = Tensor{d_ptr, dtype, rows, cols};
    if (!m->gq.built.empty()) std::fill(m->gq.built.begin(), m->gq.built.end(), 0);   // the cached query side belongs to the old weights
    return R3G_OK;
}

int r3g_model_set_scalar(r3g_ctx* ctx, const char* name, float value) {
    NEED_MODEL("r3g_model_set_scalar");
    if (!name) return fail(R3G_ERR_INVALID, "r3g_model_set_scalar: null name");
    m->scalars[name] = value;
    return R3G_OK;
}

int r3g_cond_encode(r3g_ctx* ctx, const float* d_image, uint16_t* d_cond_out, void* stream) {
    NEED_MODEL("r3g_cond_encode");
    if (!d_image || !d_cond_out) return fail(R3G_ERR_INVALID, "r3g_cond_encode: null argument");
    return cond_encode(*m, d_image, d_cond_out, (hipStream_t)stream);
}

int r3g_dit_forward(r3g_ctx* ctx, const float* d_x, const float* d_t, const uint16_t* d_cond, float* d_out, int batch,
                    int n_double, int n_single, void* stream) {
    NEED_MODEL("r3g_dit_forward");
    if (!d_x || !d_t || !d_cond || !d_out) return fail(R3G_ERR_INVALID, "r3g_dit_forward: null argument");
    return dit_forward(*m, d_x, d_t, 0.f, d_cond, d_out, batch, n_double, n_single, (hipStream_t)stream);
}

int r3g_dit_stream(r3g_ctx* ctx, float* d_out, int batch, void* stream) {
    NEED_MODEL("r3g_dit_stream");
    if (!d_out || batch < 1 || batch > 2) return fail(R3G_ERR_INVALID, "r3g_dit_stream: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int64_t H = m->H, Nl = m->c.vae_num_latents, Lc = m->Lc, T = m->T, xs = (int64_t)m->Tpad * H;
    for (int b = 0; b < batch; ++b) {   // arena order [latent | cond | pad]  ->  upstream order cat(cond, latent)
        R3G_TRY(hipMemcpyAsync(d_out + b * T * H, m->f32a + b * xs + Nl * H, (size_t)(Lc * H) * 4, hipMemcpyDeviceToDevice, s));
        R3G_TRY(hipMemcpyAsync(d_out + b * T * H + Lc * H, m->f32a + b * xs, (size_t)(Nl * H) * 4, hipMemcpyDeviceToDevice, s));
    }
    return R3G_OK;
}

// The denoising loop for n_objects objects (latents f32 [n][Nl][Cin], cond2 bf16 [n][2][Lc][D]) over the sigma table
// sig[0 .. steps].  With a de-duplicated unconditional context all objects go through every DiT layer together; otherwise one
// after the other.  A guidance-distilled model (model.guidance_in.*) has no CFG batch: its objects always share the launches,
// one entry each, the unconditional half of cond2 is never read and guidance_scale only feeds guidance_in.
static int flow_sample(Model* m, float* d_latents, const uint16_t* d_cond2, int n_objects, const std::vector<float>& sig,
                       float guidance_scale, int uncond_uniform, hipStream_t s) {
    const r3g_model_config& c = m->c;
    const int steps = (int)sig.size() - 1;
    const int64_t n = (int64_t)c.vae_num_latents * c.dit_in_channels;
    const int64_t cond_elems = (int64_t)m->Lc * c.dit_context_dim;
    bool distilled = false;
    R3G_RC(dit_latents_aligned(*m));
    R3G_RC(model_distilled(*m, &distilled));
    const bool dedup = g_cfg_dedup && uncond_uniform != 0;
    if (!dedup && !distilled) {
        float* x2 = m->v2 + 2 * n;  // [2][n] duplicated latents (CFG batch)
        for (int o = 0; o < n_objects; ++o) {
            float* lat = d_latents + o * n;
            const uint16_t* cond2 = d_cond2 + 2 * o * cond_elems;
            for (int i = std::max(0, g_flow_first_step); i < flow_last_step(steps); ++i) {
                const float ds = sig[i + 1] - sig[i];
                if (ds == 0.f && g_skip_zero_step) continue;
                R3G_TRY(hipMemcpyAsync(x2, lat, n * 4, hipMemcpyDeviceToDevice, s));
                R3G_TRY(hipMemcpyAsync(x2 + n, lat, n * 4, hipMemcpyDeviceToDevice, s));
                counter_add(LC_DIT_EVALS);
                R3G_RC(dit_forward(*m, x2, nullptr, sig[i], cond2, m->v2, 2, -1, -1, s));
                R3G_TRY(cfg_euler_launch(lat, m->v2, n, guidance_scale, ds, s));
            }
        }
        return R3G_OK;
    }
    const int E = distilled ? 1 : 2, group = distilled ? kMaxObjectsDistilled : kMaxObjects;
    if (distilled) {
        // guidance_in(timestep_embedding(g)) depends on neither the step nor the object: once per call.  g goes through the same
        // embedding as t (time_factor applied, cos first).
        const int H = m->H;
        Lin l;
        R3G_TRY(timestep_embedding_launch(nullptr, guidance_scale, 1, c.dit_time_factor, m->gemb, s));
        R3G_RC(get_lin(*m, "model.guidance_in.in_layer", true, &l));
        if (l.N != H || l.K != 256) return fail(R3G_ERR_INVALID, "'model.guidance_in.in_layer.weight' is [%d][%d], expected [%d][256]", l.N, l.K, H);
        R3G_TRY(gemv_launch(m->gemb, 1, 256, l.w, l.ldw, l.b, m->gth, H, 0, 1, s));
        R3G_RC(get_lin(*m, "model.guidance_in.out_layer", true, &l));
        if (l.N != H || l.K < H) return fail(R3G_ERR_INVALID, "'model.guidance_in.out_layer.weight' is [%d][%d], expected [%d][%d]", l.N, l.K, H, H);
        R3G_TRY(gemv_launch(m->gth, 1, H, l.w, l.ldw, l.b, m->gvec, H, 0, 0, s));
    }
    for (int o0 = 0; o0 < n_objects; o0 += group) {
        const int NB = std::min(group, n_objects - o0);
        R3G_RC(ensure_dit_batch(*m, NB, E));
        Model::DitBatch& d = m->db;
        const int Ltp = dit_txt_rows(*m);
        for (int o = 0; o < NB; ++o) {   // context rows of object o: its Lc cond tokens, then (CFG) ONE unconditional token
            const uint16_t* cond2 = d_cond2 + 2 * (int64_t)(o0 + o) * cond_elems;
            uint16_t* dst = d.ctx + (int64_t)o * Ltp * c.dit_context_dim;
            R3G_TRY(hipMemcpyAsync(dst, cond2, (size_t)cond_elems * 2, hipMemcpyDeviceToDevice, s));
            if (E == 2)
                R3G_TRY(hipMemcpyAsync(dst + cond_elems, cond2 + cond_elems, (size_t)c.dit_context_dim * 2, hipMemcpyDeviceToDevice, s));
        }
        float* lat = d_latents + o0 * n;
        // The fp16 residual stream (option dit_resid_f16, default) tops out at 65504 where the fp32 stream of rounds 1-3 could not
        // overflow: the group's initial latents are kept, the final latents are checked for NaN / infinity once per group (one
        // small kernel and a 4-byte read-back behind ~5 s of GPU work), and a group that overflowed is run again on the fp32
        // stream -- never silently wrong latents from a checkpoint whose activations outgrow fp16.
        const bool guard = g_dit_resid_f16 && m->H % 256 == 0 && g_dit_f16_guard;
        if (guard) R3G_TRY(hipMemcpyAsync(d.lat0, lat, (size_t)NB * n * 4, hipMemcpyDeviceToDevice, s));
        counter_add(LC_DIT_GROUPS);
        for (int attempt = 0; attempt < 2; ++attempt) {
            const bool allow_f16 = attempt == 0;
            for (int i = std::max(0, g_flow_first_step); i < flow_last_step(steps); ++i) {
                // the final step of upstream's schedule has d_sigma = 0: its update is x += 0 * v, so the evaluation is skipped
                // (bit-identical; r3g_set_option("skip_zero_step", 0) evaluates it as upstream does)
                const float ds = sig[i + 1] - sig[i];
                if (ds == 0.f && g_skip_zero_step) continue;
                R3G_RC(dit_forward_grouped(*m, lat, sig[i], d.v2, NB, s, allow_f16, distilled ? m->gvec : nullptr));
                if (distilled) R3G_TRY(euler_step_launch(lat, d.v2, (int64_t)NB * n, ds, s));   // all objects of the group: lat += d_sigma v
                else for (int o = 0; o < NB; ++o) R3G_TRY(cfg_euler_launch(lat + o * n, d.v2 + 2 * o * n, n, guidance_scale, ds, s));
            }
            if (!guard || attempt == 1) break;
            int bad = 0;
            R3G_TRY(hipMemsetAsync(d.bad, 0, 4, s));
            R3G_TRY(nonfinite_flag_launch(lat, (int64_t)NB * n, d.bad, s));
            R3G_TRY(hipMemcpyAsync(&bad, d.bad, 4, hipMemcpyDeviceToHost, s));
            R3G_TRY(hipStreamSynchronize(s));
            if (!bad) break;
            counter_add(LC_DIT_F16_FALLBACKS);
            fprintf(stderr, "[r3g] the fp16 residual stream of the DiT overflowed (non-finite latents): this launch group runs again on "
                            "the fp32 stream (r3g_set_option(\"dit_resid_f16\", 0) makes that the default)\n");
            R3G_TRY(hipMemcpyAsync(lat, d.lat0, (size_t)NB * n * 4, hipMemcpyDeviceToDevice, s));
        }
    }
    return R3G_OK;
}

// sigmas of FlowMatchEulerDiscreteScheduler: linspace(0,1,steps) (shifted), + a trailing 1: the last update has d_sigma = 0, as upstream
static std::vector<float> linspace_sigmas(int steps, float shift) {
    std::vector<float> sig(steps + 1);
    for (int i = 0; i < steps; ++i) {
        const double v = steps == 1 ? 0.0 : (double)i / (double)(steps - 1);
        sig[i] = (float)(shift * v / (1.0 + (shift - 1.0) * v));
    }
    sig[steps] = 1.0f;
    return sig;
}

int r3g_get_counter(const char* name, int64_t* value) {
    if (!name || !value) return fail(R3G_ERR_INVALID, "r3g_get_counter: null argument");
    for (int i = 0; i < LC_COUNT; ++i)
        if (!strcmp(name, kCounterNames[i])) {
            *value = i == LC_DEVICE_BYTES_LIVE ? g_device_bytes_live.load() : g_counters[i].load(std::memory_order_relaxed);
            return R3G_OK;
        }
    return fail(R3G_ERR_INVALID, "r3g_get_counter: unknown counter '%s'", name);
}

const char* r3g_counter_name(int index) { return index >= 0 && index < LC_COUNT ? kCounterNames[index] : nullptr; }

int r3g_model_trim(r3g_ctx* ctx) {
    NEED_MODEL("r3g_model_trim");
    Model::GeoCache& gq = m->gq;
    m->kv_last_q = nullptr;
    if (gq.x0) {
        R3G_TRY(hipDeviceSynchronize());
        gq.x0.release();
        gq.Q = nullptr;
        gq.passes = 0;
        gq.built.clear();
    }
    gq.refused = false;
    return R3G_OK;
}

int r3g_flow_sample(r3g_ctx* ctx, float* d_latents, const uint16_t* d_cond2, int steps, float guidance_scale,
                    float shift, int uncond_uniform, void* stream) {
    NEED_MODEL("r3g_flow_sample");
    if (!d_latents || !d_cond2 || steps < 1) return fail(R3G_ERR_INVALID, "r3g_flow_sample: bad argument");
    return flow_sample(m, d_latents, d_cond2, 1, linspace_sigmas(steps, shift), guidance_scale, uncond_uniform, (hipStream_t)stream);
}

int r3g_flow_sample_batch(r3g_ctx* ctx, float* d_latents, const uint16_t* d_cond2, int n_objects, int steps,
                          float guidance_scale, float shift, int uncond_uniform, void* stream) {
    NEED_MODEL("r3g_flow_sample_batch");
    if (!d_latents || !d_cond2 || steps < 1 || n_objects < 1) return fail(R3G_ERR_INVALID, "r3g_flow_sample_batch: bad argument");
    return flow_sample(m, d_latents, d_cond2, n_objects, linspace_sigmas(steps, shift), guidance_scale, uncond_uniform,
                       (hipStream_t)stream);
}

int r3g_flow_sample_sigmas(r3g_ctx* ctx, float* d_latents, const uint16_t* d_cond2, int n_objects, const float* sigmas, int n_sigmas,
                           float guidance_scale, int uncond_uniform, void* stream) {
    NEED_MODEL("r3g_flow_sample_sigmas");
    if (!d_latents || !d_cond2 || !sigmas || n_sigmas < 2 || n_objects < 1)
        return fail(R3G_ERR_INVALID, "r3g_flow_sample_sigmas: bad argument");
    for (int i = 0; i < n_sigmas; ++i)
        if (!std::isfinite(sigmas[i])) return fail(R3G_ERR_INVALID, "r3g_flow_sample_sigmas: sigmas[%d] is not finite", i);
    return flow_sample(m, d_latents, d_cond2, n_objects, std::vector<float>(sigmas, sigmas + n_sigmas), guidance_scale, uncond_uniform,
                       (hipStream_t)stream);
}

int r3g_vae_decode(r3g_ctx* ctx, const float* d_latents, float* d_z_out, void* stream) {
    NEED_MODEL("r3g_vae_decode");
    if (!d_latents) return fail(R3G_ERR_INVALID, "r3g_vae_decode: null argument");
    R3G_RC(vae_decode(*m, d_latents, (hipStream_t)stream));
    if (d_z_out)
        R3G_TRY(hipMemcpyAsync(d_z_out, m->z, (size_t)m->c.vae_num_latents * m->W * 4, hipMemcpyDeviceToDevice,
                               (hipStream_t)stream));
    return R3G_OK;
}

int r3g_grid_query(r3g_ctx* ctx, double bound, int octree_resolution, float* d_grid, int64_t start, int64_t count,
                   void* stream) {
    NEED_MODEL("r3g_grid_query");
    if (!d_grid || octree_resolution < 1) return fail(R3G_ERR_INVALID, "r3g_grid_query: bad argument");
    return grid_query(*m, bound, octree_resolution, d_grid, start, count, (hipStream_t)stream);
}

int r3g_grid_query_points(r3g_ctx* ctx, double bound, int octree_resolution, const int32_t* d_idx, int64_t count, float* d_values,
                          void* stream) {
    NEED_MODEL("r3g_grid_query_points");
    if (octree_resolution < 1 || octree_resolution > 1289 || count < 0 || (count && (!d_idx || !d_values)))
        return fail(R3G_ERR_INVALID, "r3g_grid_query_points: bad argument");
    if (g_geo_fp8) return fail(R3G_ERR_INVALID, "r3g_grid_query_points: not available with option geo_fp8");
    if (count == 0) return R3G_OK;
    return grid_query(*m, bound, octree_resolution, d_values, 0, count, (hipStream_t)stream, d_idx, false);
}

// levels(R, min_resolution): halve while even and the half is >= min_resolution; coarsest first
static std::vector<int> hier_levels(int R, int min_resolution) {
    std::vector<int> l{R};
    while (l.back() % 2 == 0 && l.back() / 2 >= min_resolution) l.push_back(l.back() / 2);
    std::reverse(l.begin(), l.end());
    return l;
}

int r3g_grid_query_hier(r3g_ctx* ctx, double bound, int octree_resolution, double mc_level, double band, int min_resolution,
                        float* d_grid, int64_t* stats, int n_stats, void* stream) {
    NEED_MODEL("r3g_grid_query_hier");
    const int R = octree_resolution;
    if (!d_grid || R < 1 || R > 1289 || min_resolution < 1 || !(band >= 0.0) || (stats && n_stats < 0))
        return fail(R3G_ERR_INVALID, "r3g_grid_query_hier: bad argument");
    if ((uintptr_t)d_grid % 16) return fail(R3G_ERR_INVALID, "r3g_grid_query_hier: d_grid must be 16-byte aligned");
    if (g_geo_fp8) return fail(R3G_ERR_INVALID, "r3g_grid_query_hier: not available with option geo_fp8");
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t s = (hipStream_t)stream;
    const std::vector<int> lv = hier_levels(R, min_resolution);
    const int L = (int)lv.size();
    if (stats && n_stats < 4 + 2 * L) return fail(R3G_ERR_INVALID, "r3g_grid_query_hier: stats needs %d slots", 4 + 2 * L);
    auto pts = [](int r) { return (int64_t)(r + 1) * (r + 1) * (r + 1); };
    std::vector<int64_t> evaluated((size_t)L, 0);
    int64_t unsafe = 0;
    if (L == 1) {
        // nothing to refine from: the dense decoder (and its query-side cache), exactly as r3g_grid_query
        R3G_RC(grid_query(*m, bound, R, d_grid, 0, pts(R), s));
        evaluated[0] = pts(R);
    } else {
        std::vector<size_t> off((size_t)L, 0);
        size_t need = 0;
        for (int l = 0; l + 1 < L; ++l) {
            off[(size_t)l] = need;
            need += ((size_t)pts(lv[(size_t)l]) * 4 + 255) & ~(size_t)255;
        }
        R3G_RC(m->hier_grids.grow(need, s, "hier level grids"));
        float* G = reinterpret_cast<float*>(m->hier_grids.p + off[0]);
        R3G_RC(grid_query(*m, bound, lv[0], G, 0, pts(lv[0]), s, nullptr, false));
        evaluated[0] = pts(lv[0]);
        for (int l = 1; l < L; ++l) {
            const bool finest = l == L - 1;
            int64_t count = 0;
            R3G_RC(hier_select(c, G, lv[(size_t)l - 1] + 1, mc_level, band, finest ? 1 : 0, &count, s));
            if (count) {
                R3G_RC(m->hier_idx.grow((size_t)count * 4, s, "hier index list"));
                R3G_RC(m->hier_val.grow((size_t)count * 4, s, "hier values"));
                R3G_RC(hier_indices(c, m->hier_idx.as<int32_t>(), s));
                R3G_RC(grid_query(*m, bound, lv[(size_t)l], m->hier_val.as<float>(), 0, count, s, m->hier_idx.as<const int32_t>(), false));
            }
            float* F = finest ? d_grid : reinterpret_cast<float*>(m->hier_grids.p + off[(size_t)l]);
            R3G_RC(hier_merge(c, G, m->hier_val.as<const float>(), F, s));
            evaluated[(size_t)l] = count;
            G = F;
        }
        if (stats) R3G_RC(hier_unsafe_cells(c, d_grid, mc_level, &unsafe, s));
    }
    if (stats) {
        int64_t total = 0;
        for (int l = 0; l < L; ++l) {
            stats[4 + 2 * l] = lv[(size_t)l];
            stats[5 + 2 * l] = evaluated[(size_t)l];
            total += evaluated[(size_t)l];
        }
        stats[0] = L;
        stats[1] = total;
        stats[2] = pts(R);
        stats[3] = unsafe;
    }
    return R3G_OK;
}

// ---- single-op entry points (parity tests call the kernels through the C ABI) ---------------------------
int r3g_op_gemm(const uint16_t* d_a, int64_t lda, const uint16_t* d_w, int64_t ldw, const float* d_bias, void* d_c,
                int64_t ldc, const float* d_gate, int m_, int n_, int k_, int epilogue, int use_lds_dma, void* stream) {
    // The contract of include/r3g.h, checked here and not in gemm_launch: the model's own launches meet it by construction.
    const bool f32_out = epilogue == EPI_RESID_F32 || epilogue == EPI_F32;
    const bool b16_out = epilogue == EPI_BF16 || epilogue == EPI_BF16_GELU_TANH || epilogue == EPI_BF16_GELU_ERF ||
                         epilogue == EPI_RESID_BF16 || epilogue == EPI_RESID_F16;
    if (!f32_out && !b16_out)     // 5 and 9-11 need operands this entry point cannot carry, 7 belongs to r3g_op_gemm_fp8_e4m3
        return fail(R3G_ERR_INVALID, "r3g_op_gemm: epilogue %d is not one of 0, 1, 2, 3, 4, 6, 8", epilogue);
    if (m_ < 0 || n_ < 0 || k_ <= 0 || k_ % 64 || (n_ & 3)) return fail(R3G_ERR_INVALID, "r3g_op_gemm: needs k %% 64 == 0, n %% 4 == 0");
    if (m_ > 0 && n_ > 0) {
        auto misaligned = [](const void* q, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; };
        if (!d_a || !d_w || !d_c) return fail(R3G_ERR_INVALID, "r3g_op_gemm: null operand");
        if ((lda & 7) || (ldw & 7) || lda < k_ || ldw < k_ || misaligned(d_a, 15) || misaligned(d_w, 15))
            return fail(R3G_ERR_INVALID, "r3g_op_gemm: a / w rows are staged 16 bytes at a time: lda, ldw %% 8 == 0, >= k, 16-byte aligned pointers");
        if (misaligned(d_bias, 15) || misaligned(d_gate, 15)) return fail(R3G_ERR_INVALID, "r3g_op_gemm: bias / gate must be 16-byte aligned");
        // the narrow epilogues store 4 consecutive columns at a time: 8 bytes of a 16-bit output, 16 bytes of an fp32 one
        if ((ldc & 3) || ldc < n_ || misaligned(d_c, f32_out ? 15 : 7))
            return fail(R3G_ERR_INVALID, "r3g_op_gemm: needs ldc %% 4 == 0, ldc >= n and c aligned to 4 elements (%d bytes)", f32_out ? 16 : 8);
    }
    GemmArgs p{};
    p.A = d_a; p.lda = lda; p.W = d_w; p.ldw = ldw; p.bias = d_bias; p.C = d_c; p.ldc = ldc; p.gate = d_gate;
    p.M = m_; p.N = n_; p.K = k_; p.epi = epilogue;
    const int staging = g_gemm_glds;      // the process-wide mode (r3g_set_staging) comes back after this launch
    g_gemm_glds = use_lds_dma != 0;
    hipError_t e = gemm_launch(p, 1, (hipStream_t)stream);
    g_gemm_glds = staging;
    if (e != hipSuccess) return hip_fail(e, "r3g_op_gemm");
    return R3G_OK;
}

int r3g_op_gemm_splitk(const uint16_t* d_a, int64_t lda, const uint16_t* d_w, int64_t ldw, const float* d_bias, float* d_c, int64_t ldc,
                       const float* d_gate, int m_, int n_, int k_, int epilogue, float* d_ws, int64_t ws_elems, int* slices,
                       void* stream) {
    if (epilogue != EPI_F32 && epilogue != EPI_RESID_F32) return fail(R3G_ERR_INVALID, "r3g_op_gemm_splitk: fp32 epilogues (3, 4) only");
    if (!d_ws || ws_elems < 1) return fail(R3G_ERR_INVALID, "r3g_op_gemm_splitk: no workspace");
    GemmArgs p{};
    p.A = d_a; p.lda = lda; p.W = d_w; p.ldw = ldw; p.bias = d_bias; p.C = d_c; p.ldc = ldc; p.gate = d_gate;
    p.M = m_; p.N = n_; p.K = k_; p.epi = epilogue;
    p.split_ws = d_ws; p.split_ws_elems = ws_elems;
    hipError_t e = gemm_launch(p, 1, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_gemm_splitk");
    if (slices) *slices = gemm_last_splitk_slices();      // what the launch actually ran with (not the rule's prediction)
    return R3G_OK;
}

int r3g_op_quant_fp8(const uint16_t* d_x, int64_t ldx, int rows, int k_, uint8_t* d_q, int64_t ldq, float* d_scale, void* stream) {
    if (!d_x || !d_q || !d_scale) return fail(R3G_ERR_INVALID, "r3g_op_quant_fp8: null argument");
    hipError_t e = quant_fp8_rows_launch(d_x, ldx, rows, k_, d_q, ldq, d_scale, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_quant_fp8");
    return R3G_OK;
}

// The contract of include/r3g.h for both fp8 entry points, checked here and not in gemm_fp8_launch (the model's own launches meet it
// by construction).  c_elem: bytes per element of C; ldc in elements.  *launch = false: m == 0 or n == 0, nothing to do.
static int op_gemm_fp8_args(const char* who, const uint8_t* d_a8, int64_t lda, const float* d_scale_a, const uint8_t* d_w8, int64_t ldw,
                            const float* d_scale_w, const float* d_bias, const void* d_c, int64_t ldc, int c_elem, const float* d_gate,
                            int m_, int n_, int k_, bool* launch) {
    *launch = false;
    if (m_ < 0 || n_ < 0 || k_ < 256 || k_ % 256 || (n_ & 3)) return fail(R3G_ERR_INVALID, "%s: needs m, n >= 0, k >= 256, k %% 256 == 0, n %% 4 == 0", who);
    if (m_ == 0 || n_ == 0) return R3G_OK;
    auto misaligned = [](const void* q, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; };
    if (!d_a8 || !d_w8 || !d_scale_a || !d_scale_w || !d_c) return fail(R3G_ERR_INVALID, "%s: null argument", who);
    if ((lda & 15) || (ldw & 15) || lda < k_ || ldw < k_ || misaligned(d_a8, 15) || misaligned(d_w8, 15))
        return fail(R3G_ERR_INVALID, "%s: a8 / w8 rows are staged 16 bytes at a time: lda, ldw %% 16 == 0, >= k, 16-byte aligned pointers", who);
    if (misaligned(d_scale_w, 15) || misaligned(d_scale_a, 3)) return fail(R3G_ERR_INVALID, "%s: scale_w must be 16-byte, scale_a 4-byte aligned", who);
    if (misaligned(d_bias, 15) || misaligned(d_gate, 15)) return fail(R3G_ERR_INVALID, "%s: bias / gate must be 16-byte aligned", who);
    if ((ldc & 3) || ldc < n_ || misaligned(d_c, (uintptr_t)(4 * c_elem - 1)))
        return fail(R3G_ERR_INVALID, "%s: needs ldc %% 4 == 0, ldc >= n and c aligned to 4 elements (%d bytes)", who, 4 * c_elem);
    if ((int64_t)m_ * lda >= (1ll << 32) || (int64_t)n_ * ldw >= (1ll << 32)) return fail(R3G_ERR_INVALID, "%s: m * lda and n * ldw must stay below 2^32", who);
    *launch = true;
    return R3G_OK;
}

int r3g_op_gemm_fp8(const uint8_t* d_a8, int64_t lda, const float* d_scale_a, const uint8_t* d_w8, int64_t ldw,
                    const float* d_scale_w, const float* d_bias, void* d_c, int64_t ldc, const float* d_gate, int m_, int n_,
                    int k_, int epilogue, void* stream) {
    const bool f32_out = epilogue == EPI_RESID_F32;
    if (!f32_out && epilogue != EPI_BF16 && epilogue != EPI_BF16_GELU_TANH && epilogue != EPI_BF16_GELU_ERF && epilogue != EPI_RESID_BF16)
        return fail(R3G_ERR_INVALID, "r3g_op_gemm_fp8: epilogue %d is not one of 0, 1, 2, 3, 6", epilogue);   // 7: r3g_op_gemm_fp8_e4m3
    bool launch = false;
    R3G_RC(op_gemm_fp8_args("r3g_op_gemm_fp8", d_a8, lda, d_scale_a, d_w8, ldw, d_scale_w, d_bias, d_c, ldc, f32_out ? 4 : 2, d_gate, m_, n_, k_, &launch));
    if (!launch) return R3G_OK;
    GemmArgs p{};
    p.A = reinterpret_cast<const uint16_t*>(d_a8); p.lda = lda; p.W = reinterpret_cast<const uint16_t*>(d_w8); p.ldw = ldw;
    p.bias = d_bias; p.C = d_c; p.ldc = ldc; p.gate = d_gate;
    p.M = m_; p.N = n_; p.K = k_; p.epi = epilogue;
    hipError_t e = gemm_fp8_launch(p, d_scale_a, d_scale_w, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_gemm_fp8");
    return R3G_OK;
}

int r3g_op_gemm_fp8_e4m3(const uint8_t* d_a8, int64_t lda, const float* d_scale_a, const uint8_t* d_w8, int64_t ldw,
                         const float* d_scale_w, const float* d_bias, uint8_t* d_c8, int64_t ldc_bytes, float out_scale, int m_, int n_,
                         int k_, void* stream) {
    if (!(out_scale > 0.f) || !std::isfinite(out_scale)) return fail(R3G_ERR_INVALID, "r3g_op_gemm_fp8_e4m3: out_scale must be positive and finite");
    bool launch = false;
    R3G_RC(op_gemm_fp8_args("r3g_op_gemm_fp8_e4m3", d_a8, lda, d_scale_a, d_w8, ldw, d_scale_w, d_bias, d_c8, ldc_bytes, 1, nullptr, m_, n_, k_, &launch));
    if (!launch) return R3G_OK;
    GemmArgs p{};
    p.A = reinterpret_cast<const uint16_t*>(d_a8); p.lda = lda; p.W = reinterpret_cast<const uint16_t*>(d_w8); p.ldw = ldw;
    p.bias = d_bias; p.C = d_c8; p.ldc = ldc_bytes;
    p.M = m_; p.N = n_; p.K = k_; p.epi = EPI_FP8_GELU_ERF;
    p.out_inv_scale = 1.0f / out_scale;
    hipError_t e = gemm_fp8_launch(p, d_scale_a, d_scale_w, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_gemm_fp8_e4m3");
    return R3G_OK;
}

int r3g_op_attention(const uint16_t* d_q, const uint16_t* d_k, const uint16_t* d_vt, uint16_t* d_o, int batch, int heads,
                     int lq, int lq_pad, int lk, int lk_pad, int shared_kv, int use_lds_dma, void* stream) {
    AttnArgs p{};
    p.Q = d_q; p.K = d_k; p.Vt = d_vt; p.O = d_o; p.ldo = (int64_t)heads * 64; p.strideO = (int64_t)lq * heads * 64;
    p.B = batch; p.H = heads; p.Lq = lq; p.Lq_pad = lq_pad; p.Lk = lk; p.Lk_pad = lk_pad;
    p.kv_batch_stride_zero = shared_kv; p.scale = 0.125f;
    const int staging = g_attn_glds;
    g_attn_glds = use_lds_dma != 0;
    hipError_t e = attention_launch(p, (hipStream_t)stream);
    g_attn_glds = staging;
    if (e != hipSuccess) return hip_fail(e, "r3g_op_attention");
    return R3G_OK;
}

int r3g_op_kv_select(const uint16_t* d_q, int lq, int lq_pad, const uint16_t* d_k, int lk, int lk_pad, int heads, int group, int stride,
                     int topk, int32_t* d_idx, void* stream) {
    if (!d_q || !d_k || !d_idx) return fail(R3G_ERR_INVALID, "r3g_op_kv_select: null argument");
    hipError_t e = kvsel_select_launch(d_q, lq, lq_pad, d_k, lk, lk_pad, heads, group, stride, topk, d_idx, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_kv_select (needs group % 256 == 0, stride >= 1, 1 <= topk <= lk <= 15360)");
    return R3G_OK;
}

int r3g_op_kv_gather(const uint16_t* d_k, const uint16_t* d_vt, int lk, int lk_pad, int heads, const int32_t* d_idx, int groups, int topk,
                     uint16_t* d_k_out, uint16_t* d_vt_out, void* stream) {
    if (!d_k || !d_vt || !d_idx || !d_k_out || !d_vt_out || lk < 1 || heads < 1) return fail(R3G_ERR_INVALID, "r3g_op_kv_gather: bad argument");
    hipStream_t s = (hipStream_t)stream;
    DevBuf tmp;      // the row-major copy of V the model keeps per object: here per call (a test hook; synchronous)
    R3G_RC(tmp.grow(2 * (size_t)heads * lk * 64, s, "r3g_op_kv_gather row-major V"));
    uint16_t* v = tmp.as<uint16_t>();
    hipError_t e = kvsel_vrows_launch(d_vt, lk, lk_pad, heads, v, s);
    if (e == hipSuccess) e = kvsel_gather_launch(d_k, v, lk, lk_pad, heads, d_idx, groups, topk, d_k_out, d_vt_out, s);
    const hipError_t e2 = hipStreamSynchronize(s);      // (before tmp goes)
    if (e != hipSuccess) return hip_fail(e, "r3g_op_kv_gather");
    if (e2 != hipSuccess) return hip_fail(e2, "r3g_op_kv_gather");
    return R3G_OK;
}

int r3g_op_geo_tail(const uint16_t* d_cat, const uint16_t* d_x0, int n, int hidden, const uint16_t* d_w_proj, const float* d_b_proj,
                    const float* d_ln3_w, const float* d_ln3_b, const uint16_t* d_w_fc, const float* d_b_fc, const uint16_t* d_w_fp,
                    const float* d_b_fp, const float* d_lnpost_w, const float* d_lnpost_b, const float* d_out_w, float out_b, float* d_logits,
                    void* stream) {
    if (!d_cat || !d_x0 || !d_w_proj || !d_w_fc || !d_w_fp || !d_logits || n < 1 || !geo_tail_supported(GEO_TAIL_WIDTH, hidden))
        return fail(R3G_ERR_INVALID, "r3g_op_geo_tail: bad argument (width 256, hidden 256 | 512 | 1024, n >= 1)");
    hipStream_t s = (hipStream_t)stream;
    DevBuf tmp;      // the fragment stream the model keeps per grid query: here per call (a test hook; synchronous)
    R3G_RC(tmp.grow(geo_tail_packed_bytes(hidden), s, "r3g_op_geo_tail fragments"));
    void* packed = tmp.p;
    hipError_t e = geo_tail_pack_launch(d_w_proj, 256, d_w_fc, 256, d_w_fp, hidden, hidden, packed, s);
    if (e == hipSuccess) {
        GeoTailArgs ta{};
        ta.cat = d_cat; ta.ld_cat = 256; ta.x0 = d_x0; ta.ld_x0 = 256; ta.packed = packed;
        ta.b_proj = d_b_proj; ta.ln3_w = d_ln3_w; ta.ln3_b = d_ln3_b; ta.b_fc = d_b_fc; ta.b_fp = d_b_fp;
        ta.lnp_w = d_lnpost_w; ta.lnp_b = d_lnpost_b; ta.out_w = d_out_w; ta.out_b = out_b;
        ta.hidden = hidden; ta.n = n; ta.out = d_logits;
        e = geo_tail_launch(ta, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s);      // (before tmp goes)
    if (e != hipSuccess) return hip_fail(e, "r3g_op_geo_tail");
    if (e2 != hipSuccess) return hip_fail(e2, "r3g_op_geo_tail");
    return R3G_OK;
}

// ---- the row kernels (LayerNorm, ln_dot, qkv_split, GroupNorm, softmax rows, GEGLU, SwiGLU), one launch each.  As in r3g_op_gemm the
// contract of include/r3g.h is checked HERE: the model's own launches meet it by construction and the launchers check only part of it.
static bool op_misaligned(const void* q, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; }

int r3g_op_layernorm(const void* d_x, int x_format, int64_t ldx, int64_t x_batch_stride, uint16_t* d_y, int64_t ldy, int64_t y_batch_stride,
                     uint8_t* d_y8, int64_t ldy8, float* d_y_scale, const float* d_w, const float* d_b, const float* d_scale,
                     const float* d_shift, int64_t mod_stride, int seg2_row0, int seg2_row1, const float* d_scale2, const float* d_shift2,
                     int rows, int c, int rows_per_batch, float eps, void* stream) {
    const char* bad = nullptr;
    const bool fp8 = d_y8 != nullptr;
    const bool seg2 = seg2_row1 > seg2_row0;
    const bool batched = rows_per_batch >= 1 && rows > rows_per_batch;
    // the row-in-registers kernel (float4 / uint2 accesses) or, for f32 rows only, the scalar one (layernorm_launch's rule)
    const bool vec = x_format != 0 || (c % 256 == 0 && (ldx & 3) == 0 && (fp8 || (ldy & 3) == 0));
    if (rows < 1 || rows_per_batch < 1) bad = "rows >= 1 and rows_per_batch >= 1";
    else if (c < 64 || c % 64 || c > 2048) bad = "c % 64 == 0, 64 <= c <= 2048";
    else if (x_format < 0 || x_format > 2 || (x_format && c % 256)) bad = "x_format 0 | 1 | 2, the 16-bit formats with c % 256 == 0";
    else if (!d_x || (fp8 ? (d_y != nullptr || !d_y_scale) : !d_y)) bad = "x and exactly one of y | (y8 and y_scale)";
    else if (ldx < c || x_batch_stride < 0 || mod_stride < 0) bad = "ldx >= c, batch and modulation strides >= 0";
    else if (seg2 && (!d_scale2 || !d_shift2)) bad = "seg2 rows need scale2 and shift2";
    else if (fp8 && (c % 256 || !vec || ldy8 < c || (ldy8 & 3) || op_misaligned(d_y8, 3) || batched || x_batch_stride || y_batch_stride || ldy))
        bad = "the e4m3 output indexes y8 / y_scale by the launch row: c % 256 == 0, vector rows, ldy8 % 4 == 0, ldy8 >= c, one batch "
              "(rows_per_batch >= rows), x_batch_stride = y_batch_stride = ldy = 0";
    else if (!fp8 && (ldy < c || y_batch_stride < 0 || (batched && y_batch_stride < (int64_t)(rows_per_batch - 1) * ldy + c)))
        bad = "ldy >= c, and y batches that do not overlap";
    else if (vec && ((ldx & 3) || (x_batch_stride & 3) || op_misaligned(d_x, x_format ? 7 : 15)))
        bad = "four x elements per access: ldx % 4 == 0, x_batch_stride % 4 == 0, x aligned to four elements";
    else if (vec && !fp8 && ((ldy & 3) || (y_batch_stride & 3) || op_misaligned(d_y, 7)))
        bad = "four y elements per store: ldy % 4 == 0, y_batch_stride % 4 == 0, y 8-byte aligned";
    else if (vec && ((mod_stride & 3) || op_misaligned(d_w, 15) || op_misaligned(d_b, 15) || op_misaligned(d_scale, 15) ||
                     op_misaligned(d_shift, 15) || op_misaligned(d_scale2, 15) || op_misaligned(d_shift2, 15)))
        bad = "w, b, scale, shift, scale2, shift2 16-byte aligned, mod_stride % 4 == 0";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_layernorm: needs %s", bad);
    LnArgs p{};
    p.x = static_cast<const float*>(d_x); p.ldx = ldx; p.x_bf16 = x_format; p.y = d_y; p.ldy = ldy;
    p.y8 = d_y8; p.ldy8 = ldy8; p.y_scale = d_y_scale;
    p.x_batch_stride = x_batch_stride; p.y_batch_stride = y_batch_stride;
    p.w = d_w; p.b = d_b; p.scale = d_scale; p.shift = d_shift; p.mod_stride = mod_stride;
    p.seg2_row0 = seg2_row0; p.seg2_row1 = seg2_row1; p.scale2 = d_scale2; p.shift2 = d_shift2;
    p.rows = rows; p.C = c; p.rows_per_batch = rows_per_batch; p.eps = eps;
    hipError_t e = layernorm_launch(p, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_layernorm");
    return R3G_OK;
}

int r3g_op_ln_dot(const void* d_x, int x_bf16, int64_t ldx, int rows, int c, int do_ln, const float* d_lnw, const float* d_lnb, float eps,
                  const float* d_w, float b, float* d_out, void* stream) {
    const char* bad = nullptr;
    const bool vec = x_bf16 != 0 || (c % 256 == 0 && (ldx & 3) == 0);      // ln_dot_launch's rule
    if (rows < 1) bad = "rows >= 1";
    else if (c < 64 || c % 64 || c > 2048) bad = "c % 64 == 0, 64 <= c <= 2048";
    else if (x_bf16 < 0 || x_bf16 > 1 || (x_bf16 && c % 256)) bad = "x_bf16 0 | 1, bf16 rows with c % 256 == 0";
    else if (!d_x || !d_w || !d_out) bad = "x, w and out";
    else if (do_ln && d_lnw && !d_lnb) bad = "lnb wherever lnw is given (the kernels load both)";
    else if (ldx < c) bad = "ldx >= c";
    else if (vec && ((ldx & 3) || op_misaligned(d_x, x_bf16 ? 7 : 15) || op_misaligned(d_w, 15) ||
                     (do_ln && d_lnw && (op_misaligned(d_lnw, 15) || op_misaligned(d_lnb, 15)))))
        bad = "four elements per access: ldx % 4 == 0, x aligned to four elements, w / lnw / lnb 16-byte aligned";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_ln_dot: needs %s", bad);
    hipError_t e = ln_dot_launch(static_cast<const float*>(d_x), ldx, rows, c, do_ln, d_lnw, d_lnb, eps, d_w, b, d_out, (hipStream_t)stream, x_bf16);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_ln_dot");
    return R3G_OK;
}

int r3g_op_qkv_split(const uint16_t* d_src, int64_t ld, int64_t src_batch_stride, int q_off, int k_off, int v_off, int head_stride,
                     uint16_t* d_q, uint16_t* d_k, uint16_t* d_vt, int lq_pad, int lk_pad, int dst_row0, int batch, int heads, int l,
                     int norm, const float* d_qw, const float* d_qb, const float* d_kw, const float* d_kb, float eps, float q_scale,
                     void* stream) {
    const char* bad = nullptr;
    const int offs[3] = {q_off, k_off, v_off};
    const void* dst[3] = {d_q, d_k, d_vt};
    bool any = false, cols_ok = true, pairs_ok = true;
    for (int i = 0; i < 3; ++i) {
        if ((offs[i] >= 0) != (dst[i] != nullptr)) pairs_ok = false;
        if (offs[i] >= 0) {
            any = true;
            if (heads >= 1 && head_stride >= 0 && (int64_t)offs[i] + (int64_t)(heads - 1) * head_stride + 64 > ld) cols_ok = false;
        }
    }
    if (l < 1 || batch < 1 || heads < 1 || batch > 65535 || heads > 65535) bad = "l >= 1, 1 <= batch, heads <= 65535";
    else if (!d_src || !any || !pairs_ok) bad = "src, and for each of q, k, v either a column offset >= 0 with its destination or -1 with null";
    else if (head_stride < 0 || src_batch_stride < 0 || !cols_ok) bad = "every head's 64 columns inside [0, ld)";
    else if (norm < QKN_NONE || norm > QKN_LAYERNORM) bad = "norm 0 | 1 | 2";
    else if (dst_row0 < 0 || dst_row0 % 64) bad = "dst_row0 % 64 == 0, >= 0";
    else if (lq_pad < 0 || lk_pad < 0 || lq_pad % 128 || lk_pad % 64) bad = "lq_pad % 128 == 0, lk_pad % 64 == 0";
    else if (d_q && (int64_t)dst_row0 + l > lq_pad) bad = "dst_row0 + l <= lq_pad";
    else if ((d_k || d_vt) && (int64_t)dst_row0 + l > lk_pad) bad = "dst_row0 + l <= lk_pad";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_qkv_split: needs %s", bad);
    QkvSplitArgs p{};
    p.src = d_src; p.ld = ld; p.src_batch_stride = src_batch_stride;
    p.q_off = q_off; p.k_off = k_off; p.v_off = v_off; p.head_stride = head_stride;
    p.Q = d_q; p.K = d_k; p.Vt = d_vt; p.Lq_pad = lq_pad; p.Lk_pad = lk_pad; p.dst_row0 = dst_row0;
    p.B = batch; p.H = heads; p.L = l; p.norm = norm; p.qw = d_qw; p.qb = d_qb; p.kw = d_kw; p.kb = d_kb; p.eps = eps; p.q_scale = q_scale;
    hipError_t e = qkv_split_launch(p, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_qkv_split");
    return R3G_OK;
}

int r3g_op_group_norm(const float* d_x, int rows, int c, int groups, const float* d_gamma, const float* d_beta, float eps, int do_silu,
                      uint16_t* d_y, int nb, const float* d_addv, int64_t add_stride, void* stream) {
    const char* bad = nullptr;
    if (rows < 1 || nb < 1 || nb > 65535) bad = "rows >= 1, 1 <= nb <= 65535";
    else if (c < 4 || c % 4 || c > 3072 || groups < 1 || groups > 256 || c % groups) bad = "c % 4 == 0, c <= 3072, 1 <= groups <= 256, c % groups == 0";
    else if (!d_x || !d_gamma || !d_beta || !d_y) bad = "x, gamma, beta and y";
    else if (op_misaligned(d_x, 15) || op_misaligned(d_gamma, 15) || op_misaligned(d_beta, 15) || op_misaligned(d_y, 7))
        bad = "x, gamma, beta 16-byte aligned, y 8-byte aligned (four channels per access)";
    else if (d_addv && (add_stride < c || (add_stride & 3) || op_misaligned(d_addv, 15))) bad = "addv 16-byte aligned, add_stride % 4 == 0, add_stride >= c";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_group_norm: needs %s", bad);
    hipStream_t s = (hipStream_t)stream;
    DevBuf tmp;      // the workspace the UNet keeps per model: here per call (a test hook; synchronous)
    R3G_RC(tmp.grow(sizeof(double) * (size_t)nb * ((size_t)group_norm_blocks(rows) * groups * 2 + groups), s, "r3g_op_group_norm partial sums"));
    hipError_t e = group_norm_launch(d_x, rows, c, groups, d_gamma, d_beta, eps, do_silu, d_y, tmp.as<double>(), s, nb, d_addv, add_stride);
    const hipError_t e2 = hipStreamSynchronize(s);      // (before tmp goes)
    if (e != hipSuccess) return hip_fail(e, "r3g_op_group_norm");
    if (e2 != hipSuccess) return hip_fail(e2, "r3g_op_group_norm");
    return R3G_OK;
}

int r3g_op_softmax_rows(const float* d_s, int64_t lds, uint16_t* d_p, int64_t ldp, int rows, int n, float scale, void* stream) {
    const char* bad = nullptr;
    if (rows < 1 || n < 4 || n % 4) bad = "rows >= 1, n >= 4, n % 4 == 0";
    else if (!d_s || !d_p) bad = "s and p";
    else if (lds < n || ldp < n || (lds & 3) || (ldp & 3) || op_misaligned(d_s, 15) || op_misaligned(d_p, 7))
        bad = "four elements per access: lds, ldp % 4 == 0 and >= n, s 16-byte and p 8-byte aligned";
    else if (!(scale > 0.f) || !(scale <= 3.0e38f)) bad = "a finite scale > 0 (the kernel scales the maximum of the scores, not the scaled scores)";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_softmax_rows: needs %s", bad);
    hipError_t e = softmax_rows_launch(d_s, lds, d_p, ldp, rows, n, scale, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_softmax_rows");
    return R3G_OK;
}

static const char* glu_contract(const uint16_t* d_in, int64_t ldi, uint16_t* d_out, int64_t ldo, int rows, int f) {
    if (rows < 1 || f < 8 || f % 8) return "rows >= 1, f >= 8, f % 8 == 0";
    if (!d_in || !d_out) return "in and out";
    if (ldi < 2 * (int64_t)f || ldo < f || (ldi & 7) || (ldo & 7) || op_misaligned(d_in, 15) || op_misaligned(d_out, 15))
        return "eight elements per access: ldi >= 2 f, ldo >= f, ldi % 8 == 0, ldo % 8 == 0, 16-byte aligned pointers";
    return nullptr;
}

int r3g_op_geglu(const uint16_t* d_in, int64_t ldi, uint16_t* d_out, int64_t ldo, int rows, int f, void* stream) {
    if (const char* bad = glu_contract(d_in, ldi, d_out, ldo, rows, f)) return fail(R3G_ERR_INVALID, "r3g_op_geglu: needs %s", bad);
    hipError_t e = geglu_launch(d_in, ldi, d_out, ldo, rows, f, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_geglu");
    return R3G_OK;
}

int r3g_op_swiglu(const uint16_t* d_in, int64_t ldi, uint16_t* d_out, int64_t ldo, int rows, int f, void* stream) {
    if (const char* bad = glu_contract(d_in, ldi, d_out, ldo, rows, f)) return fail(R3G_ERR_INVALID, "r3g_op_swiglu: needs %s", bad);
    hipError_t e = swiglu_launch(d_in, ldi, d_out, ldo, rows, f, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_swiglu");
    return R3G_OK;
}

// ---- the small kernels of the sampler step and of input staging (GEMV, embeddings, Euler updates, casts and copies), one launch each.
// The contract of include/r3g.h is checked here, as above; tests/test_vec_kernels_gpu.py drives them.
static const char* gemv_contract(const float* d_x, int b, int k, int max_b) {
    if (!d_x) return "x";
    if (b < 1 || b > max_b) return max_b == 8 ? "1 <= b <= 8" : "1 <= b <= 2";
    if (k < 8 || k % 8 || (int64_t)b * k * 4 > 65536) return "k % 8 == 0, k >= 8, b * k * 4 <= 65536 (the inputs are held in LDS)";
    return nullptr;
}

static const char* gemv_matrix_contract(const void* w, int64_t ldw, int k, int n) {
    if (!w || n < 1) return "a matrix and n >= 1";
    if (ldw < k || (ldw & 7) || op_misaligned(w, 15)) return "16 bytes of w per lane: ldw % 8 == 0, ldw >= k, w 16-byte aligned";
    return nullptr;
}

int r3g_op_gemv(const float* d_x, int b, int k, const uint16_t* d_w, int64_t ldw, const float* d_bias, float* d_y, int n, int silu_in,
                int silu_out, void* stream) {
    const char* bad = gemv_contract(d_x, b, k, 8);
    if (!bad) bad = gemv_matrix_contract(d_w, ldw, k, n);
    if (!bad && !d_y) bad = "y";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_gemv: needs %s", bad);
    hipError_t e = gemv_launch(d_x, b, k, d_w, ldw, d_bias, d_y, n, silu_in, silu_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_gemv");
    return R3G_OK;
}

int r3g_op_gemv_multi(const float* d_x, int b, int k, const void* const* w, const void* const* bias, const int64_t* ldw, const int* n,
                      const int64_t* out_off, int njobs, float* d_y, int silu_in, void* stream) {
    const char* bad = gemv_contract(d_x, b, k, 2);
    if (!bad && (!w || !ldw || !n || !out_off || !d_y)) bad = "the host arrays w, ldw, n, out_off and y";
    if (!bad && (njobs < 1 || njobs > 65535)) bad = "1 <= njobs <= 65535";
    for (int j = 0; !bad && j < njobs; ++j) {
        bad = gemv_matrix_contract(w[j], ldw[j], k, n[j]);
        if (!bad && out_off[j] < 0) bad = "out_off >= 0";
    }
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_gemv_multi: needs %s", bad);
    std::vector<GemvJob> jobs;
    for (int j = 0; j < njobs; ++j)
        jobs.push_back(GemvJob{static_cast<const uint16_t*>(w[j]), bias ? static_cast<const float*>(bias[j]) : nullptr, ldw[j], n[j], out_off[j]});
    hipStream_t s = (hipStream_t)stream;
    DevBuf table;      // the table the model builds once per checkpoint: here per call (a test hook; synchronous)
    R3G_RC(table.grow(jobs.size() * sizeof(GemvJob), s, "r3g_op_gemv_multi jobs"));
    R3G_TRY(hipMemcpy(table.p, jobs.data(), jobs.size() * sizeof(GemvJob), hipMemcpyHostToDevice));
    hipError_t e = gemv_multi_launch(d_x, b, k, table.as<GemvJob>(), njobs, d_y, silu_in, s);
    const hipError_t e2 = hipStreamSynchronize(s);      // (before the table goes)
    if (e != hipSuccess) return hip_fail(e, "r3g_op_gemv_multi");
    if (e2 != hipSuccess) return hip_fail(e2, "r3g_op_gemv_multi");
    return R3G_OK;
}

int r3g_op_timestep_embedding(const float* d_t, float t_scalar, int b, float time_factor, float* d_out, void* stream) {
    if (b < 1 || !d_out) return fail(R3G_ERR_INVALID, "r3g_op_timestep_embedding: needs b >= 1 and out");
    hipError_t e = timestep_embedding_launch(d_t, t_scalar, b, time_factor, d_out, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_timestep_embedding");
    return R3G_OK;
}

static const char* fourier_contract(const uint16_t* d_out, int r, int num_freqs) {
    if (!d_out) return "out";
    if (r < 1) return "r >= 1";
    if (num_freqs < 0 || 3 + 6 * num_freqs > 64) return "0 <= num_freqs, 3 + 6 num_freqs <= 64";
    return nullptr;
}

int r3g_op_fourier_grid(uint16_t* d_out, int64_t start, int count, int r, double bound, int num_freqs, int include_pi, void* stream) {
    const char* bad = fourier_contract(d_out, r, num_freqs);
    if (!bad && (start < 0 || count < 1)) bad = "start >= 0, count >= 1";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_fourier_grid: needs %s", bad);
    hipError_t e = fourier_grid_launch(d_out, start, count, r, bound, num_freqs, include_pi, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_fourier_grid");
    return R3G_OK;
}

int r3g_op_fourier_points(uint16_t* d_out, const int32_t* d_list, int count, int rows, int r, double bound, int num_freqs, int include_pi,
                          void* stream) {
    const char* bad = fourier_contract(d_out, r, num_freqs);
    if (!bad && (count < 1 || rows < 1 || count > rows)) bad = "1 <= count <= rows";
    if (!bad && !d_list) bad = "list";
    if (!bad && op_misaligned(d_out, 15)) bad = "out 16-byte aligned (eight channels per store)";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_fourier_points: needs %s", bad);
    hipError_t e = fourier_points_launch(d_out, d_list, count, rows, r, bound, num_freqs, include_pi, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_fourier_points");
    return R3G_OK;
}

int r3g_op_cfg_euler(float* d_lat, const float* d_v2, int64_t n, float guidance, float dsigma, void* stream) {
    if (!d_lat || !d_v2 || n < 1) return fail(R3G_ERR_INVALID, "r3g_op_cfg_euler: needs lat, v2 and n >= 1");
    hipError_t e = cfg_euler_launch(d_lat, d_v2, n, guidance, dsigma, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_cfg_euler");
    return R3G_OK;
}

int r3g_op_euler_step(float* d_lat, const float* d_v, int64_t n, float dsigma, void* stream) {
    if (!d_lat || !d_v || n < 1) return fail(R3G_ERR_INVALID, "r3g_op_euler_step: needs lat, v and n >= 1");
    hipError_t e = euler_step_launch(d_lat, d_v, n, dsigma, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_euler_step");
    return R3G_OK;
}

int r3g_op_nonfinite_flag(const float* d_x, int64_t n, int* d_flag, void* stream) {
    if (!d_x || !d_flag || n < 1) return fail(R3G_ERR_INVALID, "r3g_op_nonfinite_flag: needs x, flag and n >= 1");
    hipError_t e = nonfinite_flag_launch(d_x, n, d_flag, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_nonfinite_flag");
    return R3G_OK;
}

int r3g_op_cast_pad(const float* d_in, int64_t ldi, uint16_t* d_out, int64_t ldo, int rows, int c, int cpad, float scale, void* stream) {
    const char* bad = nullptr;
    if (!d_in || !d_out) bad = "in and out";
    else if (rows < 1 || c < 1 || cpad < c) bad = "rows >= 1, 1 <= c <= cpad";
    else if (ldi < c || ldo < cpad) bad = "ldi >= c, ldo >= cpad";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_cast_pad: needs %s", bad);
    hipError_t e = cast_pad_launch(d_in, ldi, d_out, ldo, rows, c, cpad, scale, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_cast_pad");
    return R3G_OK;
}

int r3g_op_fill_rows(float* d_dst, int64_t ld, int rows, int c, const float* d_vals, void* stream) {
    if (!d_dst || !d_vals || rows < 1 || c < 1 || ld < c) return fail(R3G_ERR_INVALID, "r3g_op_fill_rows: needs dst, vals, rows >= 1, c >= 1, ld >= c");
    hipError_t e = fill_rows_launch(d_dst, ld, rows, c, d_vals, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_fill_rows");
    return R3G_OK;
}

int r3g_op_add_rows(float* d_x, int64_t ldx, const float* d_pos, int64_t ldp, int rows, int c, void* stream) {
    if (!d_x || !d_pos || rows < 1 || c < 1 || ldx < c || ldp < c)
        return fail(R3G_ERR_INVALID, "r3g_op_add_rows: needs x, pos, rows >= 1, c >= 1, ldx >= c, ldp >= c");
    hipError_t e = add_rows_launch(d_x, ldx, d_pos, ldp, rows, c, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_add_rows");
    return R3G_OK;
}

int r3g_op_f32_to_bf16(const float* d_in, uint16_t* d_out, int64_t n, void* stream) {
    if (!d_in || !d_out || n < 1) return fail(R3G_ERR_INVALID, "r3g_op_f32_to_bf16: needs in, out and n >= 1");
    hipError_t e = f32_to_bf16_launch(d_in, d_out, n, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_f32_to_bf16");
    return R3G_OK;
}

int r3g_op_patch_rows(const float* d_img, int s, int ps, uint16_t* d_out, int kpad, void* stream) {
    const char* bad = nullptr;
    if (!d_img || !d_out) bad = "img and out";
    else if (s < 1 || ps < 1 || ps > 1024 || s % ps) bad = "s >= 1, 1 <= ps <= 1024, s % ps == 0";
    else if (kpad < 3 * ps * ps) bad = "kpad >= 3 ps^2";
    if (bad) return fail(R3G_ERR_INVALID, "r3g_op_patch_rows: needs %s", bad);
    hipError_t e = im2col_launch(d_img, s, ps, d_out, kpad, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_patch_rows");
    return R3G_OK;
}

int r3g_op_vec_add_inplace(float* d_y, const float* d_x, int n, void* stream) {
    if (!d_y || !d_x || n < 1) return fail(R3G_ERR_INVALID, "r3g_op_vec_add_inplace: needs y, x and n >= 1");
    hipError_t e = vec_add_launch(d_y, d_x, n, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "r3g_op_vec_add_inplace");
    return R3G_OK;
}

int r3g_kv_selection_last(r3g_ctx* ctx, int32_t* d_idx, int64_t capacity, int* groups, int* heads, int* k, void* stream) {
    NEED_MODEL("r3g_kv_selection_last");
    if (!m->kv_last_groups) return fail(R3G_ERR_STATE, "r3g_kv_selection_last: no pass has been evaluated in top-k mode");
    const int64_t count = (int64_t)m->kv_last_groups * m->Hg * m->kv_last_k;
    if (groups) *groups = m->kv_last_groups;
    if (heads) *heads = m->Hg;
    if (k) *k = m->kv_last_k;
    if (d_idx) {
        if (capacity < count) return fail(R3G_ERR_INVALID, "r3g_kv_selection_last: the table has %lld entries, capacity %lld", (long long)count, (long long)capacity);
        R3G_TRY(hipMemcpyAsync(d_idx, m->kv_idx.p, 4 * (size_t)count, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return R3G_OK;
}

int r3g_kv_selection_operands(r3g_ctx* ctx, uint16_t* d_q, int64_t q_capacity, uint16_t* d_k, int64_t k_capacity, int* lq, int* lq_pad,
                              int* lk, int* lk_pad, void* stream) {
    NEED_MODEL("r3g_kv_selection_operands");
    if (!m->kv_last_groups || !m->kv_last_q) return fail(R3G_ERR_STATE, "r3g_kv_selection_operands: no pass has been evaluated in top-k mode");
    if (!m->have_z) return fail(R3G_ERR_STATE, "r3g_kv_selection_operands: r3g_vae_decode has not run");
    const int Nl = m->c.vae_num_latents, Lkp = (int)rup(Nl, 64);
    const int64_t qn = (int64_t)m->Hg * m->kv_last_npad * 64, kn = (int64_t)m->Hg * Lkp * 64;
    if (lq) *lq = m->kv_last_n;
    if (lq_pad) *lq_pad = m->kv_last_npad;
    if (lk) *lk = Nl;
    if (lk_pad) *lk_pad = Lkp;
    if ((d_q && q_capacity < qn) || (d_k && k_capacity < kn)) return fail(R3G_ERR_INVALID, "r3g_kv_selection_operands: capacity too small");
    if (d_q) R3G_TRY(hipMemcpyAsync(d_q, m->kv_last_q, 2 * (size_t)qn, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (d_k) R3G_TRY(hipMemcpyAsync(d_k, m->geoK, 2 * (size_t)kn, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return R3G_OK;
}

int r3g_prof_enable(int on) {
    prof_enable(on != 0);
    return R3G_OK;
}

int r3g_prof_read(int64_t* counts, double* ms, double* work, int n) {
    if (!counts || !ms || !work || n < PC_COUNT) return fail(R3G_ERR_INVALID, "r3g_prof_read: need %d slots", (int)PC_COUNT);
    long long c[PC_COUNT];
    prof_read(c, ms, work);
    for (int i = 0; i < PC_COUNT; ++i) counts[i] = c[i];
    return R3G_OK;
}

int r3g_prof_read_bytes(double* bytes, int n) {
    if (!bytes || n < PC_COUNT) return fail(R3G_ERR_INVALID, "r3g_prof_read_bytes: need %d slots", (int)PC_COUNT);
    prof_read_bytes(bytes);
    return R3G_OK;
}

int r3g_set_option(const char* name, int value) {
    if (!name) return fail(R3G_ERR_INVALID, "r3g_set_option: null name");
    const Option* o = find_option(name);
    // (a refused value or an unknown name starts a new epoch as well; an unknown "geo_kv_*" name does not, like the three known ones)
    if (o ? o->new_epoch : strncmp(name, "geo_kv_", 7) != 0) ++g_option_epoch;
    return store(o, name, value);
}

int r3g_get_option(const char* name, int* value) {
    if (!name || !value) return fail(R3G_ERR_INVALID, "r3g_get_option: null argument");
    const Option* o = find_option(name);
    if (!o) return fail(R3G_ERR_INVALID, "r3g_get_option: unknown option '%s'", name);
    *value = o->slot2 ? *o->slot && *o->slot2 : *o->slot;
    return R3G_OK;
}

const char* r3g_option_name(int index) { return index >= 0 && index < (int)options().size() ? options()[index]->name : nullptr; }

int r3g_set_staging(int use_lds_dma) { return option_store("lds_dma", use_lds_dma); }

}  // extern "C"
