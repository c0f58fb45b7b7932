"""Float64 references and ELEMENT-WISE error bounds for the MFMA kernels (csrc/gemm.hip, csrc/attn.hip), shared by
tests/test_edge_bounds_cpu.py (the bounds are neither vacuous nor unreachable), tests/test_gemm_edges_gpu.py and
tests/test_attention_edges_gpu.py (every tile kernel and attention generation at ragged shapes).

Everything here is plain torch float64 and runs on whatever device the operands live on; nothing needs a GPU.

The bounds are DERIVED from the arithmetic the kernels are written to do, not measured.  u = 2^-24 is the unit roundoff of
float32.  The only margin in them is named where it enters (the factor 2 of E below).

Rounding to a 16-bit type.  A kernel that rounds an fp32 value x' to nearest-even stores a value within HALF A UNIT IN THE LAST
PLACE of x': half_ulp(x') = 2^(floor(log2 |x'|) - p) for a significand of p bits (bf16: p = 8, fp16: p = 11; fp16 subnormals:
2^-25).  If x' is within e of the exact x, the stored value is within half_ulp(|x| + e) + e of x.  That is the form used for every
16-bit output below.  bf16's unit roundoff is 2^-8, not 2^-9: 1 + 2^-8 lies half way between 1 and 1 + 2^-7 and rounds to 1, an
error of 2^-8 (tests/test_edge_bounds_cpu.py::test_the_relative_bf16_unit_is_2_to_the_minus_8).  half_ulp is never above 2^-8 |x'|
(2^-11 |x'| for fp16) and is the tightest bound a correctly rounding kernel meets at every value; a kernel that truncates is off by
up to a whole ulp and fails it.

GEMM.  Operands as the kernel sees them: bf16 a [M][K] and w [N][K], fp32 bias and gate, the old C in its stored type.
    lin = a64 w64^T + bias            t = |a|64 |w|64^T + |bias|            E = 2 K u t
A float32 sum of K products (bf16 x bf16 is exact in float32) and the bias, in any order, errs by at most K u t to first order; the
factor 2 covers whatever the MFMA does inside one 32-deep instruction (its internal alignment of 32 products and the accumulator
is not specified to be a chain of IEEE additions).  That factor is the only margin.
    epilogue 4 (fp32 store)        |c - lin| <= E
    epilogue 3 (fp32 residual)     ref = c0 + gate lin,  e3 = |gate| E + 3 u (|c0| + |gate lin|)     (the rounding of acc + bias, of the
                                   product with the gate, of the sum with the old value)
    epilogue 0 (bf16 store)        |c - lin| <= half_ulp_bf16(|lin| + E) + E
    epilogue 6 (bf16 residual)     |c - ref| <= half_ulp_bf16(|ref| + e3) + e3
    epilogue 8 (fp16 residual)     the same with half_ulp_fp16 (old values far below 65504)
    epilogues 1, 2 (GELU tanh / erf, bf16)   ref = gelu(lin) of the stated flavour in float64.  The kernel evaluates x S(x) at an x
                                   within E of lin: |gelu'| <= 1.13 carries E to the output, the form adds |S error| (|lin| + E), the
                                   product x S one rounding:  eg = 1.13 E + S_ERR (|lin| + E) + 2 u |ref|;  bound half_ulp_bf16(|ref| + eg) + eg.
                                   S_ERR = 1e-3 for the packed-fp16 form ("gelu_pk" 1, the default): the project's own number,
                                   asserted by tests/test_ops_gpu.py::test_gelu_packed_fp16_form_equals_its_emulation.  S_ERR = 1e-6 for
                                   the fp32 forms ("gelu_pk" 0), READ from csrc/gemm_common.h, not measured: the erf form is x times
                                   Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7) evaluated with about ten fp32 operations and two
                                   1-ulp transcendentals on values <= 1 (each <= 2^-23); the tanh form is x / (1 + 2^z), whose error
                                   is S (1 - S) ln 2 |dz| with |dz| <= 3 u |z|, and S (1 - S) |z| <= 0.25.

Attention (head_dim 64).  Float64 softmax from the Q the MFMA actually sees:
  * generations 2 and later (and 7 = 6 | 2): r3g_op_attention hands them plain q, and the kernel re-rounds q * (0.125 log2 e) -- the
    product in float32 -- to bf16 ("a second bf16 rounding", attn2_kernel / attn3_kernel / attn6_kernel); scores are in base 2;
  * generation 1 and the pipelined kernel ("attn_pipelined") keep q and scale the float32 scores by 0.125 log2 e themselves.
ref = sum_j p_j v_j with p_j = 2^(s_j - max s) / sum,   s = sum_j p_j |v_j| per output element.
What the kernels do with P, read in csrc/attn.hip: EVERY generation converts P to bf16 with v_cvt_pk_bf16_f32 (pack_bf16: round to
nearest even), so u_P = 2^-8 (the unit roundoff of bf16's 8-bit significand; a truncating conversion would be 2^-7), and EVERY
generation forms the row sum from the UNROUNDED float32 exponentials (gen 1 / pipelined: psum += p before the packing; gen 2, 6, 9:
sum16(pe); gens 3, 4: ps0), so there is no u_P |ref| term for the sum.  P is rounded relative to a stabiliser that need not be the
maximum (generations 2+ re-stabilise only 8 log2 units above it), which changes nothing: the rounding is relative.
    e_in = u_P s                                              P in bf16
         + eps (s + |ref|)                                    the scores' own float32 error, carried through 2^x into every p_j:
                                                              eps = ln 2 * 2 * 65 u * 2 ts + 2^-22, ts = max_j sum_d |q_d| |k_jd| in log2 units
                                                              (64 products and the stabiliser, the MFMA factor 2 as above, |stabiliser| <= ts;
                                                              2^-22: v_exp_f32 and the rounding of its argument)
         + 2 Lk u s                                           the float32 accumulation of P V, of the GEMM kind (factor 2 as above)
         + (Lk + Lk / 32 + 4) u (s + |ref|)                   the float32 row sum, one rescale per 32-key block at most, reciprocal, product
    |o - ref| <= e_in + half_ulp_bf16(|ref| + e_in)            the bf16 rounding of the output
"""
import math

import torch

U32 = 2.0 ** -24
S_ERR_PK = 1e-3
S_ERR_F32 = 1e-6
U_P = 2.0 ** -8
SM_SCALE32 = None   # float32(0.125 * log2 e) as a python float, set below


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


# the kernel's constant: p.scale * 1.4426950408889634f, both float32 (0.125 is a power of two: the product is exact)
SM_SCALE32 = _f32(1.4426950408889634) * 0.125


def half_ulp(x, fmt):
    """half a unit in the last place of |x| in the 16-bit format (float64 tensor in, float64 tensor out)"""
    p, tiny = {"bf16": (8, 2.0 ** -134), "f16": (11, 2.0 ** -25)}[fmt]
    _, e = torch.frexp(x.abs().double())          # |x| = m 2^e, m in [0.5, 1): floor(log2 |x|) = e - 1
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 1 - p).clamp_min(tiny)


OUT_FMT = {0: "bf16", 1: "bf16", 2: "bf16", 3: "f32", 4: "f32", 6: "bf16", 8: "f16"}
TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
GEMM_EPILOGUES = (0, 1, 2, 3, 4, 6, 8)
GEMM_REFUSED = (7, 9, 10, 11)      # (5 is refused as well; it is never passed: its operands cannot travel through r3g_op_gemm)

# (M, N, K, what the shape is for).  Nothing above 512.  M covers {1, 17, 127, 129, 257}, N {4, 68, 132, 252, 256, 260, 512},
# K {64, 128, 192, 256, 320, 512}.  K = 96 is not here: gemm_args_ok requires K % 64 == 0, so the deep-ring kernel's K % 32 form is
# not admitted through any entry point.
GEMM_SHAPES = (
    (1, 4, 64, "one row, one 4-column group, one k-tile: only the prologue stages, every staging row is clamped to row 0"),
    (17, 68, 64, "N % 16 == 4 and N % 8 == 4: the narrow store path of every epilogue, a partial 16-row group; K = 64 (nk <= 2 of the deep ring)"),
    (129, 132, 128, "one past the 128 tile both ways: a second block that holds one row / four columns; smallest K of the phased kernel"),
    (127, 252, 192, "one short of 128 / 256; K % 128 != 0: gemm_waves 11, 12, 13 are rerouted to the 8-wave kernel"),
    (130, 136, 64, "N % 8 == 0 with a ragged N and an M that ends inside an 8-row store group: the predicated form of the LDS-transposed stores"),
    (257, 260, 256, "one past the 256 tile both ways; smallest K of the persistent kernel, four tiles for its tile walk"),
    (1, 256, 256, "one row under a full-width tile: 255 clamped staging rows, wide stores with every row but one masked"),
    (255, 256, 320, "five k-tiles (an odd count, K % 128 != 0) with an M tail and full columns"),
    (257, 512, 512, "smallest K of split-K (K % 256 == 0, K >= 512, N % 256 == 0) with an M tail; four tiles"),
)


def gemm_operands(M, N, K, device="cpu", draw=0):
    """randn operands with w / sqrt(K) as in tests/test_ops_gpu.py, drawn on the CPU (the same values whatever `device` is).  draw: further
    independent operand sets of the same shape (tests/test_edge_bounds_cpu.py pools them where a shape has too few outputs to show a
    mutant that each element shows only with some probability); the GPU tests run draw 0."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + 7919 * draw)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    gate = torch.randn(N, generator=g)
    c0 = torch.randn(M, N, generator=g)
    ops = dict(M=M, N=N, K=K, a=a, w=w, bias=bias, gate=gate,
               c0={"f32": c0, "bf16": c0.to(torch.bfloat16), "f16": c0.to(torch.float16)})
    to = lambda x: x.to(device)
    return {k: ({f: to(t) for f, t in v.items()} if isinstance(v, dict) else to(v) if torch.is_tensor(v) else v) for k, v in ops.items()}


def gemm_lin(ops):
    """lin, t, E in float64"""
    a, w, b = ops["a"].double(), ops["w"].double(), ops["bias"].double()
    lin = a @ w.t() + b
    t = a.abs() @ w.abs().t() + b.abs()
    return lin, t, 2.0 * ops["K"] * U32 * t


def gelu64(x, tanh):
    return torch.nn.functional.gelu(x, approximate="tanh" if tanh else "none")


def gemm_ref_bound(ops, epi, gelu_pk=True, lin_t_e=None):
    """(reference, bound) of one epilogue, float64 [M][N]"""
    lin, t, E = lin_t_e if lin_t_e is not None else gemm_lin(ops)
    fmt = OUT_FMT[epi]
    if epi == 4:
        return lin, E
    if epi == 0:
        return lin, half_ulp(lin.abs() + E, fmt) + E
    if epi in (1, 2):
        ref = gelu64(lin, epi == 1)
        eg = 1.13 * E + (S_ERR_PK if gelu_pk else S_ERR_F32) * (lin.abs() + E) + 2 * U32 * ref.abs()
        return ref, half_ulp(ref.abs() + eg, fmt) + eg
    c0, gate = ops["c0"][fmt].double(), ops["gate"].double()
    ref = c0 + gate * lin
    e3 = gate.abs() * E + 3 * U32 * (c0.abs() + (gate * lin).abs())
    if epi == 3:
        return ref, e3
    return ref, half_ulp(ref.abs() + e3, fmt) + e3


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (NaN / inf in `got` count as infinitely wrong)"""
    r = (got.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


# ---- attention ---------------------------------------------------------------------------------------------------------------
# (B, H, Lq, Lk, shared, what the shape is for).  Lq covers {1, 33, 128, 129, 257, 385}, Lk {1, 5, 16, 17, 63, 64, 65, 129}, H {1, 2}.
ATTN_SHAPES = (
    (1, 1, 1, 1, 0, "one query, one key: p = 1, the output is v[0] to the bit; 127 junk query rows and 63 junk keys in the only tiles"),
    (1, 2, 33, 5, 0, "a second 32-query wave holding one query; five keys: one key in the second 4-key block of the first 16-key group"),
    (1, 1, 128, 16, 0, "a full 128-query tile against exactly one 16-key group"),
    (1, 2, 129, 17, 0, "one query past the 128 tile (a second workgroup, or the second half of a 256 tile); one key past the 16-key group"),
    (1, 1, 257, 63, 0, "one query past the 256 tile of generation 6; the key tile one short of full: a single masked key "
     "(where generations 3 and 4 read a rewritten stabiliser block: profiles/mfma_edge_parity.md)"),
    (1, 2, 385, 64, 0, "one query past the 384 tile of generation 9; exactly one unmasked key tile"),
    (1, 1, 33, 65, 0, "a second key tile that holds one valid key"),
    (1, 2, 257, 129, 0, "three key tiles, the last with one key: the stabiliser of generations 2+ is two tiles old when the mask arrives"),
    (2, 2, 129, 65, 1, "two batch entries reading ONE K / V^T (shared = 1)"),
    (1, 2, 129, 65, 0, "the same lengths with ONE batch entry: the guard rows behind O follow Lq directly (with two entries a store past "
                       "Lq of the first lands in the second's rows, which it overwrites)"),
    (2, 1, 33, 17, 0, "two batch entries with K / V^T of their own: the batch strides of Q, K, V^T and O"),
    (1, 1, 385, 1, 0, "one key under every query tile size: p = 1 in each of 385 rows"),
    (1, 2, 1, 129, 0, "one valid query in its wave (63 junk lanes beside it) against three key tiles"),
)
# (padded Q rows, padded K rows) of the fills a result must not depend on.  +-1e4 in the padded KEYS puts a junk score thousands of
# log2 units from the valid ones: a kernel that takes a maximum, a stabiliser or a range test before it masks ends in 0/0 or inf.
# The third fill keeps the 7.0 of tests/test_ops_gpu.py (a junk score about 10 log2 units off: inside the float32 range of 2^x).
JUNK_FILLS = ((1.0e4, 1.0e4), (-1.0e4, -1.0e4), (1.0e4, 7.0))


def vt_positions(n):
    """position of key j in a V^T row: inside every aligned group of 16 keys the two middle 4-key blocks are swapped"""
    j = torch.arange(n)
    return (j & ~15) | ((j & 4) << 1) | ((j & 8) >> 1) | (j & 3)


def attn_operands(B, H, Lq, Lk, shared, device="cpu"):
    """randn q, k, v rounded to bf16 (float32 tensors holding bf16 values), drawn on the CPU"""
    g = torch.Generator().manual_seed(100003 * Lq + 101 * Lk + 7 * B + H + shared)
    Bk = 1 if shared else B
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float().to(device)
    return dict(B=B, H=H, Lq=Lq, Lk=Lk, shared=shared, q=r(B, H, Lq, 64), k=r(Bk, H, Lk, 64), v=r(Bk, H, Lk, 64))


def attn_padded(ops, q_junk, k_junk):
    """the ABI's operands: Q bf16 [B][H][lq_pad][64], K bf16 [Bk][H][lk_pad][64] with junk in the padded rows (alternating sign by
    row), V^T bf16 [Bk][H][64][lk_pad] in the kernel's key order with ZERO padded keys (include/r3g.h)"""
    B, H, Lq, Lk = ops["B"], ops["H"], ops["Lq"], ops["Lk"]
    dev = ops["q"].device
    lqp, lkp = (Lq + 127) // 128 * 128, (Lk + 63) // 64 * 64
    Bk = ops["k"].shape[0]
    sq = (1.0 - 2.0 * (torch.arange(lqp, device=dev) % 2)).view(1, 1, lqp, 1)
    sk = (1.0 - 2.0 * (torch.arange(lkp, device=dev) % 2)).view(1, 1, lkp, 1)
    Q = (q_junk * sq).expand(B, H, lqp, 64).to(torch.bfloat16).contiguous()
    K = (k_junk * sk).expand(Bk, H, lkp, 64).to(torch.bfloat16).contiguous()
    Q[:, :, :Lq] = ops["q"].to(torch.bfloat16)
    K[:, :, :Lk] = ops["k"].to(torch.bfloat16)
    Vt = torch.zeros(Bk, H, 64, lkp, dtype=torch.bfloat16, device=dev)
    Vt[..., vt_positions(Lk).to(dev)] = ops["v"].to(torch.bfloat16).transpose(-1, -2)
    return Q, K, Vt, lqp, lkp


def attn_q_seen(q, prescaled):
    """the Q the MFMA sees, and the factor that takes its scores to log2 units"""
    if prescaled:
        return (q.float() * SM_SCALE32).to(torch.bfloat16).double(), 1.0
    return q.double(), SM_SCALE32


def attn_ref_bound(ops, prescaled):
    """(reference, bound), float64 [B][Lq][H * 64] (the layout of O)"""
    B, H, Lq, Lk = ops["B"], ops["H"], ops["Lq"], ops["Lk"]
    q, sc = attn_q_seen(ops["q"], prescaled)
    k = ops["k"].double().expand(B, -1, -1, -1)
    v = ops["v"].double().expand(B, -1, -1, -1)
    s2 = (q @ k.transpose(-1, -2)) * sc                       # log2 units
    p = torch.exp2(s2 - s2.max(-1, keepdim=True).values)
    p = p / p.sum(-1, keepdim=True)
    ref = p @ v
    s = p @ v.abs()
    ts = (q.abs() @ k.abs().transpose(-1, -2)).max(-1, keepdim=True).values * sc
    eps = math.log(2.0) * 2 * 65 * U32 * 2 * ts + 2.0 ** -22
    e_in = U_P * s + eps * (s + ref.abs()) + 2 * Lk * U32 * s + (Lk + Lk / 32 + 4) * U32 * (s + ref.abs())
    bound = e_in + half_ulp(ref.abs() + e_in, "bf16")
    lay = lambda x: x.permute(0, 2, 1, 3).reshape(B, Lq, H * 64)
    return lay(ref), lay(bound)


# ---- which GEMM kernel a launch ends in ------------------------------------------------------------------------------------------
GEMM_WAVES = (0, 4, 8, 9, 10, 11, 12, 13, 16, 32)
GEMM_COUNTERS = ("gemm_w4_128", "gemm_w8_128", "gemm_w16_256", "gemm_two_stage_256", "gemm_256x128", "gemm_phased",
                 "gemm_phased_persistent", "gemm_splitk2", "gemm_deep_ring")
# tile (rows, columns) and the smallest K launch_epi admits the kernel at (gemm_args_ok: K % 64 == 0 for all of them)
GEMM_KERNELS = {
    "gemm_w4_128": dict(tile=(128, 128), min_k=64), "gemm_w8_128": dict(tile=(128, 128), min_k=64),
    "gemm_w16_256": dict(tile=(256, 256), min_k=64), "gemm_two_stage_256": dict(tile=(256, 256), min_k=64),
    "gemm_256x128": dict(tile=(256, 128), min_k=64),
    "gemm_phased": dict(tile=(256, 256), min_k=128),                 # K % 128 == 0
    "gemm_phased_persistent": dict(tile=(256, 256), min_k=256),      # K % 128 == 0, K >= 256
    "gemm_splitk2": dict(tile=(256, 256), min_k=512, full_n=True),   # K % 256 == 0, K >= 512, N % 256 == 0
    "gemm_deep_ring": dict(tile=(256, 256), min_k=64),               # K % 32 == 0 in the kernel, K % 64 == 0 at the door
}
REGISTER_STAGED = ("gemm_w4_128", "gemm_w8_128", "gemm_w16_256", "gemm_two_stage_256", "gemm_256x128")   # the phased / deep-ring kernels have no such form


def gemm_switches(waves):
    """switches moved beside gemm_waves: the persistent kernel gets two CUs, so that a workgroup of the four-tile shapes walks two tiles"""
    return {"gemm_num_cu": 2} if waves == 12 else {}


def gemm_expected_kernel(waves, M, N, K, epi, num_cu=256):
    """launch_epi (csrc/gemm.hip) restated for ONE problem under the default switches: the launch counter that must move"""
    t256 = ((N + 255) // 256) * ((M + 255) // 256)
    w = waves
    if w == 0:
        assert t256 < 128, "the automatic rule takes 256 x 256 tiles from 128 tiles on: not at these shapes"
        w = 8
    if w == 13:
        if epi in (0, 3, 6, 8) and K % 256 == 0 and K >= 512 and N % 256 == 0 and 2 * t256 <= num_cu and t256 <= 128:
            return "gemm_splitk2"
        w = 11
    if w in (11, 12):
        if K % 128 == 0:
            return "gemm_phased_persistent" if (w == 12 and K >= 256) else "gemm_phased"
        w = 8
    return {32: "gemm_deep_ring", 16: "gemm_w16_256", 9: "gemm_two_stage_256", 10: "gemm_256x128", 8: "gemm_w8_128", 4: "gemm_w4_128"}[w]


def gemm_coverage(reached):
    """reached: iterable of (kernel, M, N, K).  What the closing test asserts, as a list of complaints (empty: covered): every kernel
    at a shape with an M tail, at one with an N tail (not where it needs N % 256 == 0), and at its smallest admitted K."""
    out = []
    for name, info in GEMM_KERNELS.items():
        shapes = [(M, N, K) for k_, M, N, K in reached if k_ == name]
        bm, bn = info["tile"]
        if not any(M % bm for M, N, K in shapes):
            out.append("%s: no shape with an M tail" % name)
        if not info.get("full_n") and not any(N % bn for M, N, K in shapes):
            out.append("%s: no shape with an N tail" % name)
        if not any(K == info["min_k"] for M, N, K in shapes):
            out.append("%s: never at its smallest K = %d" % (name, info["min_k"]))
    return out
