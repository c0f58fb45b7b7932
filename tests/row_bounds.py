"""Float64 references and ELEMENT-WISE error bounds for the row kernels -- LayerNorm, ln_dot, qkv_split, swiglu (csrc/elem.hip) and
GroupNorm, softmax rows, geglu (csrc/conv_kernels.hip) -- shared by tests/test_row_bounds_cpu.py (the bounds are neither vacuous nor
unreachable), tests/test_row_kernels_gpu.py and tests/test_tex_row_kernels_gpu.py (every kernel form through its r3g_op_* entry point).

Conventions of tests/edge_bounds.py: plain torch float64 on whatever device the operands live on, operands drawn on the CPU from seeds,
every bound DERIVED from the arithmetic read in the kernel and none measured, every margin factor named where it enters.  u = 2^-24.

Tools.  g(k) = k u / (1 - k u) bounds the relative error of k float32 roundings in sequence; a float32 sum of terms each of which passes
through at most k additions errs by at most g(k) sum |term|.  Every value is carried as a pair (v, e): the exact v and a bound e on
|computed - v|.  One separately rounded product (MUL) or sum (ADD) of two such pairs:
    MUL: E = |a| eb + |b| ea + ea eb,  e = E + u (|a b| + E)          ADD: E = ea + eb,  e = E + u (|a + b| + E)
A fused multiply-add rounds once where MUL then ADD round twice: its error is below theirs, so kernels whose `o * w + b` the compiler
may or may not contract are covered either way.  A 16-bit output stored by round-to-nearest: half_ulp(|v| + e) + e (edge_bounds).

Row statistics (LayerNorm, ln_dot, the 64-wide norms of qkv_split).  A row of C elements, lane l holding kl = C / 64 of them (0 extra
additions in qkv_split: one element per lane), six levels of the wave tree, one division (or an exact power-of-two product).
    mean    m^ = fl(sum) / C:  every element passes through at most kl additions in its lane (the float4 form adds x+y+z+w, then the
            group to the lane's sum: 3 + the number of later groups + 1 <= kl for C >= 256) and 6 in the tree, then the division:
            e_m = g(kl + 7) mean|x|
    x - m^  one rounding of a value within e_m of x - mean:   e_d = (u (|x| + |mean|) + e_m) (1 + u)
    var     v^ = fl(sum d^2) / C.  sum (x - m^)^2 / C = var + (mean - m^)^2 <= var + e_m^2; the rounding of each d twice (squared), the
            product (once, where it is not fused), kl additions, the tree, the division:   e_v = g(kl + 10) (var + e_m^2) + e_m^2
    rstd    a = var + eps (eps the float32 the kernel is handed), a^ = fl(v^ + eps): e_a = e_v + u (a + e_v).  r = a^-1/2 is decreasing and
            convex, so |r(a^) - r| <= r(a - e_a) - r, taken exactly (no first-order step: at a constant row a = eps and e_a is all there
            is).  rsqrtf is v_rsq_f32, specified to 1 ulp = 2 u; RSQ_ULPS = 2 is a margin factor of two on that:
            e_r = (a - e_a)^-1/2 - r + RSQ_ULPS 2 u (a - e_a)^-1/2
    RMS     the same without the mean: d = x exactly.
LayerNorm then is MUL(d, r) [MUL w] [ADD b] [MUL (1 + scale), where 1 + scale is itself one rounding: (1 + s, u |1 + s|)] [ADD shift],
each step present when its operand is; rows in [seg2_row0, seg2_row1) take scale2 / shift2, every other row the vectors of its batch.
The order is the kernel's: affine BEFORE modulation.  bf16 output: half_ulp(|ref| + e) + e.
  e4m3 output.  The finished float32 values o^ (within e of ref) are scaled by the row: qs = fl(amax^ fl(1 / 448)) -- two roundings --
  with |amax^ - amax| <= max e, so |qs - amax / 448| <= (max e + g(2) (amax + max e)) / 448, and an all-zero row (amax = 0, e = 0) has
  qs = 1 to the bit; a row with amax <= max e (the constant row: ref = 0, o^ = rounding residue or zero) may have either.  The code of o^ is the e4m3 nearest to fl(o^ fl(1 / qs)), saturating at 448: with t = ref / qs (qs the STORED
  scale), e_t = e / qs + g(2) (|t| + e / qs), the decoded code is within half_ulp_e4m3(min(|t| + e_t, 448)) + e_t of t
  (half_ulp_e4m3(v) = 2^(floor(log2 v) - 4), at least 2^-10: three mantissa bits, subnormal step 2^-9).
ln_dot.  out = sum_c o_c w_c + b with o = LayerNorm without modulation (x itself when do_ln == 0: e = 0), no 16-bit rounding.  A term passes
through at most 4 roundings inside its group of four (product, three fused steps), kl additions of groups, the tree, and + b:
    e = sum |w_c| e_c + g(kl + 11) (sum |o_c w_c| + sum |w_c| e_c + |b|)            (absolute values, as edge_bounds does for t)

qkv_split.  Per (token, head): 64 columns of q and of k, one per lane.  RMSNorm: q r qw with r = (mean q^2 + eps)^-1/2; LayerNorm:
(q - mean) r qw + qb; both as "row statistics" with kl = 0; then q (not k) times q_scale when q_scale != 0 (one more MUL), then bf16.
norm 0 with q_scale 0 copies bits.  V^T[d][vt_key_pos(dst_row0 + t)] = v[t][d] bit for bit, the columns of the last 64-token block
past l are zeros, bit for bit.

GroupNorm.  z = x + addv[sample] is ONE float32 rounding in both passes (exact without addv).  Pass 1 keeps, per (row lane p, channel),
float32 sums of z and of z^2 over m = ceil(rpb / P) rows at most (rpb rows per block, P row lanes), and folds them in float64 (2^-53: not
carried).  With Ez = mean |z|, Ez2 = mean z^2 over the group:
    mean    e_m = g(m + 1) Ez                          (the rounding of z, m additions), + u |mean| where it is stored as float32
    var     pass 2 forms E[z^2] - mean^2:  e_v = g(m + 3) Ez2 + 2 |mean| e_m + e_m^2
            THE ERROR IS RELATIVE TO E[z^2], NOT TO THE VARIANCE: for a group whose mean is k standard deviations from zero it is
            (1 + k^2) times what a two-pass variance would have.  That cancellation is inherent to the kernel's stated arithmetic
            (single pass, float32 partial sums); the term is carried here, and the GPU shapes keep |mean| <= 2 std so that it stays small.
    rstd    float64 1 / sqrt(var + eps), rounded to float32:  e_r = (a - e_v)^-1/2 - r + u (a - e_v)^-1/2
    apply   ADD(z, -mean) MUL r MUL gamma ADD beta, then SiLU where asked, then bf16.
SiLU / GELU forms, READ from the device functions as S_ERR_F32 was (edge_bounds):
    silu(x) = x / (1 + __expf(-x)), __expf = v_exp_f32(x log2 e).  With S = 1 / (1 + E), E = e^-x: dS = S (1 - S) dE / E, and dE / E <=
    2 u |x| (the product with log2 e and the constant) + 2^-22 (v_exp_f32 and its argument conversion, as in the attention bound);
    1 + E and the division add 3 u S.  |x| dS <= |x| (0.25 2^-22 + 3 u) + 2 u x^2 S (1 - S) <= 4 u |x| + 0.9 u  (x^2 S (1 - S) <= 0.44)
    <= 1e-6 |x| wherever 0.9 u <= 7.6e-7 |x|, and below that |x| the x^2 term is 0.5 u x^2 < 1e-6 |x| as well: SILU_ERR = 1e-6 |x|.
    |silu'| <= 1.1 carries the error of the argument.
    gelu_erf(x) = x Phi(x), Phi by Abramowitz & Stegun 7.1.26 with halved coefficients (|error| <= 0.75e-7), a v_rcp_f32 and a
    v_exp_f32 (1 ulp each, on values <= 1) and about ten float32 operations: S_ERR_F32 = 1e-6 |x| of edge_bounds, the same function.
geglu: out = bf16(a gelu_erf(g)): e = |a| S_ERR |g| + u |ref|.   swiglu: out = bf16(silu(a) g): e = |g| S_ERR |a| + u |ref|.  (One product
rounding each; the operands are bf16 and exact.)

Softmax rows.  sl = fl(scale * fl(log2 e)) in float32, the kernel's own constant; the reference is softmax of v sl in base 2.  The kernel
subtracts mx^ = fl(max v * sl) (scale > 0: the maximum of the raw scores is the maximum of the scaled ones) inside one fma: a_i = v_i sl -
mx^ rounded once.  A common factor 2^(mx - mx^) cancels in p = 2^a / sum.  Per exponential, relative: eps_i = ln 2 u |a_i| (that rounding)
+ 2^-22 (v_exp_f32 and its argument conversion, as in the attention bound).  The sum: a thread adds four exponentials per 1024-column
sweep, then the wave tree (6) and the four waves (3): ks = 4 ceil(n / 1024) + 9; its relative error is the p-weighted mean of eps_i plus
g(ks).  The reciprocal and the product: 2 u.  v_exp_f32 returns zero below the smallest normal 2^-126 (the raw instruction has no
denormal results); the sum is at least 1 - its error, so that is an absolute 2^-126 on p:
    e_i = p_i (eps_i + sum_j p_j eps_j + g(ks + 2)) + 2^-126          bound: half_ulp_bf16(p_i + e_i) + e_i
An element whose exact p is below 2^-135 (it rounds to zero in bf16 with room to spare) must be stored as zero, bit for bit.

The launch rules are restated at the end (ln_form, ln_dot_form, gn_geometry), as edge_bounds.gemm_expected_kernel restates launch_epi.
"""
import math

import torch

from edge_bounds import S_ERR_F32, U32, half_ulp, vt_positions, worst_ratio  # noqa: F401  (re-exported for the tests)

RSQ_ULPS = 2.0
SILU_ERR = 1e-6
SILU_SLOPE = 1.1
LOG2E32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
FLUSH = 2.0 ** -126


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def g(k):
    return k * U32 / (1.0 - k * U32)


def MUL(a, ea, b, eb):
    E = a.abs() * eb + b.abs() * ea + ea * eb
    return a * b, E + U32 * ((a * b).abs() + E)


def ADD(a, ea, b, eb):
    E = ea + eb
    return a + b, E + U32 * ((a + b).abs() + E)


def bf16_bound(ref, e):
    return half_ulp(ref.abs() + e, "bf16") + e


def row_stats(x, eps, kl, center=True, rsq_rel=RSQ_ULPS * 2 * U32):
    """(d, e_d, r, e_r) of the module docstring for the rows x [..., C] (float64); eps: the float32 value as a python float"""
    A = x.abs().mean(-1, keepdim=True)
    if center:
        mu = x.mean(-1, keepdim=True)
        e_m = g(kl + 7) * A
        d = x - mu
        e_d = (U32 * (x.abs() + mu.abs()) + e_m) * (1 + U32)
    else:
        e_m = torch.zeros_like(A)
        d, e_d = x, torch.zeros_like(x)
    var = (d * d).mean(-1, keepdim=True)
    e_v = g(kl + 10) * (var + e_m ** 2) + e_m ** 2
    a = var + eps
    e_a = e_v + U32 * (a + e_v)
    r = a ** -0.5
    r_hi = (a - e_a).clamp_min(0.25 * a) ** -0.5
    e_r = r_hi - r + rsq_rel * r_hi
    return d, e_d, r, e_r


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
LN_EPS = f32(1e-6)
LN_C = (64, 192, 256, 768, 1024, 1536, 2048)
LN_COMBOS = ("none", "affine", "mod", "affine_mod", "scale_only")
# (name, rows, rows_per_batch, (seg2_row0, seg2_row1))
LN_ROWCFGS = (("rows1", 1, 1, None), ("rows5", 5, 5, None), ("rows17", 17, 17, None),
              ("batches6x3", 18, 3, None),        # batch changes inside a 4-row wave, mod_stride != 0, batch strides > rows_per_batch * ld
              ("seg2", 13, 13, (6, 11)))          # start and end both inside a 4-row wave
LN_PAD = 8          # ldx = ldy = C + 8; batch strides rows_per_batch * ld + 8
XDTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


def ln_formats(C):
    return (0, 1, 2) if C % 256 == 0 else (0,)


def ln_rows_draw(gen, rows, C, zero_row=None):
    """rows with |mean| <= 2 std; from five rows on, row 1 has variance 1e-6 (eps matters) and row 3 is constant; zero_row: all zeros"""
    std = torch.exp(torch.rand(rows, 1, generator=gen) * 1.4 - 0.7)
    mean = (torch.rand(rows, 1, generator=gen) * 4 - 2) * std
    x = torch.randn(rows, C, generator=gen)
    x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)
    if rows >= 5:
        std[1], mean[1] = 1e-3, 1.5e-3
    x = x * std + mean
    if rows >= 5:
        x[3] = 0.8125
    if zero_row is not None:
        x[zero_row] = 0.0
    return x


def ln_case(C, x_format, rowcfg, combo, device="cpu", draw=0, zero_row=None):
    """operands of one LayerNorm launch.  x: [rows][C] float32 holding values of the row format.  The per-row vectors the kernel must
    pick (sc_rows / sh_rows [rows][C], has_sc / has_sh [rows]) are spelled out here from (batch, seg2), independently of the kernel."""
    name, rows, rpb, seg2 = rowcfg
    gen = torch.Generator().manual_seed(7919 * C + 131 * x_format + 17 * rows + LN_COMBOS.index(combo) + 1000003 * draw + (rpb != rows))
    x = ln_rows_draw(gen, rows, C, zero_row).to(XDTYPE[x_format]).float()
    nbatch = (rows + rpb - 1) // rpb
    aff = combo in ("affine", "affine_mod")
    has_scale = combo in ("mod", "affine_mod", "scale_only")
    has_shift = combo in ("mod", "affine_mod")
    w = 1 + 0.1 * torch.randn(C, generator=gen) if aff else None
    b = 0.1 * torch.randn(C, generator=gen) if aff else None
    scale = 0.3 * torch.randn(nbatch, C, generator=gen) if has_scale else None
    shift = 0.3 * torch.randn(nbatch, C, generator=gen) if has_shift else None
    scale2 = 0.3 * torch.randn(C, generator=gen) if seg2 else None
    shift2 = 0.3 * torch.randn(C, generator=gen) if seg2 else None
    batch = torch.arange(rows) // rpb
    in2 = torch.zeros(rows, dtype=torch.bool)
    if seg2:
        in2[seg2[0]:seg2[1]] = True
    zero = torch.zeros(rows, C)
    sc_rows = torch.where(in2[:, None], scale2[None] if seg2 else zero, scale[batch] if has_scale else zero)
    sh_rows = torch.where(in2[:, None], shift2[None] if seg2 else zero, shift[batch] if has_shift else zero)
    has_sc = in2 | has_scale
    has_sh = in2 | has_shift
    t = lambda v: v.to(device) if torch.is_tensor(v) else v
    return {k: t(v) for k, v in dict(C=C, x_format=x_format, rows=rows, rpb=rpb, seg2=seg2, combo=combo, x=x, w=w, b=b, scale=scale, shift=shift,
                                     scale2=scale2, shift2=shift2, sc_rows=sc_rows, sh_rows=sh_rows, has_sc=has_sc, has_sh=has_sh,
                                     nbatch=nbatch, eps=LN_EPS).items()}


def ln_ref_err(case):
    """(ref, e) float64 [rows][C]: the exact LayerNorm and the bound on the kernel's float32 value BEFORE the output rounding"""
    C = case["C"]
    x = case["x"].double()
    d, e_d, r, e_r = row_stats(x, case["eps"], C // 64)
    v, e = MUL(d, e_d, r, e_r)
    zero = torch.zeros_like(v)
    if case["w"] is not None:
        v, e = MUL(v, e, case["w"].double().expand_as(v), zero)
    if case["b"] is not None:
        v, e = ADD(v, e, case["b"].double().expand_as(v), zero)
    one_s = 1.0 + case["sc_rows"].double()
    v2, e2 = MUL(v, e, one_s, U32 * one_s.abs())
    m = case["has_sc"][:, None]
    v, e = torch.where(m, v2, v), torch.where(m, e2, e)
    v2, e2 = ADD(v, e, case["sh_rows"].double(), zero)
    m = case["has_sh"][:, None]
    return torch.where(m, v2, v), torch.where(m, e2, e)


def ln_ref_bound(case):
    ref, e = ln_ref_err(case)
    return ref, bf16_bound(ref, e)


# e4m3 (OCP, "fn": no infinities, 448 the largest): value of every code
def _e4m3_table():
    vals = []
    for code in range(256):
        s, ex, m = code >> 7, (code >> 3) & 15, code & 7
        v = (m / 8.0) * 2.0 ** -6 if ex == 0 else (1 + m / 8.0) * 2.0 ** (ex - 7)
        if ex == 15 and m == 7:
            v = float("nan")
        vals.append(-v if s else v)
    return torch.tensor(vals, dtype=torch.float64)


E4M3 = _e4m3_table()


def e4m3_decode(codes):
    return E4M3.to(codes.device)[codes.long()]


def e4m3_half_ulp(v):
    _, ex = torch.frexp(v.abs().double())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), ex - 1 - 4).clamp_min(2.0 ** -10)


def ln_fp8_check(case, codes, scales, ref_err=None):
    """(worst |scale - amax / 448| / bound over the rows with amax > 0, worst code error / bound, all-zero rows have scale 1 and codes 0)"""
    ref, e = ref_err if ref_err is not None else ln_ref_err(case)
    amax, emax = ref.abs().amax(-1), e.amax(-1)
    zero = (amax == 0) & (emax == 0)
    sb = (emax + g(2) * (amax + emax)) / 448.0
    qs = scales.double()
    alt = (amax <= emax) & (qs == 1.0)          # amax^ may be exactly zero there: the kernel's scale of an all-zero row
    keep = ~zero & ~alt
    rs = worst_ratio(qs[keep], amax[keep] / 448.0, sb[keep])
    zeros_ok = bool((qs[zero] == 1.0).all()) and bool(((codes[zero] & 127) == 0).all())
    t = ref / qs[:, None]
    e_t = e / qs[:, None] + g(2) * (t.abs() + e / qs[:, None])
    bound = e4m3_half_ulp((t.abs() + e_t).clamp_max(448.0)) + e_t
    return rs, worst_ratio(e4m3_decode(codes), t, bound), zeros_ok


# ---- ln_dot ---------------------------------------------------------------------------------------------------------------------------
LND_C = (64, 192, 256, 1024, 2048)
LND_ROWS = (1, 5, 17)
LND_PAD = 4
LND_BIAS = f32(0.37)


def lnd_case(C, x_bf16, rows, do_ln, affine, device="cpu", draw=0):
    gen = torch.Generator().manual_seed(104729 * C + 977 * rows + 4 * x_bf16 + 2 * do_ln + affine + 1000003 * draw)
    x = ln_rows_draw(gen, rows, C).to(XDTYPE[x_bf16]).float()
    lnw = 1 + 0.1 * torch.randn(C, generator=gen) if affine else None
    lnb = 0.1 * torch.randn(C, generator=gen) if affine else None
    w = torch.randn(C, generator=gen) / C ** 0.5
    t = lambda v: v.to(device) if torch.is_tensor(v) else v
    return {k: t(v) for k, v in dict(C=C, x_bf16=x_bf16, rows=rows, do_ln=do_ln, affine=affine, x=x, lnw=lnw, lnb=lnb, w=w, b=LND_BIAS,
                                     eps=LN_EPS).items()}


def lnd_ref_bound(case):
    """(reference, bound) float64 [rows]"""
    C = case["C"]
    x = case["x"].double()
    if case["do_ln"]:
        d, e_d, r, e_r = row_stats(x, case["eps"], C // 64)
        v, e = MUL(d, e_d, r, e_r)
        if case["affine"]:
            v, e = MUL(v, e, case["lnw"].double().expand_as(v), torch.zeros_like(v))
            v, e = ADD(v, e, case["lnb"].double().expand_as(v), torch.zeros_like(v))
    else:
        v, e = x, torch.zeros_like(x)
    w = case["w"].double()
    ref = (v * w).sum(-1) + case["b"]
    carried = (w.abs() * e).sum(-1)
    return ref, carried + g(C // 64 + 11) * ((v * w).abs().sum(-1) + carried + abs(case["b"]))


# ---- qkv_split ------------------------------------------------------------------------------------------------------------------------
QKV_EPS = f32(1e-6)
QKV_L = (1, 63, 65, 130)
QKV_BH = ((1, 1), (2, 3))
QKV_LAYOUTS = ("khd", "head_qkv", "head_kv", "q_only")
QKV_QSCALE = (0.0, f32(0.125 * LOG2E32))


def qkv_layout(layout, H):
    """(q_off, k_off, v_off, head_stride, columns) of the four QkvLayouts"""
    return {"khd": (0, 64 * H, 128 * H, 64, 192 * H), "head_qkv": (0, 64, 128, 192, 192 * H),
            "head_kv": (-1, 0, 64, 128, 128 * H), "q_only": (0, -1, -1, 64, 64 * H)}[layout]


def qkv_case(L, B, H, layout, norm, weights, q_scale, device="cpu", draw=0):
    gen = torch.Generator().manual_seed(15485863 * L + 31 * B + H + 7 * QKV_LAYOUTS.index(layout) + 101 * norm + 3 * weights + 1000003 * draw)
    q_off, k_off, v_off, hs, cols = qkv_layout(layout, H)
    ld = cols + 8
    src = (torch.randn(B, L, ld, generator=gen) * 1.5 + 0.5).to(torch.bfloat16)
    vec = lambda: 1 + 0.2 * torch.randn(64, generator=gen)
    qw, kw = (vec(), vec()) if (weights and norm) else (None, None)
    qb, kb = (vec() - 1, vec() - 1) if (weights and norm == 2) else (None, None)
    t = lambda v: v.to(device) if torch.is_tensor(v) else v
    return {k: t(v) for k, v in dict(L=L, B=B, H=H, layout=layout, norm=norm, q_scale=q_scale, q_off=q_off, k_off=k_off, v_off=v_off, hs=hs,
                                     ld=ld, src=src, qw=qw, qb=qb, kw=kw, kb=kb, eps=QKV_EPS).items()}


def qkv_heads(case, off):
    """[B][H][L][64] float64 view of one operand's columns"""
    B, H, L = case["B"], case["H"], case["L"]
    cols = (off + case["hs"] * torch.arange(H, device=case["src"].device))[:, None] + torch.arange(64, device=case["src"].device)[None]
    return case["src"].double()[:, :, cols].permute(0, 2, 1, 3)


def qkv_norm_ref_bound(case, which):
    """(reference, bound) float64 [B][H][L][64] of Q ("q") or K ("k")"""
    x = qkv_heads(case, case["q_off"] if which == "q" else case["k_off"])
    wt, bs = (case["qw"], case["qb"]) if which == "q" else (case["kw"], case["kb"])
    zero = torch.zeros_like(x)
    v, e = x, zero
    if case["norm"]:
        d, e_d, r, e_r = row_stats(x, case["eps"], 0, center=case["norm"] == 2)
        v, e = MUL(d, e_d, r, e_r)
        v, e = MUL(v, e, (wt.double() if wt is not None else torch.ones(64, dtype=torch.float64, device=x.device)).expand_as(v), zero)
        if case["norm"] == 2:
            v, e = ADD(v, e, (bs.double() if bs is not None else torch.zeros(64, dtype=torch.float64, device=x.device)).expand_as(v), zero)
    if which == "q" and case["q_scale"] != 0.0:
        v, e = MUL(v, e, torch.full_like(v, case["q_scale"]), zero)
    return v, bf16_bound(v, e)


def qkv_vt_expected(case, dst_row0):
    """{V^T column: bf16 [B][H][64] column values} as a dense tensor [B][H][64][n] over the columns the call owns: n = the 64-token
    blocks of l, starting at dst_row0; returns (first column, tensor) with the kernel's key order applied inside"""
    B, H, L = case["B"], case["H"], case["L"]
    n = (L + 63) // 64 * 64
    dev = case["src"].device
    cols = (case["v_off"] + case["hs"] * torch.arange(H, device=dev))[:, None] + torch.arange(64, device=dev)[None]
    v = case["src"][:, :, cols].permute(0, 2, 3, 1)            # [B][H][64][L]
    out = torch.zeros(B, H, 64, n, dtype=torch.bfloat16, device=dev)
    out[..., vt_positions(L).to(dev)] = v
    return dst_row0, out


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------------
GN_EPS = f32(1e-5)
GN_SHAPES = ((1, 32, 32, "one row, one channel per group, 32 row lanes of which one has a row"),
             (17, 64, 32, "two blocks (rpb 9), 16 row lanes"),
             (67, 320, 32, "three row lanes; 10 channels per group: groups straddle float4 columns"),
             (3, 12, 3, "85 row lanes, the last thread idle; 4 channels per group"),
             (33, 1280, 32, "two columns per thread (320 float4 columns), one row lane"),
             (16, 2560, 32, "three columns per thread (640 float4 columns)"),
             (4100, 32, 8, "the 256-block cap: rpb 17, the last 14 blocks empty"))


def gn_geometry(rows, C):
    """group_norm_blocks and the thread geometry of gn_partial_kernel / gn_apply_kernel, restated"""
    nblk = min(256, max(1, (rows + 15) // 16))
    rpb = (rows + nblk - 1) // nblk
    cq = C // 4
    P = 1 if cq >= 256 else 256 // cq
    return dict(nblk=nblk, rpb=rpb, P=P, cols_per_thread=(cq + 255) // 256, m=(rpb + P - 1) // P, capped=(rows + 15) // 16 > 256,
                empty_blocks=nblk - (rows + rpb - 1) // rpb)


def gn_case(rows, C, groups, nb, addv, device="cpu", draw=0):
    """x with group means within 2 std of zero"""
    gen = torch.Generator().manual_seed(32452843 * rows + 257 * C + 5 * groups + 2 * nb + addv + 1000003 * draw)
    cpg = C // groups
    std = torch.exp(torch.rand(nb, 1, groups, 1, generator=gen) * 1.4 - 0.7)
    mean = (torch.rand(nb, 1, groups, 1, generator=gen) * 3 - 1.5) * std
    x = (torch.randn(nb, rows, groups, cpg, generator=gen) * std + mean).reshape(nb, rows, C)
    add_stride = C + 4
    av = None
    if addv:
        av = torch.zeros(nb, add_stride)
        av[:, :C] = (0.25 * torch.randn(nb, groups, 1, generator=gen) * std[:, 0]).expand(nb, groups, cpg).reshape(nb, C) + \
            0.1 * torch.randn(nb, C, generator=gen)
    gamma = 1 + 0.2 * torch.randn(C, generator=gen)
    beta = 0.2 * torch.randn(C, generator=gen)
    t = lambda v: v.to(device) if torch.is_tensor(v) else v
    return {k: t(v) for k, v in dict(rows=rows, C=C, groups=groups, nb=nb, x=x, addv=av, add_stride=add_stride, gamma=gamma, beta=beta,
                                     eps=GN_EPS).items()}


def gn_ref_bound(case, silu):
    """(reference, bound) float64 [nb][rows][C]"""
    rows, C, G, nb = case["rows"], case["C"], case["groups"], case["nb"]
    geo = gn_geometry(rows, C)
    m = geo["m"]
    z = case["x"].double()
    e_z = torch.zeros_like(z)
    if case["addv"] is not None:
        z = z + case["addv"].double()[:, None, :C]
        e_z = U32 * z.abs()
    zg = z.view(nb, rows, G, C // G)
    Ez = zg.abs().mean((1, 3), keepdim=True)
    Ez2 = (zg * zg).mean((1, 3), keepdim=True)
    mu = zg.mean((1, 3), keepdim=True)
    var = ((zg - mu) ** 2).mean((1, 3), keepdim=True)
    e_m = g(m + 1) * Ez
    e_v = g(m + 3) * Ez2 + 2 * mu.abs() * e_m + e_m ** 2
    a = var + case["eps"]
    r = a ** -0.5
    r_hi = (a - e_v).clamp_min(0.25 * a) ** -0.5
    e_r = r_hi - r + U32 * r_hi
    full = lambda s: s.expand(nb, rows, G, C // G).reshape(nb, rows, C)
    zero = torch.zeros_like(z)
    v, e = ADD(z, e_z, -full(mu), full(e_m + U32 * mu.abs()))
    v, e = MUL(v, e, full(r), full(e_r))
    v, e = MUL(v, e, case["gamma"].double().expand_as(v), zero)
    v, e = ADD(v, e, case["beta"].double().expand_as(v), zero)
    if silu:
        ref = v * torch.sigmoid(v)
        e = SILU_SLOPE * e + SILU_ERR * (v.abs() + e)
        v = ref
    return v, bf16_bound(v, e)


# ---- softmax rows -----------------------------------------------------------------------------------------------------------------------
SM_N = (4, 1020, 1024, 1028, 4100)
SM_ROWS = (1, 3)
SM_SCALE = f32(512 ** -0.5)
SM_PAD = 4


def sm_case(rows, n, device="cpu", draw=0):
    """row 0: scaled scores scale * s of standard deviation 3; with three rows, row 1 holds equal scores and row 2 spreads scale * s over 300
    units ([-120, 180]): most of its probabilities are far below the smallest bf16 and must be stored as zeros"""
    gen = torch.Generator().manual_seed(49979687 * rows + n + 1000003 * draw)
    s = torch.randn(rows, n, generator=gen) * (3.0 / SM_SCALE)
    if rows >= 3:
        s[1] = 41.5
        s[2] = (torch.rand(n, generator=gen) * 300.0 - 120.0) / SM_SCALE
    return dict(rows=rows, n=n, s=s.to(device), scale=SM_SCALE)


def sm_ref_bound(case):
    """(reference, bound, must_be_zero) float64 / bool [rows][n]"""
    n = case["n"]
    sl = f32(case["scale"] * LOG2E32)
    a = case["s"].double() * sl
    a = a - a.max(-1, keepdim=True).values
    p = torch.exp2(a)
    p = p / p.sum(-1, keepdim=True)
    eps = math.log(2.0) * U32 * a.abs() + 2.0 ** -22
    ks = 4 * ((n + 1023) // 1024) + 9
    e = p * (eps + (p * eps).sum(-1, keepdim=True) + g(ks + 2)) + FLUSH
    return p, bf16_bound(p, e), p < 2.0 ** -135


# ---- GEGLU / SwiGLU ---------------------------------------------------------------------------------------------------------------------
GLU_F = (8, 72, 1288)
GLU_ROWS = (1, 3)
GLU_PAD = 8


def glu_case(rows, F, device="cpu", draw=0):
    """bf16 [rows][2 F] with values drawn uniformly from +-6"""
    gen = torch.Generator().manual_seed(86028121 * rows + F + 1000003 * draw)
    x = ((torch.rand(rows, 2 * F, generator=gen) * 12.0 - 6.0)).to(torch.bfloat16)
    return dict(rows=rows, F=F, x=x.to(device))


def glu_ref_bound(case, kind):
    F = case["F"]
    a, b = case["x"][:, :F].double(), case["x"][:, F:].double()
    if kind == "geglu":
        ref = a * torch.nn.functional.gelu(b)
        e = a.abs() * S_ERR_F32 * b.abs() + U32 * ref.abs()
    else:
        ref = a * torch.sigmoid(a) * b
        e = b.abs() * SILU_ERR * a.abs() + U32 * ref.abs()
    return ref, bf16_bound(ref, e)


# ---- which kernel form a launch takes (layernorm_launch / ln_dot_launch of csrc/elem.hip, restated) -----------------------------------------
LN_COUNTERS = ("ln_rows1", "ln_rows4", "ln_fixed_count", "ln_mode_inst")


def ln_form(C, x_format, ldx, ldy, has, rows, ln_rows=0, ln_fixed=1, ln_modes=1, rows4_min=65536, fp8=False, seg2=False):
    """has: the set of operands given, of {"w", "b", "scale", "shift", "scale2", "shift2"}.  -> dict(kernel "small" | "vec", rpw, nv (0:
    run-time count), mode, counters: the increments of LN_COUNTERS)"""
    none = {c: 0 for c in LN_COUNTERS}
    if not (x_format != 0 or (C % 256 == 0 and ldx % 4 == 0 and ldy % 4 == 0)):
        return dict(kernel="small", rpw=1, nv=0, mode=-1, counters=none)       # the scalar kernel bumps no counter
    rpw = ln_rows if ln_rows in (1, 4) else (4 if rows >= rows4_min else 1)
    fixed = bool(ln_fixed) and C in (1024, 1536)
    m_aff = bool(ln_modes) and {"w", "b"} <= has and not (has & {"scale", "shift", "scale2", "shift2"}) and not fp8
    m_mod = bool(ln_modes) and not (has & {"w", "b"}) and {"scale", "shift"} <= has and not fp8 and (not seg2 or {"scale2", "shift2"} <= has)
    mode = (2 if m_mod else 1 if m_aff else -1) if (fixed and C == 1024) else -1
    cnt = dict(none)
    cnt["ln_rows4" if rpw == 4 else "ln_rows1"] = 1
    cnt["ln_fixed_count"] = int(fixed)
    cnt["ln_mode_inst"] = int(mode != -1)
    return dict(kernel="vec", rpw=rpw, nv=(C // 256 if fixed else 0), mode=mode, counters=cnt)


def ln_dot_form(C, x_bf16, ldx, rows, ln_rows=0, ln_fixed=1, rows4_min=65536):
    none = {c: 0 for c in LN_COUNTERS}
    if not (x_bf16 or (C % 256 == 0 and C <= 2048 and ldx % 4 == 0)):
        return dict(kernel="small", rpw=1, nv=0, counters=none)
    rpw = ln_rows if ln_rows in (1, 4) else (4 if rows >= rows4_min else 1)
    fixed = bool(ln_fixed) and C == 1024
    cnt = dict(none)
    cnt["ln_rows4" if rpw == 4 else "ln_rows1"] = 1
    cnt["ln_fixed_count"] = int(fixed)
    return dict(kernel="vec", rpw=rpw, nv=(4 if fixed else 0), counters=cnt)


def ln_switch_sets(C, x_format, ldx, ldy):
    """the (ln_rows, ln_fixed, ln_modes) settings that select different code at this width: the scalar kernel has none, ln_fixed acts at
    1024 / 1536, ln_modes at a fixed 1024"""
    if not (x_format != 0 or (C % 256 == 0 and ldx % 4 == 0 and ldy % 4 == 0)):
        return ((1, 1, 1),)
    out = []
    for rpw in (1, 4):
        for fixed in ((0, 1) if C in (1024, 1536) else (1,)):
            for modes in ((0, 1) if (C == 1024 and fixed) else (1,)):
                out.append((rpw, fixed, modes))
    return tuple(out)


def ln_plan():
    """every (C, x_format, (ln_rows, ln_fixed, ln_modes), row configuration, operand combination) tests/test_row_kernels_gpu.py launches"""
    for C in LN_C:
        for xf in ln_formats(C):
            for sw in ln_switch_sets(C, xf, C + LN_PAD, C + LN_PAD):
                for rc in LN_ROWCFGS:
                    for combo in LN_COMBOS:
                        yield C, xf, sw, rc, combo


def ln_forms_required():
    """what the closing test of tests/test_row_kernels_gpu.py asserts was reached: (kernel, nv, mode, rpw, x_format)"""
    out = {("small", 0, -1, 1, 0)}
    for rpw in (1, 4):
        for xf in (0, 1, 2):
            out |= {("vec", 0, -1, rpw, xf), ("vec", 6, -1, rpw, xf)} | {("vec", 4, mode, rpw, xf) for mode in (1, 2, -1)}
    return out


def combo_has(combo, seg2):
    has = {"none": set(), "affine": {"w", "b"}, "mod": {"scale", "shift"}, "affine_mod": {"w", "b", "scale", "shift"}, "scale_only": {"scale"}}[combo]
    return has | ({"scale2", "shift2"} if seg2 else set())
