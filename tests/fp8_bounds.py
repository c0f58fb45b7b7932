"""Float64 references, ELEMENT-WISE bounds and the bit-exact quantiser restatement for the FP8 path -- quant_fp8_rows_kernel (csrc/elem.hip),
gemm8f_kernel and the e4m3-output epilogue (csrc/gemm.hip) -- shared by tests/test_fp8_bounds_cpu.py (the bounds are neither vacuous
nor unreachable) and tests/test_fp8_edges_gpu.py (r3g_op_quant_fp8, r3g_op_gemm_fp8, r3g_op_gemm_fp8_e4m3 at ragged shapes).

Conventions of tests/edge_bounds.py: plain torch on whatever device the operands live on, operands drawn on the CPU from a seed that is
a function of the shape, every bound DERIVED from the arithmetic read in the kernel and none measured.  u = 2^-24.

The quantiser, restated to the bit (quant_ref; float32 on the CPU, where torch neither flushes subnormals nor fuses):
    amax = max |x| over the row (a NaN element does not enter: fmaxf drops it)
    sc   = amax > 0 ? max(fl(amax * fl(1 / 448)), 2^-126) : 1          the floor keeps 1 / sc <= 2^126 finite (include/r3g.h)
    inv  = fl(1 / sc)                                                  HIP's float division is correctly rounded by default
    code = RNE_saturating_e4m3(fl(x * inv))                            ties to even, sign kept, NaN -> 0x7F; |x * inv| <= 448 (1 + 3 u) rounds to 448
e4m3_encode is that conversion from the table of row_bounds.E4M3 (the nearer of the two neighbouring codes; on a tie the even code).  If
the GPU's 1 / sc were not correctly rounded, a code could differ by one step on an exact tie only; no such allowance is made here --
the division is IEEE in the build the project ships (no fast-math flag in 3d-re-gen_amd/build.py), the GPU test compares bits, and on
an MI355X every code and every scale of the cases below came out equal (profiles/fp8_edge_parity.md).
fl(448 * fl(1 / 448)) is exactly 1 in float32, so a row whose amax is 448 * 2^e has the scale 2^e to the bit: the "sat" rows below hold
+-448 * scale exactly and every other e4m3 value at that scale (the codes come back unchanged), and the "ties" rows every midpoint
between two neighbouring e4m3 values, on which the conversion must take the even code.

GEMM.  Operands as the kernel sees them: e4m3 codes a8 [M][K], w8 [N][K], fp32 row scales sa [M], sw [N], fp32 bias and gate, the old C.
With A, W the decoded codes in float64 and s = sa[m] sw[n]:
    lin = s (A W^T) + bias            t = s (|A| |W|^T) + |bias|            E = (2 K + 2) u t
  * 2 K u t is edge_bounds' E with K counting fp8 products: a product of two e4m3 values has at most 8 significant bits and is exact in
    float32; a float32 sum of K of them and the bias, in any order, errs by at most K u t to first order, and the single factor 2 covers
    whatever v_mfma_scale_f32_16x16x128_f8f6f4 does inside one 128-deep instruction (the same one margin as for the bf16 MFMA).
  * + 2 u t: gemm8f_kernel forms fl(sw * sa) and multiplies the accumulator by it (`acc[j][i] *= swv[j] * sav[i]`): two more roundings
    of a value bounded by s |A| |W|^T <= t.  (The sum with the bias is inside K u t, as in edge_bounds.)
The epilogues are the shared ones of gemm_epilogue, so (lin, t, E) goes into edge_bounds.gemm_ref_bound for 0, 1, 2, 3, 6 unchanged.  The
fp8 launcher does not carry "gelu_pk" (gemm_fp8_launch leaves GemmArgs.gelu_pk zero): epilogues 1 and 2 take the fp32 forms whatever the
option says, so the GPU test holds both settings against S_ERR_F32.
    epilogue 7 (r3g_op_gemm_fp8_e4m3): v = gelu_erf4<false>(acc + bias) * inv with inv = fl(1 / out_scale), then v_cvt_pk_fp8_f32.
        ref = gelu_erf(lin) in float64,  eg = 1.13 E + S_ERR_F32 (|lin| + E) + 2 u |ref|            (edge_bounds: the fp32 erf form)
        tt  = ref / out_scale,           e_t = eg / out_scale + g(2) (|tt| + eg / out_scale)        (inv's rounding, the product's)
        |decode(code) - clamp(tt, +-448)| <= half_ulp_e4m3(min(|tt| + e_t, 448)) + e_t              (row_bounds.ln_fp8_check's code-space form;
        the conversion saturates, clamping is 1-Lipschitz).  OUT_SCALE = fl(0.011) puts lin > 4.93 past 448: a few elements of the larger
        random shapes saturate.  FINDING (first GPU run of tests/test_fp8_edges_gpu.py::test_fp8_gemm_edges): v_cvt_pk_fp8_f32 itself does
        not saturate -- every element with |tt| past 448 came back as the NaN code 0x7F (7 of 17680 elements at (130, 136, 512), 708 of
        66820 of the exact set at (257, 260, 256)), and a NaN in the MLP hidden poisons a whole row of the next GEMM.  The epilogue now
        clamps to +-448 in front of the conversion (a NaN stays a NaN).  The quantisers need no clamp: |x * inv| <= 448 (1 + 3 u) there.
"exact" operand set.  Codes with integer values in [-4, 4], sa = 2^(-5 + m % 3), sw = 2^(-4 + n % 3), integer bias in [-2, 2], gate
+-2^{-1, 0, 1}, integer old C in [-8, 8].  Every partial sum of products is an integer of magnitude <= 16 K <= 12288 < 2^24 in any order,
the scaled sum a multiple of 2^-9 below 2^9, the gated sum with the old C a multiple of 2^-10 below 2^11: every float32 operation up to
the output rounding is exact.  Epilogue 3 must match bit for bit, epilogues 0 and 6 the correctly rounded bf16 of the exact value; for
1, 2 and 7 the bounds above hold with E = 0.  No tolerance enters the first three.

Shapes: GEMM_SHAPES, with the reason for each.  Quantiser cases: QUANT_ROWS x QUANT_K with ldx = ldq = K + 8 and row kinds QUANT_KINDS
cycling with the row and the K index (quant_case), so that the 15 cases together hold every kind.
"""
import torch

import edge_bounds as EB
import row_bounds as RB
import row_guard as G
from edge_bounds import S_ERR_F32, U32, worst_ratio  # noqa: F401
from row_bounds import e4m3_decode, e4m3_half_ulp, f32, g

FLOOR = 2.0 ** -126
INV448 = f32(1.0 / 448.0)
OUT_SCALE = f32(0.011)
NAN_CODE = 0x7F

GEMM_SHAPES = (
    (1, 4, 256, "every staging row clamped to row 0; nk = 2, so only the closing phases of the k-loop run"),
    (17, 68, 256, "N % 16 == 4: the narrow 8-byte (bf16) / 4-byte (e4m3) stores and the scale_w + N - 4 clamp"),
    (130, 136, 512, "N % 8 == 0 and ragged; M ends inside an 8-row store group; one full k-loop iteration"),
    (130, 144, 256, "N % 16 == 0 and ragged: the wide e4m3 stores, predicated"),
    (257, 260, 256, "one past the 256 tile both ways; four tiles"),
    (1, 256, 768, "wide stores with 255 rows masked; nk = 6"),
    (255, 256, 512, "an M tail with full columns"),
    (129, 1284, 256, "tiles_n = 6: a ragged last raster group (gn_cur = 2 < GN = 4) under the default gemm_raster"),
)
GEMM_EPILOGUES = (0, 1, 2, 3, 6, 7)
GEMM_REFUSED = (4, 5, 7, 8, 9, 10, 11)
KINDS = ("exact", "random")
OUT_FMT = {0: "bf16", 1: "bf16", 2: "bf16", 3: "f32", 6: "bf16", 7: "u8"}
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8}
LAYOUTS = ("loose", "wide")
GUARD_ROWS = 8
LDA_PAD, LDW_PAD = 16, 32


# ---- e4m3 conversion and the row quantiser ----------------------------------------------------------------------------------------
def e4m3_encode(y, truncate=False):
    """float32 -> e4m3 codes (uint8): nearest, ties to even, saturating at 448, NaN -> 0x7F, the sign kept.  truncate: toward zero."""
    a = y.abs().double()
    pos = RB.E4M3[:127].to(y.device)                         # codes 0x00 .. 0x7E: 0 .. 448, ascending
    hi = torch.searchsorted(pos, a.contiguous()).clamp(1, 126)
    lo = hi - 1
    dl, dh = a - pos[lo], pos[hi] - a
    up = (a >= pos[hi]) if truncate else ((dh < dl) | ((dh == dl) & ((hi & 1) == 0)))
    code = torch.where(up, hi, lo)
    code = torch.where(a >= 448.0, torch.full_like(code, 126), code)
    code = torch.where(torch.isnan(y), torch.full_like(code, NAN_CODE), code)
    return (code | (torch.signbit(y).long() << 7)).to(torch.uint8)


def quant_ref(x):
    """(codes uint8 [rows][K], scale f32 [rows]) of bf16 rows, the kernel's float32 operations one by one (module docstring)"""
    xf = x.float().cpu()
    amax = torch.where(torch.isnan(xf), torch.zeros_like(xf), xf.abs()).amax(-1)
    sc = torch.where(amax > 0, torch.maximum(amax * torch.tensor(INV448), torch.tensor(FLOOR, dtype=torch.float32)), torch.ones_like(amax))
    inv = 1.0 / sc
    return e4m3_encode(xf * inv[:, None]), sc


QUANT_ROWS = (1, 4, 5)
QUANT_K = (8, 504, 512, 520, 1024)
QUANT_PAD = 8
QUANT_KINDS = ("rand-120", "zero", "tiny", "sat", "ties", "rand100", "rand0", "rand-60")


def quant_kind(rows, K, r):
    return QUANT_KINDS[(r + 3 * QUANT_K.index(K) + rows) % len(QUANT_KINDS)]


def quant_row(kind, K, gen):
    """one bf16 row [K] of the kind"""
    if kind.startswith("rand"):
        return (torch.randn(K, generator=gen) * 2.0 ** int(kind[4:])).to(torch.bfloat16)
    if kind == "zero":
        return torch.zeros(K, dtype=torch.bfloat16)
    if kind == "tiny":      # amax = 2^-130 (a bf16 subnormal) and zeros: amax / 448 is a float32 subnormal whose reciprocal is +inf
        base = torch.tensor([2.0 ** -130, 0.0, -2.0 ** -130, 0.0, 2.0 ** -131, 0.0, -2.0 ** -133, 0.0], dtype=torch.float64)
        return base.repeat((K + 7) // 8)[:K].to(torch.bfloat16)
    pos = RB.E4M3[:127]
    if kind == "sat":       # +-448 * 2^3 exactly, and other e4m3 values at the same scale
        v = pos[torch.randint(0, 127, (K,), generator=gen)] * 8.0
    else:                   # "ties": every midpoint between two neighbouring e4m3 values, at the scale 2^-7
        v = (0.5 * (pos[:-1] + pos[1:]))[torch.arange(K) % 126] * 2.0 ** -7
    v = v * (1.0 - 2.0 * torch.randint(0, 2, (K,), generator=gen))
    e = 3 if kind == "sat" else -7
    v[0], v[1] = 448.0 * 2.0 ** e, -448.0 * 2.0 ** e
    out = v.to(torch.bfloat16)
    assert torch.equal(out.double(), v), "the row is not representable in bf16"
    return out


def quant_case(rows, K):
    gen = torch.Generator().manual_seed(7919 * rows + K)
    kinds = [quant_kind(rows, K, r) for r in range(rows)]
    return dict(rows=rows, K=K, kinds=kinds, x=torch.stack([quant_row(k, K, gen) for k in kinds]))


def quant_nonfinite_case():
    """rows with one NaN, one +Inf and one -Inf element among finite ones (K = 16): what include/r3g.h says they do"""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3, 16, generator=gen)
    x[0, 3], x[1, 5], x[2, 9] = float("nan"), float("inf"), float("-inf")
    return x.to(torch.bfloat16)


# ---- GEMM operands ------------------------------------------------------------------------------------------------------------------
def gemm_operands(M, N, K, kind, device="cpu", draw=0):
    gen = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + 7919 * draw + (104729 if kind == "exact" else 0))
    if kind == "exact":
        a8 = e4m3_encode(torch.randint(-4, 5, (M, K), generator=gen).float())
        w8 = e4m3_encode(torch.randint(-4, 5, (N, K), generator=gen).float())
        sa = (2.0 ** (-5 + torch.arange(M) % 3)).float()
        sw = (2.0 ** (-4 + torch.arange(N) % 3)).float()
        bias = torch.randint(-2, 3, (N,), generator=gen).float()
        gate = (1.0 - 2.0 * torch.randint(0, 2, (N,), generator=gen)) * 2.0 ** (torch.randint(0, 3, (N,), generator=gen) - 1.0)
        c0 = torch.randint(-8, 9, (M, N), generator=gen).float()
    else:
        a8, sa = quant_ref(torch.randn(M, K, generator=gen).to(torch.bfloat16))
        w8, sw = quant_ref((torch.randn(N, K, generator=gen) / K ** 0.5).to(torch.bfloat16))
        bias = torch.randn(N, generator=gen)
        gate = torch.randn(N, generator=gen)
        c0 = torch.randn(M, N, generator=gen)
    to = lambda v: v.to(device)
    return dict(M=M, N=N, K=K, kind=kind, a8=to(a8), sa=to(sa), w8=to(w8), sw=to(sw), bias=to(bias), gate=to(gate.float()),
                c0={"f32": to(c0), "bf16": to(c0.to(torch.bfloat16))})


def gemm_lin(ops):
    """lin, t, E in float64 (E = 0 for the exact set)"""
    A, W = e4m3_decode(ops["a8"]), e4m3_decode(ops["w8"])
    s = ops["sa"].double()[:, None] * ops["sw"].double()[None]
    b = ops["bias"].double()
    lin = s * (A @ W.t()) + b
    t = s * (A.abs() @ W.abs().t()) + b.abs()
    E = torch.zeros_like(t) if ops["kind"] == "exact" else (2.0 * ops["K"] + 2.0) * U32 * t
    return lin, t, E


def is_bitwise(ops, epi):
    return ops["kind"] == "exact" and epi in (0, 3, 6)


def gemm_ref_bound(ops, epi, lin_t_e=None):
    """(reference, bound) float64 [M][N].  Epilogue 7: in code space (decoded codes).  Bitwise cases (is_bitwise): (the expected tensor in
    the output type, None)."""
    lte = lin_t_e if lin_t_e is not None else gemm_lin(ops)
    lin, t, E = lte
    if is_bitwise(ops, epi):
        exact = lin if epi == 0 else ops["c0"][OUT_FMT[epi]].double() + ops["gate"].double() * lin
        assert torch.equal(exact.float().double(), exact), "the exact set is not exact in float32"
        return exact.float().to(TORCH_DTYPE[OUT_FMT[epi]]), None
    if epi != 7:
        return EB.gemm_ref_bound(ops, epi, gelu_pk=False, lin_t_e=lte)
    ref = EB.gelu64(lin, False)
    eg = 1.13 * E + S_ERR_F32 * (lin.abs() + E) + 2 * U32 * ref.abs()
    tt = ref / OUT_SCALE
    e_t = eg / OUT_SCALE + g(2) * (tt.abs() + eg / OUT_SCALE)
    return tt.clamp(-448.0, 448.0), e4m3_half_ulp((tt.abs() + e_t).clamp_max(448.0)) + e_t


# ---- the guarded C and its verdict (shared by the CPU emulation and the GPU launches) ---------------------------------------------
def c_layout(ops, epi, layout):
    """(elements in front of C, ldc) -- loose: four elements in front, ldc = N + 4; wide: 16-byte aligned, ldc = N + 8 (e4m3: N + 16 bytes)"""
    if layout == "loose":
        return 4, ops["N"] + 4
    off = 16 if epi == 7 else 8
    return off, ops["N"] + off


def c_buffer(ops, epi, layout, device="cpu"):
    """(flat, C [M + 8][ldc], ldc, off): the guard pattern everywhere, the old values inside for the residual epilogues"""
    fmt = OUT_FMT[epi]
    off, ldc = c_layout(ops, epi, layout)
    M, N = ops["M"], ops["N"]
    flat = torch.empty(off + (M + GUARD_ROWS) * ldc, device=device, dtype=TORCH_DTYPE[fmt])
    G.bits(torch, flat).fill_(G.pattern(torch, flat.dtype))
    C = flat[off:].view(M + GUARD_ROWS, ldc)
    if epi in (3, 6):
        C[:M, :N] = ops["c0"][fmt]
    return flat, C, ldc, off


def verdict(ops, epi, flat, C, off, ref, bound):
    """(error / bound -- 0 or inf for the bitwise cases --, complaints) of one finished launch"""
    M, N = ops["M"], ops["N"]
    out, got = [], C[:M, :N]
    if bound is None:
        same = G.bits(torch, got.contiguous()) == G.bits(torch, ref.contiguous())
        r = 0.0 if bool(same.all()) else float("inf")
        if r:
            i = int((~same).reshape(-1).nonzero()[0])
            out.append("%d of %d elements differ from the exact result, the first at (%d, %d): %r for %r" % (
                int((~same).sum()), M * N, i // N, i % N, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i])))
    else:
        val = e4m3_decode(got) if epi == 7 else got.double()
        d = (val - ref).abs() / bound
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
        r = float(d.max())
        if not r <= 1.0:
            i = int(d.argmax())
            out.append("error / bound %.3f at (%d, %d), %d of %d elements outside" % (r, i // N, i % N, int((d > 1.0).sum()), M * N))
    bad = G.bits(torch, flat) != G.pattern(torch, flat.dtype)
    bad[off:].view(C.shape)[:M, :N] = False
    if bool(bad.any()):
        j = int(bad.nonzero()[0]) - off
        out.append("%d elements outside [M) x [N) were written, the first at row %d column %d" % (int(bad.sum()), j // C.shape[1], j % C.shape[1]))
    return r, out


def gemm_coverage(reached):
    """reached: iterable of (epilogue, M, N, K, store path "wide" | "narrow").  What the closing test asserts, as complaints."""
    out = []
    for epi in GEMM_EPILOGUES:
        mine = [(M, N, K, p) for e, M, N, K, p in reached if e == epi]
        for what, ok in (("an M tail", any(M % 256 for M, N, K, p in mine)),
                         ("an N tail with N % 16 == 4", any(N % 256 and N % 16 == 4 for M, N, K, p in mine)),
                         ("an N tail with N % 16 == 0", any(N % 256 and N % 16 == 0 for M, N, K, p in mine)),
                         ("nk = 2", any(K == 256 for M, N, K, p in mine)), ("nk > 2", any(K > 256 for M, N, K, p in mine)),
                         ("the wide stores", any(p == "wide" for M, N, K, p in mine)),
                         ("the narrow stores", any(p == "narrow" for M, N, K, p in mine))):
            if not ok:
                out.append("epilogue %d: never reached with %s" % (epi, what))
    return out


def store_path(epi, N, layout, wide_switch):
    """gemm_epilogue's choice restated: the LDS-transposed ("wide") stores or the per-lane ("narrow") ones.  The 16-bit and e4m3 outputs
    need a 16-byte aligned C (the wide layout) and N % 8 == 0 (e4m3: N % 16 == 0); epilogue 3 stores 16 bytes per lane either way and
    transposes whenever C is 16-byte aligned, which include/r3g.h demands of it: both layouts."""
    if not wide_switch:
        return "narrow"
    if epi == 3:
        return "wide"
    return "wide" if (layout == "wide" and N % (16 if epi == 7 else 8) == 0) else "narrow"


REFUSED_ENTRIES = ((0, 2), (6, 2), (3, 4), ("e4m3", 1))       # (epilogue | the e4m3 entry point, bytes per element of C)
ADMITTED_EMPTY = (("m == 0", dict(m=0)), ("n == 0", dict(n=0)), ("m == 0 with null operands", dict(m=0, a=None, c=None)))


def gemm_refusals(epi, esz, a, N, K):
    """{what: arguments to replace} -- one violation of the contract of include/r3g.h each, from the admitted arguments `a` (addresses a, w,
    sa, sw, bias, gate, c; strides lda, ldw, ldc).  Checked before anything touches the GPU: tests/test_fp8_bounds_cpu.py runs them
    against the library without one, tests/test_fp8_edges_gpu.py with the guards watched."""
    bad = {"m < 0": dict(m=-1), "n < 0": dict(n=-4), "k == 0": dict(k=0), "k < 256": dict(k=128), "k % 256": dict(k=384), "n % 4": dict(n=N - 2),
           "lda % 16": dict(lda=a["lda"] + 8), "lda < k": dict(lda=K - 16), "ldw % 16": dict(ldw=a["ldw"] + 8), "ldw < k": dict(ldw=K - 16),
           "a8 8 bytes off": dict(a=a["a"] + 8), "w8 8 bytes off": dict(w=a["w"] + 8),
           "scale_w 4 bytes off": dict(sw=a["sw"] + 4), "scale_a 2 bytes off": dict(sa=a["sa"] + 2), "bias 4 bytes off": dict(bias=a["bias"] + 4),
           "ldc % 4": dict(ldc=a["ldc"] + 2), "ldc < n": dict(ldc=N - 4), "c two elements off": dict(c=a["c"] + 2 * esz),
           "a8 null": dict(a=None), "w8 null": dict(w=None), "scale_a null": dict(sa=None), "scale_w null": dict(sw=None), "c null": dict(c=None)}
    if epi in (3, 6):
        bad["gate 4 bytes off"] = dict(gate=a["gate"] + 4)
    if epi == "e4m3":
        for v in (0.0, -0.011, float("inf"), float("nan")):
            bad["out_scale %r" % v] = dict(out_scale=v)
    else:
        for e in GEMM_REFUSED:
            bad["epilogue %d" % e] = dict(epi=e)
    return bad


def gemm_abi_call(L, epi0, stream, a):
    """the ABI call with the arguments `a` as a closure (epi "e4m3": r3g_op_gemm_fp8_e4m3)"""
    import ctypes
    a = dict(dict(epi=epi0, out_scale=OUT_SCALE), **a)
    if a["epi"] == "e4m3":
        return lambda: L.r3g_op_gemm_fp8_e4m3(a["a"], a["lda"], a["sa"], a["w"], a["ldw"], a["sw"], a["bias"], a["c"], a["ldc"],
                                              ctypes.c_float(a["out_scale"]), a["m"], a["n"], a["k"], stream)
    return lambda: L.r3g_op_gemm_fp8(a["a"], a["lda"], a["sa"], a["w"], a["ldw"], a["sw"], a["bias"], a["c"], a["ldc"], a.get("gate"),
                                     a["m"], a["n"], a["k"], a["epi"], stream)
