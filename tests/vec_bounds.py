"""Float64 references and ELEMENT-WISE bounds for the small kernels of a sampling step and of input staging -- gemv, gemv_multi,
timestep_embedding, fourier_grid, fourier_points, cfg_euler, euler_step (both kernels), nonfinite_flag, cast_pad, fill_rows, add_rows,
f32_to_bf16, the patch rows of im2col_kernel and the in-place vec_add (csrc/elem.hip), the out-of-place vec_add (csrc/conv_kernels.hip) --
shared by tests/test_vec_bounds_cpu.py (the bounds are neither vacuous nor unreachable) and tests/test_vec_kernels_gpu.py (every kernel
through its r3g_op_* entry point).

Conventions of tests/row_bounds.py: plain torch float64 on whatever device the operands live on, operands drawn on the CPU from seeds,
every bound DERIVED from the arithmetic read in the kernel and none measured, every margin factor named where it enters.  u = 2^-24, g(k),
MUL and ADD (one separately rounded product / sum of two (value, error) pairs; a fused multiply-add errs by less than MUL then ADD),
bf16_bound, SILU_ERR and SILU_SLOPE are row_bounds' own.

LIBM_ULPS = 4.  expf, sinf, cosf (and the constant logf(10000.0f)) are the device library's; its accuracy table states them in ulps of the
result, small integers.  That table was looked for among the documents installed with the toolkit and is not there, so the figure is NOT
taken from a file: 4 is a margin over the library's nominal small-integer figure.  One ulp of a float32 result r is at most 2 u |r|, so a
library result errs by at most LIBM_ULPS 2 u |r|.  The choice decides no verdict: in the Fourier embeddings the bf16 rounding (2^-9
relative) exceeds it by 2^13, in the timestep embedding the error of the float32 argument does.

BIT-EXACT KERNELS: one IEEE operation, or a copy, per element; the expected values are a float32 torch emulation compared as bit patterns.
  cast_pad      bf16(in * scale): one float32 product, then round to nearest even (torch's .to(bfloat16)); columns [C, Cpad) are zero bits.
  fill_rows     dst[r][c] = vals[c].        add_rows  x[r][c] + pos[r][c], one float32 sum.        vec_add (both forms)  one float32 sum.
  f32_to_bf16   round to nearest even.  F2B_SPECIALS: +-0, +-inf, a quiet NaN and a NaN with only low mantissa bits set (truncating it
                would give an infinity; each must stay a NaN: NaNs are compared as "is a NaN", every other element by its bits), exact
                ties in both directions, a rounding that carries into the exponent, and the largest finite float32, which rounds to
                inf.  Float32 DENORMALS ARE LEFT OUT: no caller produces them, and their handling is the compiler's default mode.
  patch_rows    out[(py, px)][(ch ps + dy) ps + dx] = bf16(img[ch][py ps + dy][px ps + dx]); columns [3 ps^2, Kpad) are zero bits.
  nonfinite_flag  the flag becomes old | 1 iff some element has all eight exponent bits set, and is never cleared; large finite values and
                denormals do not set it.

EULER STEPS.  lat + ds v is MUL(ds, v) then ADD(lat, .); lat + ds (vu + g (vc - vu)) is ADD(vc, -vu), MUL(g, .), ADD(vu, .), MUL(ds, .),
ADD(lat, .).  elem.hip is built with the default -ffp-contract, so any of these may be contracted into an FMA, which errs by less: the
chains cover both forms.  The float4 kernel and the one-element-per-lane kernel get the same bound.  The output is float32: no further
rounding.  cfg_euler reads the conditional half at [0, n) and the unconditional one at [n, 2 n): the halves are drawn around -2 and around
+3, so that exchanging them moves every element by about 5 |ds| (and at ds = 0 nothing reads them).

GEMV (gemv_kernel, gemv_multi_kernel).  The weights are bf16 and exact.  An input is silu(x) with error SILU_ERR |x| when silu_in is set,
x itself (error 0) otherwise.  Lane l adds the eight terms at k = 8 l + 512 s for every stride s: 8 ceil(K / 512) fused terms (gemv_multi
adds two products and then their sum: no more roundings per term), then the six levels of wave_sum, then the bias:
    e = sum |w| e_x + g(8 ceil(K / 512) + 7) (sum |w x| + sum |w| e_x + |bias|)
silu_out: SILU_SLOPE e + SILU_ERR |v|.  The output is float32 and is not rounded further.

TIMESTEP EMBEDDING.  out[b][c] = cos (c < 128) | sin of a = t tf exp(-ln(10000) j / 128), j = c mod 128; the reference takes t and tf
as the float32 values they are and everything else in float64.  The kernel's float32 argument:
    L^ = logf(10000.0f), a float32 constant: e_L = LIBM_ULPS 2 u L          p = L^ j: MUL          q = p / 128: exact
    f^ = expf(q^): |f^ - f| <= f (expm1(e_q) + LIBM_ULPS 2 u exp(e_q))       a^ = (t tf) f^: MUL, MUL
    out: |cos a^ - cos a| <= e_a (the slope is at most 1), and the library's own LIBM_ULPS 2 u (|ref| + e_a)
At t = 1, tf = 1000 and j = 0 that is about 6e-4, nearly all of it e_a = 1000 (8 u + 2 u): inherent to a float32 argument of size 1000,
and the torch oracle (oracle/hy3d_torch.py) has the same.  At t = 0 the argument is an exact zero: cos must be 1.0 and sin 0.0 exactly
(e_a = 0: the bound is 8 u for cos and 0 for sin, and worst() counts an exact hit as ratio 0 whatever the bound).

FOURIER EMBEDDINGS (fourier_grid_kernel, fourier_points_kernel).  Row of lattice point idx = (i (R + 1) + j) (R + 1) + k:
    [x y z | sin(x_c fr_f): c major, f minor | cos likewise | zeros up to 64],  fr_f = 2^f, times float32(pi) when include_pi.
  coordinates  np.linspace(-bound, bound, R + 1, dtype=np.float32) BIT FOR BIT (lin_coord's float64 i * step - bound, the last one pinned
               to bound), stored as bf16: compared as bits.
  argument     coord * fr: ONE float32 product with a frequency that is exact in float32 (a power of two times the float32 pi) -- the
               same product the torch oracle forms.  It is computed here in float32 on the CPU, and the reference is float64 sin / cos
               of THAT float32 argument, so no argument error enters.
  bound        bf16_bound(ref, LIBM_ULPS 2 u |ref|)
  rows outside a row at or past (R + 1)^3, and a row in [count, rows) of fourier_points, is the embedding of the origin, bit for bit
               (zeros, cos = 1.0).  A listed point's row equals the dense kernel's row for that index, bit for bit.

LAUNCH RULES, restated as row_bounds.ln_form restates layernorm_launch: gemv_blocks (256 blocks from N = 1024 on, a grid-stride loop over
the rows; ceil(N / 4) below) and euler_form (the scalar kernel iff either pointer is not 16-byte aligned).
"""
import math

import numpy as np
import torch

from row_bounds import ADD, MUL, SILU_ERR, SILU_SLOPE, U32, bf16_bound, f32, g, half_ulp, worst_ratio  # noqa: F401  (re-exported for the tests)

LIBM_ULPS = 4.0
ULP = 2.0 * U32                 # one unit in the last place of a float32 r is at most ULP |r|
PI32 = float(torch.tensor(math.pi, dtype=torch.float32))


def worst(got, ref, bound):
    """worst_ratio, with an exact hit counted as ratio 0 whatever the bound (a bound may be zero where the result must be exact)"""
    d = (got.double() - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def ibits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def bit_mismatches(got, want):
    """number of elements whose bit patterns differ"""
    return int((ibits(got) != ibits(want)).sum())


def _dev(d, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}


# ---- gemv / gemv_multi --------------------------------------------------------------------------------------------------------------
GEMV_B = (1, 3, 8)
GEMV_K = (8, 256, 520, 1032)
GEMV_N = (1, 5, 1023, 1029)
GEMV_PAD = 8                                            # ldw = K + 8
# (B, K, N, silu_in, silu_out, bias): the full cross at silu 0 / 0 with a bias; every other flag combination, and a null bias, at two shapes
GEMV_EXTRA = tuple((B, K, N, si, so, 1) for (B, K, N) in ((3, 520, 5), (8, 1032, 1029)) for (si, so) in ((1, 0), (0, 1), (1, 1))) + \
    ((3, 520, 5, 0, 0, 0), (1, 256, 1029, 1, 1, 0))


def gemv_plan():
    for B in GEMV_B:
        for K in GEMV_K:
            for N in GEMV_N:
                yield B, K, N, 0, 0, 1
    for c in GEMV_EXTRA:
        yield c


def gemv_blocks(N):
    """gemv_launch's grid, restated"""
    return 256 if N >= 1024 else (N + 3) // 4


def gemv_matrix(K, N, seed=0):
    """(w bf16 [N][K], bias f32 [N]) -- a function of (K, N) alone, shared by every launch of that matrix"""
    gen = torch.Generator().manual_seed(2750159 * K + 31 * N + 1000003 * seed)
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(torch.bfloat16)
    return w, 0.5 * torch.randn(N, generator=gen)


def gemv_input(B, K):
    gen = torch.Generator().manual_seed(3497861 * B + K)
    return 1.5 * torch.randn(B, K, generator=gen)


def gemv_case(B, K, N, silu_in, silu_out, bias, device="cpu"):
    w, b = gemv_matrix(K, N)
    return _dev(dict(B=B, K=K, N=N, silu_in=silu_in, silu_out=silu_out, x=gemv_input(B, K), w=w, bias=b if bias else None), device)


def gemv_ref_bound(x, w, bias, K, silu_in, silu_out):
    """(reference, bound) float64 [B][N] of act_out(act_in(x) w^T + bias)"""
    x, w = x.double(), w.double()
    e_x = torch.zeros_like(x)
    if silu_in:
        e_x = SILU_ERR * x.abs()
        x = x * torch.sigmoid(x)
    v = x @ w.t()
    t = x.abs() @ w.abs().t()
    carried = e_x @ w.abs().t()
    babs = 0.0
    if bias is not None:
        v = v + bias.double()
        babs = bias.double().abs()
    e = carried + g(8 * ((K + 511) // 512) + 7) * (t + carried + babs)
    if silu_out:
        return v * torch.sigmoid(v), SILU_SLOPE * e + SILU_ERR * v.abs()
    return v, e


GEMVM_B = (1, 2)
GEMVM_K = (8, 520)
GEMVM_N = (1, 5, 261)
GEMVM_PADS = (8, 16, 24)                                # ldw = K + pad: distinct per job
GEMVM_NULL_BIAS = 1                                     # the job without a bias


def gemvm_layout(B):
    """out_off of the three jobs: not in job order, gaps between them (job j owns [off, off + B N_j))"""
    return (2 * B * 261 + 24, 7, B * 5 + 16 + 7), 2 * B * 261 + 24 + B * 1 + 9      # (offsets of jobs N = 1, 5, 261; total elements)


def gemvm_case(B, K, silu_in, device="cpu"):
    offs, total = gemvm_layout(B)
    jobs = []
    for j, N in enumerate(GEMVM_N):
        w, b = gemv_matrix(K, N, seed=1 + j)
        jobs.append(_dev(dict(N=N, w=w, bias=None if j == GEMVM_NULL_BIAS else b, ldw=K + GEMVM_PADS[j], off=offs[j]), device))
    return dict(B=B, K=K, silu_in=silu_in, x=gemv_input(B, K).to(device), jobs=jobs, total=total)


def gemvm_owned(case, j):
    """flat element indices [B][N_j] of job j's outputs"""
    job = case["jobs"][j]
    dev = case["x"].device
    return job["off"] + torch.arange(case["B"], device=dev)[:, None] * job["N"] + torch.arange(job["N"], device=dev)[None]


# ---- timestep embedding -------------------------------------------------------------------------------------------------------------
TS_B = (1, 3)
TS_T = (0.0, 1e-3, 0.37, 1.0)
TS_TF = (1000.0, 1.0)


def ts_times(B, t):
    """t [B] float32: the value itself, then smaller ones (a device array whose entries differ: row b must read t[b])"""
    return torch.tensor([t * (1.0 - 0.25 * b) for b in range(B)], dtype=torch.float32)


def ts_ref_bound(t, tf):
    """t: float32 tensor [B]; tf: python float (a float32 value) -> (reference, bound) float64 [B][256]"""
    t = t.double()[:, None]
    j = torch.arange(128, dtype=torch.float64, device=t.device)[None]
    L = math.log(10000.0)
    zero = torch.zeros_like(j)
    p, e_p = MUL(torch.full_like(j, L), torch.full_like(j, LIBM_ULPS * ULP * L), j, zero)
    q, e_q = -p / 128.0, e_p / 128.0
    f = torch.exp(q)
    e_f = f * (torch.expm1(e_q) + LIBM_ULPS * ULP * torch.exp(e_q))
    tt, e_tt = MUL(t, torch.zeros_like(t), torch.full_like(t, tf), torch.zeros_like(t))
    a, e_a = MUL(tt.expand(-1, 128), e_tt.expand(-1, 128), f.expand(t.shape[0], -1), e_f.expand(t.shape[0], -1))
    ref = torch.cat([torch.cos(a), torch.sin(a)], -1)
    e_a = torch.cat([e_a, e_a], -1)
    return ref, e_a + LIBM_ULPS * ULP * (ref.abs() + e_a)


# ---- Fourier embeddings -------------------------------------------------------------------------------------------------------------
FOURIER_GRIDS = ((1, 1.0), (7, 1.01), (8, 1.05))        # whole lattice + FOURIER_BEHIND rows, in two calls
FOURIER_BIG = (512, 1.01)                               # windows only
FOURIER_BEHIND = 40
FOURIER_NF = (0, 1, 8, 10)
FOURIER_LISTS = (1, 37, 300)
FOURIER_ROWS_EXTRA = 27


def fourier_split(R):
    """where the two dense calls over [0, (R + 1)^3 + 40) part: inside the lattice, not a multiple of 256 (nor of R + 1)"""
    return {1: 3, 7: 301, 8: 515}[R]


def fourier_big_windows():
    """(start, count) of the dense calls at R = 512: the first rows, rows in the middle, and the last 100 lattice rows with 200 behind"""
    n3 = 513 ** 3
    return ((0, 300), (n3 // 2 - 77, 300), (n3 - 100, 300))


def lin_coords(R, bound):
    """float32 tensor [R + 1]: the coordinates as the reference's numpy call gives them"""
    return torch.from_numpy(np.linspace(-bound, bound, R + 1, dtype=np.float32).copy())


def fourier_freqs(nf, pi):
    fr = torch.tensor([float(1 << f) for f in range(nf)], dtype=torch.float32)
    return fr * torch.tensor(PI32, dtype=torch.float32) if pi else fr          # (a power of two times float32(pi): exact)


def fourier_xyz(idx, R, coords):
    """float32 [n][3] of the lattice points idx (int64 [n], on coords' device); a point at or past (R + 1)^3 is the origin"""
    n = R + 1
    ii, jj, kk = idx // (n * n), (idx // n) % n, idx % n
    inside = (ii < n)[:, None]
    xyz = torch.stack([coords[ii.clamp_max(R)], coords[jj], coords[kk]], -1)
    return torch.where(inside, xyz, torch.zeros_like(xyz))


def fourier_ref_bound(xyz, nf, pi):
    """xyz float32 [n][3] -> (ref float64 [n][64], bound float64 [n][64], exact bool [64]: channels compared as bits -- xyz and the zeros)"""
    n, dev = xyz.shape[0], xyz.device
    ref = torch.zeros(n, 64, dtype=torch.float64, device=dev)
    exact = torch.ones(64, dtype=torch.bool, device=dev)
    ref[:, :3] = xyz.to(torch.bfloat16).double()
    if nf:
        arg = (xyz[:, :, None] * fourier_freqs(nf, pi).to(dev)[None, None, :]).reshape(n, 3 * nf).double()      # the float32 product, c major
        ref[:, 3:3 + 3 * nf] = torch.sin(arg)
        ref[:, 3 + 3 * nf:3 + 6 * nf] = torch.cos(arg)
        exact[3:3 + 6 * nf] = False
    return ref, bf16_bound(ref, LIBM_ULPS * ULP * ref.abs()), exact


def fourier_check(got, ref, bound, exact):
    """got bf16 [n][64] -> (worst error / bound over the sin / cos channels, bit mismatches over the exact channels)"""
    r = worst(got[:, ~exact], ref[:, ~exact], bound[:, ~exact]) if bool((~exact).any()) else 0.0
    return r, bit_mismatches(got[:, exact], ref[:, exact].to(torch.bfloat16))


def fourier_list(R, count, seed=0):
    """count lattice indices (int64) in random order, with repeats from three entries on, holding 0 and (R + 1)^3 - 1 from two on (the one-
    entry list holds the last point); at R = 512 drawn from fourier_big_windows so that the dense rows are there to compare with"""
    gen = torch.Generator().manual_seed(6700417 * R + count + 1000003 * seed)
    n3 = (R + 1) ** 3
    if R == FOURIER_BIG[0]:
        pool = torch.cat([torch.arange(s, min(s + c, n3)) for s, c in fourier_big_windows()])
    else:
        pool = torch.arange(n3)
    idx = pool[torch.randint(0, pool.numel(), (count,), generator=gen)]
    idx[0] = n3 - 1
    if count >= 2:
        idx[1] = 0
    if count >= 3:
        idx[2] = idx[count // 2]                     # a repeat
    return idx[torch.randperm(count, generator=gen)]


# ---- Euler steps ------------------------------------------------------------------------------------------------------------------------
EULER_N = (1, 3, 4, 5, 1023, 1024, 1027)
EULER_ALIGN = ("aligned", "lat_off", "v_off")
CFG_N = (1, 255, 257, 1027)
CFG_G = (0.0, 1.0, 5.0)
DS = (f32(-0.02), 0.0)


def euler_form(lat_addr, v_addr):
    """euler_step_launch's rule, restated: "scalar" iff either address is not 16-byte aligned"""
    return "scalar" if ((lat_addr | v_addr) & 15) else "vec"


def euler_case(n, device="cpu"):
    gen = torch.Generator().manual_seed(9999991 + n)
    return dict(n=n, lat=torch.randn(n, generator=gen).to(device), v=(2.0 * torch.randn(n, generator=gen)).to(device))


def euler_ref_bound(lat, v, ds):
    lat, v = lat.double(), v.double()
    z = torch.zeros_like(v)
    p, e = MUL(torch.full_like(v, ds), z, v, z)
    return ADD(lat, z, p, e)


def cfg_case(n, device="cpu"):
    """v2 [2 n]: the conditional half around -2, the unconditional one around +3"""
    gen = torch.Generator().manual_seed(15485867 + n)
    lat = torch.randn(n, generator=gen)
    v2 = torch.cat([torch.randn(n, generator=gen) * 0.5 - 2.0, torch.randn(n, generator=gen) * 0.5 + 3.0])
    return dict(n=n, lat=lat.to(device), v2=v2.to(device))


def cfg_ref_bound(lat, v2, gd, ds):
    n = lat.numel()
    lat, vc, vu = lat.double(), v2[:n].double(), v2[n:].double()
    z = torch.zeros_like(lat)
    d, e = ADD(vc, z, -vu, z)
    d, e = MUL(torch.full_like(d, gd), z, d, e)
    d, e = ADD(vu, z, d, e)
    d, e = MUL(torch.full_like(d, ds), z, d, e)
    return ADD(lat, z, d, e)


# ---- nonfinite_flag ---------------------------------------------------------------------------------------------------------------------
NF_N = (1, 63, 257, 262145)
NF_BAD = (float("inf"), float("-inf"), float("nan"))
NF_OLD = (0, 2)


def nf_positions(n):
    return sorted({0, n // 2, n - 1})


def nf_vector(n, device="cpu"):
    """finite values only: normals, the largest finite float32 (both signs) and denormals -- none of which sets the flag"""
    gen = torch.Generator().manual_seed(32452867 + n)
    x = torch.randn(n, generator=gen)
    big = torch.tensor([0x7F7FFFFF, -8388609, 1, -2147483647, 0x007FFFFF], dtype=torch.int32).view(torch.float32)   # +-max, +-min denormal, max denormal
    pos = torch.randperm(n, generator=gen)[:min(n, 5)]
    x[pos] = big[:pos.numel()]
    return x.to(device)


def nf_expected(x, old):
    bad = bool(((ibits(x) & 0x7F800000) == 0x7F800000).any())
    return old | 1 if bad else old


# ---- bit-exact copies and casts ---------------------------------------------------------------------------------------------------------
CAST_ROWS = (1, 3)
CAST_CC = ((3, 8), (4, 64), (64, 64), (5, 72))
CAST_SCALE = (1.0, f32(0.18215))
CAST_LDI_PAD = (0, 3)
CAST_LDO_PAD = 8
ROWS_ROWS = (1, 3)
ROWS_C = (1, 5, 260)
ROWS_PAD = 3
VADD_N = (1, 255, 257)
F2B_N = (1, 257)
PATCH_SHAPES = ((4, 2, 16), (28, 14, 592), (6, 2, 12))


def cast_case(rows, C, device="cpu"):
    gen = torch.Generator().manual_seed(49979693 * rows + C)
    x = torch.randn(rows, C, generator=gen) * 3.0
    x.view(-1)[0] = 1.00390625              # a tie at scale 1: 1 + 2^-8 lies midway between two bf16 values (to even: 1.0)
    return x.to(device)


def cast_expected(x, scale):
    return (x * torch.tensor(scale, dtype=torch.float32, device=x.device)).to(torch.bfloat16)


def rows_case(rows, C, device="cpu"):
    gen = torch.Generator().manual_seed(67867979 * rows + C)
    return torch.randn(rows, C, generator=gen).to(device), torch.randn(rows, C, generator=gen).to(device), torch.randn(C, generator=gen).to(device)


def vadd_case(n, device="cpu"):
    gen = torch.Generator().manual_seed(86028157 + n)
    return torch.randn(n, generator=gen).to(device), (torch.randn(n, generator=gen) * 1e-3).to(device)


F2B_SPECIALS = torch.tensor([
    0x00000000, -2147483648,            # +-0
    0x7F800000, -8388608,               # +-inf
    0x7FC00000, 0x7F800001,             # a quiet NaN; a NaN with only a low mantissa bit set
    0x3F808000, 0x3F818000,             # ties: 1 + 2^-8 -> 1.0 (down to even), 1 + 3 2^-8 -> 1 + 2^-6 (up to even)
    -1082097664, -1082032128,           # the same two, negative
    0x3FFFFFFF,                         # rounds up with a carry into the exponent: 2.0
    0x3F807FFF, 0x3F808001,             # one float32 step below / above the tie
    0x7F7FFFFF, -8388609,               # +-the largest finite float32: rounds to +-inf
], dtype=torch.int32).view(torch.float32)


def f2b_case(n, device="cpu"):
    gen = torch.Generator().manual_seed(104395303 + n)
    return (torch.randn(n, generator=gen) * 7.0).to(device)


def f2b_mismatches(got, x):
    """elements of got (bf16) that differ from round-to-nearest-even of x: a NaN must be a NaN, anything else must match to the bit"""
    want = x.to(torch.bfloat16)
    nan = torch.isnan(x)
    return int((torch.isnan(got.float()) != nan).sum()) + int(((ibits(got) != ibits(want)) & ~nan).sum())


def patch_case(S, device="cpu"):
    gen = torch.Generator().manual_seed(122949829 + S)
    return torch.randn(3, S, S, generator=gen).to(device)


def patch_expected(img, S, ps, Kpad):
    """bf16 [(S / ps)^2][Kpad], spelled out by indexing, independently of the kernel's index arithmetic"""
    P = S // ps
    p = img.view(3, P, ps, P, ps).permute(1, 3, 0, 2, 4).reshape(P * P, 3 * ps * ps)      # [py][px][ch][dy][dx]
    out = torch.zeros(P * P, Kpad, dtype=torch.bfloat16, device=img.device)
    out[:, :3 * ps * ps] = p.to(torch.bfloat16)
    return out
