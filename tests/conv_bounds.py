"""Float64 reference, ELEMENT-WISE error bound and restated launch rules of the texture stage's 3 x 3 convolution (r3g_op_conv3x3:
conv_gemm_kernel, or im2col3x3_kernel + the GEMM, either as a split-K launch with splitk_reduce_kernel), shared by
tests/test_conv_bounds_cpu.py (the bound is neither unreachable nor vacuous) and tests/test_conv_edges_gpu.py.

Everything here is plain torch on the CPU; nothing needs a GPU.

Reference.  torch.nn.functional.conv2d in float64 on NCHW tensors, the formulation diffusers runs: the rows x [nb][H*W][cin] are
permuted to [nb][cin][H][W], the weights w [cout][ky][kx][cin] back to [O][I][3][3]; pad 1 is padding=1, pad 0 is an explicit
F.pad(x, (0, 1, 0, 1)) in front of an unpadded convolution.  It shares no indexing with the kernel's gather or with im2col.

Bound.  The convolution is a GEMM with K = 9 cin, so the derivation at the top of tests/edge_bounds.py applies unchanged
(u = 2^-24 = EB.U32):
    lin = conv2d(x, w) + bias        t = conv2d(|x|, |w|) + |bias|        E = 2 K u t
    epilogue 4 (fp32 store)        |c - lin| <= E
    epilogue 3 (fp32 residual)     ref = c0 + lin,  |c - ref| <= E + 3 u (|c0| + |lin|)       (r3g_op_conv3x3 carries no gate: 1)
The factor 2 of E is edge_bounds' existing one (the MFMA's unspecified inner order); no other margin enters.  A padded tap adds exact
zeros on both sides.  Split-K: with S slices each slice sums K / S products (2 (K / S) u t_s over the slices adds up to 2 (K / S) u t)
and splitk_reduce_kernel adds S partial sums and the bias in fp32 (at most S u t more): 2 (K / S) u t + S u t.  That is below E
whenever S <= 2 K (1 - 1 / S), and every slice keeps at least 8 k-steps = 512 columns (K / S >= 512, so S <= K / 512): the one bound E
holds for every S, and the tests use it for split and unsplit launches alike.

Restated rules (csrc/unet.cpp: conv3x3_run, csrc/gemm.hip: splitk128_factor, gemm_auto_takes_256): out_hw, splitk128_factor,
expected_slices, expected_implicit.
"""
import torch
import torch.nn.functional as F

import edge_bounds as EB
import row_guard as G

GUARD_ROWS = 8                 # rows of guard pattern behind row M of C
LDC_PAD = 4                    # ldc = cout + 4
F32_GUARD = G.GUARD_BITS["f32"]

# (nb, H, W, cin, cout, stride, pad, what the shape is for).  The largest operand is the weight of the last row (64 x 9216 bf16, 1.2 MB).
SHAPES = (
    (1, 1, 1, 64, 4, 1, 1, "one row, one 4-column group, smallest K (576); eight of nine taps are padding"),
    (1, 2, 1, 64, 64, 1, 1, "W = 1: left and right taps are both padding"),
    (1, 5, 7, 64, 68, 1, 1, "M = 35 < 128, clamped staging rows, narrow N tail"),
    (3, 7, 9, 64, 132, 1, 1, "M = 189: the first tile spans two sample boundaries, second M tile of 61 rows, second N tile of 4 columns"),
    (2, 5, 7, 128, 64, 2, 1, "stride 2, odd map"),
    (2, 6, 8, 128, 64, 2, 1, "stride 2, even map"),
    (2, 6, 8, 128, 64, 2, 0, "one-sided padding, last window reads the pad row / column"),
    (2, 5, 7, 128, 64, 2, 0, "one-sided padding, no window reaches the pad"),
    (2, 5, 7, 256, 64, 1, 1, "smallest split: K = 2304, S = 4, slices of 576 begin mid-tap"),
    (1, 9, 15, 320, 132, 1, 1, "the model's width: S = 5, mid-tap, M and N tails under a split"),
    (2, 4, 4, 512, 64, 2, 1, "S = 9, every slice one whole tap, stride 2"),
    (1, 3, 3, 1024, 64, 1, 1, "S = 18, slices of half a tap"),
)
NO_WORKSPACE = 8               # index of the cin = 256 row, which also runs without a workspace: one launch over 36 k-steps
EPILOGUES = (4, 3)


def out_hw(H, W, stride, pad):
    """output geometry: pad rows / columns of zeros in front, one behind, a 3-wide window"""
    return (H + pad - 2) // stride + 1, (W + pad - 2) // stride + 1


def geometry(shape):
    nb, H, W, cin, cout, stride, pad = shape[:7]
    Ho, Wo = out_hw(H, W, stride, pad)
    return dict(nb=nb, H=H, W=W, cin=cin, cout=cout, stride=stride, pad=pad, Ho=Ho, Wo=Wo, M=nb * Ho * Wo, N=cout, K=9 * cin)


def splitk128_factor(M, N, K, num_cu=256):
    """csrc/gemm.hip: the largest divisor S of K / 64 with S * tiles <= 512 slots (at 256 CUs) and >= 8 k-steps per slice; two slices only
    from K = 4096; 1: no split"""
    if K < 2048 or K % 64:
        return 1
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    slots = 512 * num_cu // 256
    if tiles * 2 > slots:
        return 1
    nk, best = K // 64, 1
    for S in range(2, 65):
        if S * tiles > slots or nk // S < 8:
            break
        if nk % S == 0:
            best = S
    if best == 2 and K < 4096:
        best = 1
    return best


def expected_slices(M, N, K, ws_elems, num_cu=256):
    """the slices a launch runs with under the default switches: the rule's, unless the workspace cannot hold them"""
    S = splitk128_factor(M, N, K, num_cu) if ws_elems > 0 else 1
    return S if S * M * N <= ws_elems else 1


def auto_takes_256(M, N, K, num_cu=256):
    """csrc/gemm.hip: gemm_auto_takes_256 under the default tile rule"""
    t256 = ((N + 255) // 256) * ((M + 255) // 256)
    rounds = (t256 + num_cu - 1) // num_cu
    fills = t256 * 10 >= rounds * num_cu * 9
    wide = N >= 4096 or t256 * 100 >= num_cu * 85
    return N % 256 == 0 and t256 >= 128 and (K >= 2048 or t256 >= 2048 or (wide and fills))


def expected_implicit(conv_implicit, M, N, K):
    """csrc/unet.cpp: conv3x3_run under LDS-DMA staging and the automatic tile rule (the defaults): conv_gemm_kernel runs unless the
    switch is off or the tile rule gives the problem to the 256 x 256 kernels"""
    return bool(conv_implicit) and not auto_takes_256(M, N, K)


def mid_tap(K, S, cin):
    """a slice of the launch begins inside a tap"""
    return S > 1 and (K // S) % cin != 0


def crosses_sample(geo):
    """an M tile of 128 rows holds rows of two samples"""
    hw = geo["Ho"] * geo["Wo"]
    return any((m0 // hw) != ((min(m0 + 127, geo["M"] - 1)) // hw) for m0 in range(0, geo["M"], 128))


def operands(shape):
    """as EB.gemm_operands: x randn in bf16, w randn / sqrt(K) in bf16, bias and the old C randn in fp32, seeded from the shape"""
    geo = geometry(shape)
    nb, H, W, cin, cout, stride, pad = shape[:7]
    g = torch.Generator().manual_seed(((((nb * 31 + H) * 31 + W) * 1031 + cin) * 257 + cout) * 8 + stride * 2 + pad)
    x = torch.randn(nb, H, W, cin, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, 3, 3, cin, generator=g) / geo["K"] ** 0.5).to(torch.bfloat16)
    bias = torch.randn(cout, generator=g)
    c0 = torch.randn(geo["M"], cout, generator=g)
    return dict(geo, x=x, w=w, bias=bias, c0=c0)


def _conv64(x, w, stride, pad):
    """x [nb][H][W][cin], w [cout][3][3][cin] (float64) -> [M][cout]"""
    xn, wn = x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2)
    if pad == 0:
        xn = F.pad(xn, (0, 1, 0, 1))
    y = F.conv2d(xn, wn, stride=stride, padding=1 if pad == 1 else 0)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def conv_lin(ops):
    """lin, t, E in float64 [M][cout]"""
    x, w, b = ops["x"].double(), ops["w"].double(), ops["bias"].double()
    lin = _conv64(x, w, ops["stride"], ops["pad"]) + b
    t = _conv64(x.abs(), w.abs(), ops["stride"], ops["pad"]) + b.abs()
    assert lin.shape == (ops["M"], ops["N"]), "out_hw disagrees with conv2d: %s for M = %d" % (tuple(lin.shape), ops["M"])
    return lin, t, 2.0 * ops["K"] * EB.U32 * t


def ref_bound(ops, epi, lte=None):
    """(reference, bound) of one epilogue, float64 [M][cout]"""
    lin, t, E = lte if lte is not None else conv_lin(ops)
    if epi == 4:
        return lin, E
    c0 = ops["c0"].double()
    return c0 + lin, E + 3 * EB.U32 * (c0.abs() + lin.abs())


def c_buffer(ops, epi, device="cpu"):
    """(flat, C view [M + GUARD_ROWS][ldc], ldc, off): C inside a buffer of NaN bits, G.OFF elements in front, ldc = cout + 4, eight rows
    past M; epilogue 3 finds the old values in [M) x [cout)"""
    M, N = ops["M"], ops["N"]
    ldc = N + LDC_PAD
    flat = torch.empty(G.OFF + (M + GUARD_ROWS) * ldc, dtype=torch.float32, device=device)
    flat.view(torch.int32).fill_(F32_GUARD)
    C = flat[G.OFF:].view(M + GUARD_ROWS, ldc)
    if epi == 3:
        C[:M, :N] = ops["c0"].to(device)
    return flat, C, ldc, G.OFF


def verdict(ops, flat, C, ref, bound):
    """(worst error / bound over [M) x [cout) -- infinite when anything outside it lost its bits --, complaints)"""
    M, N = ops["M"], ops["N"]
    out = []
    r = EB.worst_ratio(C[:M, :N], ref.to(C.device), bound.to(C.device))
    if not r <= 1.0:
        out.append("error / bound %.4g" % r)
    keep = C[:M, :N].clone()
    C[:M, :N].view(torch.int32).fill_(F32_GUARD)
    moved = flat.view(torch.int32) != F32_GUARD
    C[:M, :N] = keep
    if bool(moved.any()):
        first = int(moved.nonzero()[0]) - G.OFF
        out.append("%d elements outside [M) x [cout) were written, the first at row %d column %d" % (
            int(moved.sum()), first // C.shape[1] if first >= 0 else -1, first % C.shape[1] if first >= 0 else first))
        r = float("inf")
    return r, out


# ---- float32 emulation of the launch, and its mutants (tests/test_conv_bounds_cpu.py) --------------------------------------------------------
MUTANTS = ("flat_neighbour", "neighbour_sample", "pad0_as_pad1", "swap_kykx", "c0_dropped", "drop_kstep", "rows_past_m", "bias_per_slice")

# the shapes (indices into SHAPES) at which each mutant computes something else than the kernel, with the reason the others do not
LIVE = {
    # a tap left or right of the image reads flat pixel iy W + ix of its sample: nothing at 1 x 1 (that index is outside the sample),
    # nothing where no window reaches the pad column (index 7)
    "flat_neighbour": (1, 2, 3, 4, 5, 6, 8, 9, 10, 11),
    # a tap above or below the image reads row iy W + ix of the stacked samples: needs a second sample and a window that reaches
    # the top or bottom padding
    "neighbour_sample": (3, 4, 5, 6, 8, 10),
    "pad0_as_pad1": (6, 7),
    # at 1 x 1 only the centre tap is inside the image, and it is its own transpose
    "swap_kykx": (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11),
    # needs a slice that begins inside a tap: S = 4 at cin 256 (slices of 576), S = 5 at cin 320 (576), S = 18 at cin 1024 (512); at cin
    # 512 the nine slices are the nine taps
    "c0_dropped": (8, 9, 11),
    "drop_kstep": tuple(range(len(SHAPES))),
    "rows_past_m": tuple(range(len(SHAPES))),          # no M is a multiple of 128: every last tile has clamped rows
    "bias_per_slice": (8, 9, 10, 11),
}


def gather(ops, mutant=None):
    """the A operand [M][9 cin] in float32, every window gathered by plain indexing"""
    nb, H, W, cin, stride, pad, Ho, Wo = (ops[k] for k in ("nb", "H", "W", "cin", "stride", "pad", "Ho", "Wo"))
    rows = ops["x"].float().reshape(nb * H * W, cin)
    A = torch.zeros(ops["M"], 9 * cin)
    p = 1 if mutant == "pad0_as_pad1" else pad
    for n in range(nb):
        for oy in range(Ho):
            for ox in range(Wo):
                m = (n * Ho + oy) * Wo + ox
                for ky in range(3):
                    for kx in range(3):
                        dy, dx = (kx, ky) if mutant == "swap_kykx" else (ky, kx)
                        iy, ix = oy * stride - p + dy, ox * stride - p + dx
                        row = None
                        if 0 <= iy < H and 0 <= ix < W:
                            row = n * H * W + iy * W + ix
                        elif mutant == "flat_neighbour" and 0 <= iy < H and 0 <= iy * W + ix < H * W:
                            row = n * H * W + iy * W + ix
                        elif mutant == "neighbour_sample" and 0 <= ix < W and 0 <= n * H * W + iy * W + ix < nb * H * W:
                            row = n * H * W + iy * W + ix
                        if row is not None:
                            A[m, (ky * 3 + kx) * cin:(ky * 3 + kx + 1) * cin] = rows[row]
    return A


def emulate(ops, epi, S, mutant=None):
    """(flat, C) as c_buffer lays them out, written as the launch writes them: fp32 products, fp32 accumulation per slice in k-steps of 64,
    the slices added in the order 0 .. S-1, then the bias, and the old value for epilogue 3"""
    M, N, K, cin = ops["M"], ops["N"], ops["K"], ops["cin"]
    A = gather(ops, mutant)
    Wm = ops["w"].float().reshape(N, K)
    Ks = K // S
    assert Ks * S == K and Ks % 64 == 0
    dropped = 4 * cin                                     # the first k-step of the centre tap (always inside the image)
    total = None
    for s in range(S):
        acc = torch.zeros(M, N)
        for t in range(Ks // 64):
            k0 = s * Ks + t * 64
            if mutant == "drop_kstep" and k0 == dropped:
                continue
            a = A[:, k0:k0 + 64]
            if mutant == "c0_dropped":                    # the channel offset from the k-step alone, without the slice's start
                tap = k0 // cin
                a = A[:, tap * cin + (t * 64) % cin:tap * cin + (t * 64) % cin + 64]
            acc = acc + a @ Wm[:, k0:k0 + 64].t()
        if mutant == "bias_per_slice":
            acc = acc + ops["bias"]
        total = acc if total is None else total + acc
    if mutant != "bias_per_slice":
        total = total + ops["bias"]
    flat, C, ldc, off = c_buffer(ops, epi)
    out = C[:M, :N] + total if epi == 3 else total
    C[:M, :N] = out
    if mutant == "rows_past_m":
        C[M:, :N] = out[M - 1]
    return flat, C
