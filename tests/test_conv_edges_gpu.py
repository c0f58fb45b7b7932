"""The texture stage's 3 x 3 convolution and its 2 x upsampling, element by element, through r3g_op_conv3x3 and r3g_op_upsample2x alone.

Convolution: every shape of tests/conv_bounds.py (what each is for stands there) x epilogues 4 and 3 x "conv_implicit" 1 and 0, the
cin = 256 shape once more without a workspace.  Per launch:
  * the ELEMENT-WISE bound of conv_bounds against torch's float64 conv2d on NCHW tensors at every element of C (derived there;
    tests/test_conv_bounds_cpu.py shows that a float32 emulation of the launch meets it and that eight mutants do not);
  * C sits in a buffer of NaN bits, G.OFF elements in front, ldc = cout + 4, eight rows past M: everything outside [M) x [cout) keeps
    its bits, an element that was never stored is a NaN;
  * x, w and bias sit in buffers of NaN bits (x with W + 2 pixels of them in front and behind, w with eight rows behind row cout): a
    read before the first sample, past the last one or past row cout of w poisons C;
  * d_col and d_ws sit in guarded buffers: nothing past M * 9 cin elements of d_col, nothing past S * M * cout floats of d_ws is written,
    and a launch that does not use one of them leaves all of it alone;
  * *implicit and the "gemm_conv_implicit" counter agree with the restated dispatch, *slices and the "gemm_splitk128" counter with the
    restated slice rule: a launch that fell back cannot pass for the path it was asked for;
  * the implicit and the im2col output of one shape and epilogue are equal bit for bit (the promise of tests/switch_table.py).
The closing test asserts reach from the launches that met all of this.  Every contract violation of include/r3g.h is refused with
R3G_ERR_INVALID and nothing written.

Upsampling: bit equality with x[oy >> 1][ox >> 1].to(torch.bfloat16) in guarded buffers; the inputs hold exact round-to-even ties in
both directions, +-0, values whose rounding carries into the exponent and values just under the bf16 maximum.  Subnormal float32 inputs
are left out: nobody has checked the conversion's denormal mode on this hardware.

A HIP error ends the session (pytest.exit): nothing more is started on a device that has faulted.  The largest launch is two tiles of
128 x 128 over 45 k-steps; the file takes a few seconds on an MI355X.
"""
import ctypes

import pytest

import conv_bounds as CB
import row_guard as G
from parity_support import report
from switch_table import switched

pytestmark = pytest.mark.gpu

COUNTERS = ("gemm_conv_implicit", "gemm_splitk128")
_PREPARED, _RESULTS = {}, {}


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    return torch, ffi.lib(), ffi, ffi.context(0)


def _guarded_copy(torch, t, front, behind):
    """(flat buffer of NaN bits holding t's elements from element `front` on, with `behind` more elements after them)"""
    flat = G.guarded(torch, t.dtype, front + t.numel() + behind)
    flat[front:front + t.numel()] = t.reshape(-1).cuda()
    return flat


def prepared(torch, i):
    """operands of shape i on the device inside their guards, the float64 references and bounds (computed once, on the CPU); memoised"""
    if i not in _PREPARED:
        ops = CB.operands(CB.SHAPES[i])
        lte = CB.conv_lin(ops)
        xoff = (ops["W"] + 2) * ops["cin"]                     # a multiple of 64 elements: the rows stay 16-byte aligned
        _PREPARED[i] = dict(
            ops=ops, rb={epi: tuple(t.cuda() for t in CB.ref_bound(ops, epi, lte)) for epi in CB.EPILOGUES},
            x=_guarded_copy(torch, ops["x"], xoff, xoff), xoff=xoff,
            w=_guarded_copy(torch, ops["w"], G.OFF, 8 * ops["K"]), bias=_guarded_copy(torch, ops["bias"], G.OFF, 8))
    return _PREPARED[i]


def conv_call(L, ctx, stream, a):
    return lambda: L.r3g_op_conv3x3(a["ctx"], a["x"], a["nb"], a["H"], a["W"], a["cin"], a["stride"], a["pad"], a["w"], a["cout"], a["bias"],
                                    a["c"], a["ldc"], a["epi"], a["col"], a["col_elems"], a["ws"], a["ws_elems"], a["implicit"], a["slices"], stream)


def conv_args(ctx, pr, epi, c_ptr, ldc, col, col_elems, ws, ws_elems, implicit=None, slices=None):
    ops = pr["ops"]
    return dict(ctx=ctx, x=G.ptr(pr["x"], pr["xoff"]), nb=ops["nb"], H=ops["H"], W=ops["W"], cin=ops["cin"], stride=ops["stride"], pad=ops["pad"],
                w=G.ptr(pr["w"], G.OFF), cout=ops["cout"], bias=G.ptr(pr["bias"], G.OFF), c=c_ptr, ldc=ldc, epi=epi,
                col=G.ptr(col, G.OFF), col_elems=col_elems, ws=G.ptr(ws, G.OFF), ws_elems=ws_elems,
                implicit=None if implicit is None else ctypes.byref(implicit), slices=None if slices is None else ctypes.byref(slices))


def one_launch(env, res, i, epi, want_implicit, workspace, tag):
    """launch, out-parameters, counters, guards, verdict; records into res"""
    torch, L, ffi, ctx = env
    pr = prepared(torch, i)
    ops = pr["ops"]
    M, N, K = ops["M"], ops["N"], ops["K"]
    ref, bound = pr["rb"][epi]
    S_rule = CB.splitk128_factor(M, N, K)
    ws_elems = S_rule * M * N if workspace else 0
    S = CB.expected_slices(M, N, K, ws_elems)
    flat, C, ldc, off = CB.c_buffer(ops, epi, "cuda")
    col = G.guarded(torch, torch.bfloat16, G.OFF + M * K + 8 * K)
    ws = G.guarded(torch, torch.float32, G.OFF + ws_elems + 8 * N) if workspace else None
    implicit, slices = ctypes.c_int(-1), ctypes.c_int(-1)
    c0 = {c: ffi.counter(c) for c in COUNTERS}
    G.run(torch, ffi, conv_call(L, ctx, G.stream(torch), conv_args(ctx, pr, epi, G.ptr(flat, off), ldc, col, M * K, ws, ws_elems, implicit, slices)), tag)
    res["launches"] += 1
    moved = {c: ffi.counter(c) - c0[c] for c in COUNTERS}
    complaints = []
    if implicit.value != int(want_implicit) or moved["gemm_conv_implicit"] != int(want_implicit):
        complaints.append("*implicit %d, gemm_conv_implicit moved by %d: the restated dispatch says %d" % (
            implicit.value, moved["gemm_conv_implicit"], int(want_implicit)))
    if slices.value != S or moved["gemm_splitk128"] != int(S > 1):
        complaints.append("*slices %d, gemm_splitk128 moved by %d: the restated rule says %d slices" % (slices.value, moved["gemm_splitk128"], S))
    r, found = CB.verdict(ops, flat, C, ref, bound)
    complaints += found
    ar = lambda n: torch.arange(n, device="cuda")
    n_col, first = G.untouched(torch, col, G.OFF + ar(0 if want_implicit else M * K))
    if n_col:
        complaints.append("%d elements of d_col outside its %s were written, the first at %d" % (
            n_col, "M * 9 cin elements" if not want_implicit else "(unused) whole", first - G.OFF))
    if ws is not None:
        n_ws, first = G.untouched(torch, ws, G.OFF + ar(S * M * N if S > 1 else 0))
        if n_ws:
            complaints.append("%d floats of d_ws outside its %d x M x cout were written, the first at %d" % (n_ws, S if S > 1 else 0, first - G.OFF))
    name = "%s %s epilogue %d" % ("implicit" if want_implicit else "im2col", "split" if S > 1 else "one launch", epi)
    res["worst"][name] = max(res["worst"].get(name, 0.0), r)
    res["out"][(i, epi, workspace)] = C[:M, :N].clone()
    if complaints:
        res["failures"] += ["%s: %s" % (tag, c) for c in complaints]
    else:
        res["reached"].add((i, bool(implicit.value), S))


def run_config(env, conv_implicit):
    """every shape x epilogue under one setting of "conv_implicit"; memoised (the bit comparison and the closing test read both)"""
    if conv_implicit in _RESULTS:
        return _RESULTS[conv_implicit]
    torch, L, ffi, ctx = env
    res = dict(worst={}, reached=set(), failures=[], launches=0, out={})
    with switched(L, ffi, conv_implicit=conv_implicit):
        for i, shape in enumerate(CB.SHAPES):
            geo = CB.geometry(shape)
            want = CB.expected_implicit(conv_implicit, geo["M"], geo["N"], geo["K"])
            for workspace in ((True, False) if i == CB.NO_WORKSPACE else (True,)):
                for epi in CB.EPILOGUES:
                    tag = "%s epilogue %d conv_implicit %d%s" % (shape[:7], epi, conv_implicit, "" if workspace else " no workspace")
                    one_launch(env, res, i, epi, want, workspace, tag)
    for name, r in sorted(res["worst"].items()):
        report("conv edges: %s (error / bound)" % name, r, 1.0)
    _RESULTS[conv_implicit] = res
    return res


@pytest.mark.parametrize("conv_implicit", [1, 0], ids=["implicit", "im2col"])
def test_conv3x3_edges(env, conv_implicit):
    res = run_config(env, conv_implicit)
    print("conv_implicit %d: %d launches, worst error / bound %s" % (conv_implicit, res["launches"], {k: round(v, 6) for k, v in sorted(res["worst"].items())}))
    assert not res["failures"], "%d findings, the first: %s" % (len(res["failures"]), "\n".join(res["failures"][:12]))


def test_implicit_and_im2col_outputs_are_equal_bit_for_bit(env):
    torch = env[0]
    a, b = run_config(env, 1)["out"], run_config(env, 0)["out"]
    assert sorted(a) == sorted(b) and len(a) == 2 * (len(CB.SHAPES) + 1)
    differ = [(CB.SHAPES[i][:7], epi, ws, int((G.bits(torch, a[(i, epi, ws)]) != G.bits(torch, b[(i, epi, ws)])).sum())) for i, epi, ws in sorted(a)
              if not torch.equal(G.bits(torch, a[(i, epi, ws)]), G.bits(torch, b[(i, epi, ws)]))]
    assert not differ, "(shape, epilogue, workspace, elements that differ): %s" % differ


def test_every_convolution_regime_was_reached(env):
    """Reads what the launches above recorded (a launch counts when it met its bound, kept every guard and reported the path and the
    slices the restated rules give).  A configuration that has not run yet in this session (the test selected alone) is run here."""
    reached = run_config(env, 1)["reached"] | run_config(env, 0)["reached"]
    geo = {i: CB.geometry(s) for i, s in enumerate(CB.SHAPES)}
    missing = []
    for path in (True, False):
        mine = [(i, S) for i, imp, S in reached if imp == path]
        what = "implicit" if path else "im2col"
        if {S for _, S in mine} != {1, 4, 5, 9, 18}:
            missing.append("%s: S took the values %s" % (what, sorted({S for _, S in mine})))
        if not any(CB.mid_tap(geo[i]["K"], S, geo[i]["cin"]) for i, S in mine):
            missing.append("%s: no slice that begins inside a tap" % what)
        if not any(S > 1 and not CB.mid_tap(geo[i]["K"], S, geo[i]["cin"]) for i, S in mine):
            missing.append("%s: no split with tap-aligned slices" % what)
        for pad in (0, 1):
            if not any(geo[i]["stride"] == 2 and geo[i]["pad"] == pad for i, _ in mine):
                missing.append("%s: stride 2 never ran with pad %d" % (what, pad))
        if not any(CB.crosses_sample(geo[i]) for i, _ in mine):
            missing.append("%s: no M tile that crosses a sample boundary" % what)
        if not any(geo[i]["N"] % 128 for i, _ in mine):
            missing.append("%s: no N tail" % what)
        if not any(geo[i]["M"] > 128 and geo[i]["M"] % 128 for i, _ in mine):
            missing.append("%s: no second M tile with a tail" % what)
    assert not missing, "\n".join(missing)


def test_a_workspace_one_float_short_is_left_alone(env):
    """the cin = 256 shape with room for S * M * cout - 1 floats: one launch over all of k, *slices 1, not one float of d_ws written"""
    torch, L, ffi, ctx = env
    pr = prepared(torch, CB.NO_WORKSPACE)
    ops = pr["ops"]
    M, N, K = ops["M"], ops["N"], ops["K"]
    ws_elems = CB.splitk128_factor(M, N, K) * M * N - 1
    assert CB.splitk128_factor(M, N, K) > 1 and CB.expected_slices(M, N, K, ws_elems) == 1
    flat, C, ldc, off = CB.c_buffer(ops, 4, "cuda")
    ws = G.guarded(torch, torch.float32, G.OFF + ws_elems + 8 * N)
    slices = ctypes.c_int(-1)
    before = ffi.counter("gemm_splitk128")
    G.run(torch, ffi, conv_call(L, ctx, G.stream(torch), conv_args(ctx, pr, 4, G.ptr(flat, off), ldc, None, 0, ws, ws_elems, None, slices)),
          "conv3x3, a workspace one float short")
    r, found = CB.verdict(ops, flat, C, *pr["rb"][4])
    assert not found, found
    assert slices.value == 1 and ffi.counter("gemm_splitk128") == before
    assert G.untouched(torch, ws, G.OFF + torch.arange(0, device="cuda"))[0] == 0
    both = run_config(env, 1)["out"]
    assert torch.equal(G.bits(torch, C[:M, :N].contiguous()), G.bits(torch, both[(CB.NO_WORKSPACE, 4, False)])), "not the bits of the launch without a workspace"


def test_conv3x3_refusals(env):
    """every violation of the contract of include/r3g.h, one at a time: R3G_ERR_INVALID, C, d_col and d_ws keep every bit, no counter moves"""
    torch, L, ffi, ctx = env
    pr = prepared(torch, 2)
    ops = pr["ops"]
    M, N, K = ops["M"], ops["N"], ops["K"]
    flat, C, ldc, off = CB.c_buffer(ops, 4, "cuda")
    col = G.guarded(torch, torch.bfloat16, G.OFF + M * K + 8 * K)
    ws = G.guarded(torch, torch.float32, G.OFF + M * N + 8 * N)
    base = conv_args(ctx, pr, 4, G.ptr(flat, off), ldc, col, M * K, ws, M * N)
    bad = {
        "ctx null": dict(ctx=None), "x null": dict(x=None), "w null": dict(w=None), "c null": dict(c=None),
        "nb 0": dict(nb=0), "height 0": dict(H=0), "width 0": dict(W=0), "nb -1": dict(nb=-1),
        "height + pad < 2": dict(H=1, pad=0), "width + pad < 2": dict(W=1, pad=0),
        "cin % 64": dict(cin=96), "cin 32": dict(cin=32), "cin 0": dict(cin=0), "cout % 4": dict(cout=66), "cout 0": dict(cout=0),
        "ldc % 4": dict(ldc=N + 2), "ldc < cout": dict(ldc=N - 4),
        "x 8 bytes off": dict(x=G.ptr(pr["x"], pr["xoff"] + 4)), "w 8 bytes off": dict(w=G.ptr(pr["w"], G.OFF + 4)),
        "c 8 bytes off": dict(c=G.ptr(flat, off + 2)), "bias 8 bytes off": dict(bias=G.ptr(pr["bias"], G.OFF + 2)),
        "col 8 bytes off": dict(col=G.ptr(col, G.OFF + 4)), "ws 8 bytes off": dict(ws=G.ptr(ws, G.OFF + 2)),
        "epilogue 0": dict(epi=0), "epilogue 5": dict(epi=5), "epilogue 6": dict(epi=6),
        "stride 0": dict(stride=0), "stride 3": dict(stride=3), "pad 2": dict(pad=2), "pad -1": dict(pad=-1),
    }
    before = {c: ffi.counter(c) for c in COUNTERS}
    for what, over in bad.items():
        G.refused(torch, L, conv_call(L, ctx, G.stream(torch), dict(base, **over)), (flat, col, ws), "conv3x3, " + what)
    with switched(L, ffi, conv_implicit=0):
        for what, over in {"im2col needed, d_col null": dict(col=None), "im2col needed, d_col one element short": dict(col_elems=M * K - 1),
                           "im2col needed, col_elems 0": dict(col_elems=0)}.items():
            G.refused(torch, L, conv_call(L, ctx, G.stream(torch), dict(base, **over)), (flat, col, ws), "conv3x3, " + what)
    assert {c: ffi.counter(c) for c in COUNTERS} == before
    # the admitted call, and the implicit launch without the matrix it does not need
    G.run(torch, ffi, conv_call(L, ctx, G.stream(torch), dict(base, col=None, col_elems=0, ws=None, ws_elems=0, bias=None)), "conv3x3, an admitted call")
    ref, bound = pr["rb"][4]
    r = CB.EB.worst_ratio(C[:M, :N], ref - ops["bias"].double().cuda(), bound)
    assert r <= 1.0 and ffi.counter("gemm_conv_implicit") == before["gemm_conv_implicit"] + 1, r


# ---- upsample2x ---------------------------------------------------------------------------------------------------------------------------
UPSAMPLE_SHAPES = ((1, 1, 4), (3, 5, 68), (5, 7, 320))
# float32 bit patterns: round-to-even ties down and up (both signs), +-0, roundings that carry into the exponent (one of them a tie),
# values at and just under the bf16 maximum 0x7F7F0000 (0x7F7F8000, half a step above it, would round to infinity and is left out)
SPECIAL_BITS = (0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x3FFFFFFF, 0x3FFF8000, 0xBFFFC000, 0x407F8001,
                0x7F7F0000, 0x7F7F7FFF, 0x7F7E8000, 0x7F7E8001, 0xFF7F7FFF, 0xFF7E8000)


def upsample_input(torch, H, W, c):
    """randn with the special values scattered over it, 37 elements apart (all sixteen at the two larger shapes; the four-element shape
    holds the four ties)"""
    g = torch.Generator().manual_seed(10007 * H + 101 * W + c)
    x = torch.randn(H * W * c, generator=g)
    sp = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in SPECIAL_BITS], dtype=torch.int64).to(torch.int32).view(torch.float32)
    n = min(len(sp), x.numel())
    pos = (torch.arange(n) * 37 + 1) % x.numel()
    assert len(set(pos.tolist())) == n
    x[pos] = sp[:n]
    return x.view(H, W, c)


def bf16_bits_rne(torch, x):
    """round to nearest even on the integer view (finite inputs): the restatement beside torch's own conversion"""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF


def test_upsample2x_is_the_bf16_of_its_source_pixel(env):
    torch, L, ffi, ctx = env
    failures = []
    for draw, (H, W, c) in enumerate(UPSAMPLE_SHAPES):
        x = upsample_input(torch, H, W, c)
        want = x.to(torch.bfloat16)
        assert torch.equal(want.view(torch.int16).to(torch.int64) & 0xFFFF, bf16_bits_rne(torch, x))
        assert bool(torch.isfinite(want.float()).all()) and bool((x.abs() >= 2.0 ** -126)[x != 0].all())
        want = want[torch.arange(2 * H) >> 1][:, torch.arange(2 * W) >> 1].contiguous()
        xin = _guarded_copy(torch, x, G.OFF, 2 * c)
        y = G.guarded(torch, torch.bfloat16, G.OFF + 4 * H * W * c + 2 * c)
        tag = "upsample2x %d x %d x %d" % (H, W, c)
        G.run(torch, ffi, lambda: L.r3g_op_upsample2x(G.ptr(xin, G.OFF), H, W, c, G.ptr(y, G.OFF), G.stream(torch)), tag)
        owned = G.OFF + torch.arange(4 * H * W * c, device="cuda")
        got = G.bits(torch, y[owned]).cpu()
        n, first = G.untouched(torch, y, owned)
        if n:
            failures.append("%s: %d elements outside [2H][2W][c] were written, the first at %d" % (tag, n, first - G.OFF))
        if not torch.equal(got, want.view(torch.int16).reshape(-1)):
            bad = (got != want.view(torch.int16).reshape(-1)).nonzero().reshape(-1)
            j = int(bad[0])
            failures.append("%s: %d elements differ, the first at %d: 0x%04X for 0x%04X" % (
                tag, bad.numel(), j, int(got[j]) & 0xFFFF, int(want.view(torch.int16).reshape(-1)[j]) & 0xFFFF))
    assert not failures, "\n".join(failures)


def test_upsample2x_refusals(env):
    torch, L, ffi, ctx = env
    H, W, c = 3, 5, 68
    xin = _guarded_copy(torch, upsample_input(torch, H, W, c), G.OFF, 2 * c)
    y = G.guarded(torch, torch.bfloat16, G.OFF + 4 * H * W * c + 2 * c)
    base = dict(x=G.ptr(xin, G.OFF), H=H, W=W, c=c, y=G.ptr(y, G.OFF))
    call = lambda a: (lambda: L.r3g_op_upsample2x(a["x"], a["H"], a["W"], a["c"], a["y"], G.stream(torch)))
    bad = {"c % 4": dict(c=66), "c 0": dict(c=0), "height 0": dict(H=0), "width 0": dict(W=0), "height -1": dict(H=-1), "x null": dict(x=None),
           "y null": dict(y=None), "x 8 bytes off": dict(x=G.ptr(xin, G.OFF + 2)), "y 4 bytes off": dict(y=G.ptr(y, G.OFF + 2))}
    for what, over in bad.items():
        G.refused(torch, L, call(dict(base, **over)), (y,), "upsample2x, " + what)
    G.run(torch, ffi, call(base), "upsample2x, an admitted call")
