"""The FP8 path -- quant_fp8_rows_kernel, gemm8f_kernel with every epilogue it is offered, the e4m3-output epilogue -- at the shapes where
its edge logic is live, through r3g_op_quant_fp8, r3g_op_gemm_fp8 and r3g_op_gemm_fp8_e4m3 alone.

Per GEMM launch (8 shapes x 2 operand sets x epilogues 0, 1, 2, 3, 6, 7 x 2 layouts of C, under "gemm_wide_epilogue" 1 and 0, the GELU
epilogues under "gelu_pk" 1 and 0):
  * the ELEMENT-WISE bound of tests/fp8_bounds.py at every element of C, or bit equality for the exact operand set (derived there;
    tests/test_fp8_bounds_cpu.py shows that a float32 emulation of the kernel meets both and that eight mutants do not);
  * C sits in a buffer of NaN bits (0x7F for the e4m3 output) -- "loose": four elements in front, ldc = N + 4; "wide": 16-byte aligned,
    ldc = N + 8 (e4m3: N + 16 bytes) -- with eight rows past M: everything outside [M) x [N) keeps its bits, an unstored element is a NaN;
  * the operands sit at lda = K + 16, ldw = K + 32 with eight rows past M / N; the pad bytes and those rows hold the e4m3 NaN code 0x7F,
    the scale, bias and gate vectors end in eight float NaNs: any read past K, M or N poisons the output;
  * "gemm_fp8" moves by exactly one and no other GEMM counter moves.
The closing test asserts from the recorded launches that every epilogue was reached with an M tail, both kinds of N tail, nk = 2 and
nk > 2, and both store paths.  The quantiser is held against the bit-exact restatement of fp8_bounds.quant_ref in guarded outputs; the
row with amax = 2^-130 goes through r3g_op_layernorm's e4m3 form as well.  Every contract violation of include/r3g.h is refused with
R3G_ERR_INVALID, nothing written and no counter moved (the 32-bit staging-offset limit is not tried here: a broken check there would
launch out of bounds).  The geo decoder under "geo_fp8" moves "gemm_fp8" by the number of fp8 GEMMs each mode implies, and not at all
at a width that fails W % 256 == 0 (the silent fallback to the bf16 kernels).
A HIP error ends the session (pytest.exit): nothing more is started on a device that has faulted, and nothing retries.  Every launch is
at most six 256 x 256 tiles; the file takes a few seconds on an MI355X.
"""
import pytest

import edge_bounds as EB
import fp8_bounds as FB
import row_bounds as RB
import row_guard as G
from parity_support import report
from switch_table import switched

pytestmark = pytest.mark.gpu

COUNTERS = EB.GEMM_COUNTERS + ("gemm_register_staged", "gemm_mixed", "gemm_splitk128", "gemm_conv_implicit", "gemm_fp8")
_PREPARED, _RESULTS = {}, {}


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    ffi.context(0)
    return torch, ffi.lib(), ffi


def _poisoned_rows(torch, codes, ld):
    """(flat uint8 buffer of 0x7F with the rows of `codes` at stride ld, eight more rows behind them)"""
    rows, K = codes.shape
    flat = torch.full(((rows + FB.GUARD_ROWS) * ld,), FB.NAN_CODE, device="cuda", dtype=torch.uint8)
    flat.view(rows + FB.GUARD_ROWS, ld)[:rows, :K] = codes
    return flat


def _poisoned_vec(torch, v):
    out = torch.full((v.numel() + 8,), float("nan"), device="cuda", dtype=torch.float32)
    out[:v.numel()] = v
    return out


def prepared(torch, M, N, K, kind):
    """operands of one shape on the device in their poisoned buffers, the references and bounds of every epilogue; memoised"""
    key = (M, N, K, kind)
    if key not in _PREPARED:
        ops = FB.gemm_operands(M, N, K, kind, "cuda")
        lte = FB.gemm_lin(ops)
        _PREPARED[key] = dict(
            ops=ops, rb={epi: FB.gemm_ref_bound(ops, epi, lte) for epi in FB.GEMM_EPILOGUES},
            a=_poisoned_rows(torch, ops["a8"], K + FB.LDA_PAD), w=_poisoned_rows(torch, ops["w8"], K + FB.LDW_PAD),
            sa=_poisoned_vec(torch, ops["sa"]), sw=_poisoned_vec(torch, ops["sw"]), bias=_poisoned_vec(torch, ops["bias"]),
            gate=_poisoned_vec(torch, ops["gate"]))
    return _PREPARED[key]


def gemm_args(pr, epi, c_ptr, ldc):
    """the admitted arguments of one launch, by name"""
    ops = pr["ops"]
    return dict(a=pr["a"].data_ptr(), lda=ops["K"] + FB.LDA_PAD, sa=pr["sa"].data_ptr(), w=pr["w"].data_ptr(), ldw=ops["K"] + FB.LDW_PAD,
                sw=pr["sw"].data_ptr(), bias=pr["bias"].data_ptr(), gate=pr["gate"].data_ptr() if epi in (3, 6) else None, c=c_ptr, ldc=ldc,
                m=ops["M"], n=ops["N"], k=ops["K"])


def one_launch(env, res, M, N, K, kind, epi, layout, wide, pk, tag):
    """launch, counters, verdict; records into res"""
    torch, L, ffi = env
    pr = prepared(torch, M, N, K, kind)
    ops = pr["ops"]
    ref, bound = pr["rb"][epi]
    flat, C, ldc, off = FB.c_buffer(ops, epi, layout, "cuda")
    c0 = {c: ffi.counter(c) for c in COUNTERS}
    G.run(torch, ffi, FB.gemm_abi_call(L, "e4m3" if epi == 7 else epi, G.stream(torch), gemm_args(pr, epi, C.data_ptr(), ldc)), tag)
    res["launches"] += 1
    moved = {c: ffi.counter(c) - c0[c] for c in COUNTERS if ffi.counter(c) != c0[c]}
    complaints = []
    if moved != {"gemm_fp8": 1}:
        complaints.append("launch counters moved %s, expected gemm_fp8 alone by 1" % moved)
    r, found = FB.verdict(ops, epi, flat, C, off, ref, bound)
    complaints += found
    name = "%s epilogue %d" % (kind, epi)
    res["worst"][name] = max(res["worst"].get(name, 0.0), r)
    if complaints:
        res["failures"] += ["%s: %s" % (tag, c) for c in complaints]
    else:
        res["reached"].add((epi, M, N, K, FB.store_path(epi, N, layout, wide)))


def run_config(env, wide):
    """every shape x operand set x epilogue x layout under one setting of "gemm_wide_epilogue"; memoised (the closing test reads both)"""
    if wide in _RESULTS:
        return _RESULTS[wide]
    torch, L, ffi = env
    res = dict(worst={}, reached=set(), failures=[], launches=0)
    with switched(L, ffi, gemm_wide_epilogue=wide):
        for M, N, K, _ in FB.GEMM_SHAPES:
            for kind in FB.KINDS:
                for epi in FB.GEMM_EPILOGUES:
                    for pk in ((1, 0) if epi in (1, 2) else (1,)):
                        for layout in FB.LAYOUTS:
                            tag = "%s %s epilogue %d gelu_pk %d %s wide %d" % ((M, N, K), kind, epi, pk, layout, wide)
                            with switched(L, ffi, gelu_pk=pk):
                                one_launch(env, res, M, N, K, kind, epi, layout, wide, pk, tag)
    for name, r in sorted(res["worst"].items()):
        report("fp8 gemm edges wide=%d %s (error / bound)" % (wide, name), r, 1.0)
    _RESULTS[wide] = res
    return res


@pytest.mark.parametrize("wide", [1, 0], ids=["wide", "narrow"])
def test_fp8_gemm_edges(env, wide):
    res = run_config(env, wide)
    print("gemm_wide_epilogue %d: %d launches, worst error / bound %s" % (wide, res["launches"], {k: round(v, 6) for k, v in sorted(res["worst"].items())}))
    assert not res["failures"], "%d findings, the first: %s" % (len(res["failures"]), "\n".join(res["failures"][:12]))


@pytest.mark.parametrize("raster", [0, 1])
def test_fp8_gemm_raster_groups(env, raster):
    """(129, 1284, 256) -- six tile columns -- with one raster group over all columns (0) and one group per column (1); the default (groups
    of four, a ragged last group) is what test_fp8_gemm_edges runs"""
    torch, L, ffi = env
    res = dict(worst={}, reached=set(), failures=[], launches=0)
    M, N, K = 129, 1284, 256
    with switched(L, ffi, gemm_raster=raster):
        for kind in FB.KINDS:
            for epi in (3, 7):
                one_launch(env, res, M, N, K, kind, epi, "wide", 1, 1, "%s %s epilogue %d gemm_raster %d" % ((M, N, K), kind, epi, raster))
    for name, r in sorted(res["worst"].items()):
        report("fp8 gemm edges gemm_raster=%d %s (error / bound)" % (raster, name), r, 1.0)
    assert not res["failures"], "\n".join(res["failures"][:12])


def test_every_fp8_epilogue_was_reached_at_every_edge(env):
    """Reads what the launches above recorded (a launch counts when it met its bound, kept the guards and moved gemm_fp8 alone).  A
    configuration that has not run yet in this session (the test selected alone) is run here."""
    reached = set()
    for wide in (1, 0):
        reached |= run_config(env, wide)["reached"]
    assert FB.gemm_coverage(reached) == []


# ---- the quantiser --------------------------------------------------------------------------------------------------------------------
BIG_BF16_BITS = 0x7F00          # 2^127: a finite value that takes over a row's maximum if a read strays past K


def _quant_run(env, x, ldx, ldq, tag):
    """x bf16 [rows][K] (CPU) through r3g_op_quant_fp8 at the given strides in guarded buffers: (codes [rows][K], scales [rows]) on the CPU"""
    torch, L, ffi = env
    rows, K = x.shape
    ar = lambda n: torch.arange(n, device="cuda")
    xi = (G.OFF + ar(rows) * ldx)[:, None] + ar(K)[None]
    qi = (G.OFF + ar(rows) * ldq)[:, None] + ar(K)[None]
    si = 4 + ar(rows)
    xbuf = torch.empty(G.OFF + (rows + 2) * ldx, device="cuda", dtype=torch.bfloat16)
    G.bits(torch, xbuf).fill_(BIG_BF16_BITS)
    G.place(torch, xbuf, xi, x.cuda())
    q = G.guarded(torch, torch.uint8, G.OFF + (rows + 2) * ldq)
    sc = G.guarded(torch, torch.float32, rows + 8)
    G.run(torch, ffi, lambda: L.r3g_op_quant_fp8(G.ptr(xbuf, G.OFF), ldx, rows, K, G.ptr(q, G.OFF), ldq, G.ptr(sc, 4), G.stream(torch)), tag)
    assert G.untouched(torch, q, qi)[0] == 0, "%s: codes outside [rows) x [K) were written" % tag
    assert G.untouched(torch, sc, si)[0] == 0, "%s: scales outside [rows) were written" % tag
    return q[qi].cpu(), sc[si].cpu()


def test_quantiser_is_the_restatement_bit_for_bit(env):
    torch, L, ffi = env
    failures = []
    for rows in FB.QUANT_ROWS:
        for K in FB.QUANT_K:
            case = FB.quant_case(rows, K)
            want_q, want_sc = FB.quant_ref(case["x"])
            tag = "quant_fp8 rows %d k %d %s" % (rows, K, case["kinds"])
            q, sc = _quant_run(env, case["x"], K + FB.QUANT_PAD, K + FB.QUANT_PAD, tag)
            if not torch.equal(G.bits(torch, sc), G.bits(torch, want_sc)):
                failures.append("%s: scales %s, expected %s" % (tag, sc.tolist(), want_sc.tolist()))
            if not torch.equal(q, want_q):
                bad = (q != want_q).nonzero()
                r, c = int(bad[0][0]), int(bad[0][1])
                failures.append("%s: %d codes differ, the first at (%d, %d): 0x%02X for 0x%02X (x = %r)" % (
                    tag, bad.shape[0], r, c, int(q[r, c]), int(want_q[r, c]), float(case["x"][r, c])))
            if bool(((q & 127) == 127).any()):
                failures.append("%s: a finite row produced a NaN code" % tag)
    assert not failures, "\n".join(failures[:12])


def test_quantiser_nonfinite_elements_as_the_header_states(env):
    """a NaN element: its own code is the NaN code, the rest of the row as if it were absent; a +-Inf element: the scale +Inf, its own
    code the NaN code, every finite element a zero code (pinned, not designed: include/r3g.h)"""
    torch, L, ffi = env
    x = FB.quant_nonfinite_case()
    want_q, want_sc = FB.quant_ref(x)
    q, sc = _quant_run(env, x, 16, 16, "quant_fp8 with non-finite elements")
    assert torch.equal(G.bits(torch, sc), G.bits(torch, want_sc)), (sc.tolist(), want_sc.tolist())
    nan_code = (want_q & 127) == 127
    assert int(nan_code.sum()) == 3 and bool(((q & 127) == 127)[nan_code].all())
    assert torch.equal(q[~nan_code], want_q[~nan_code])


def test_layernorm_e4m3_row_with_a_tiny_maximum(env):
    """LayerNorm weights of 2^-130 (and zeros) put every finished row at amax ~ 2^-129: the scale is the floor 2^-126, no code is a NaN, the
    zero columns are zero codes and every code is the e4m3 nearest to the finished value over the stored scale"""
    torch, L, ffi = env
    C, rows = 256, 5
    case = dict(RB.ln_case(C, 0, RB.LN_ROWCFGS[1], "none", "cuda"))
    sign = 1.0 - 2.0 * (torch.arange(C, device="cuda") % 2)
    w = (sign * 2.0 ** -130).float()
    w[::4] = 0.0
    case["w"] = w
    assert float(w.abs().max()) == 2.0 ** -130
    ld8 = C + 8
    i8 = (G.OFF + torch.arange(rows, device="cuda") * ld8)[:, None] + torch.arange(C, device="cuda")[None]
    isc = 4 + torch.arange(rows, device="cuda")
    for rpw in (1, 4):
        y8 = G.guarded(torch, torch.uint8, G.OFF + (rows + 2) * ld8)
        ysc = G.guarded(torch, torch.float32, rows + 8)
        x = case["x"].contiguous()
        with switched(L, ffi, ln_rows=rpw):
            G.run(torch, ffi, lambda: L.r3g_op_layernorm(x.data_ptr(), 0, C, 0, None, 0, 0, G.ptr(y8, G.OFF), ld8, G.ptr(ysc, 4), w.data_ptr(), None,
                                                         None, None, 0, 0, 0, None, None, rows, C, rows, case["eps"], G.stream(torch)),
                  "layernorm e4m3, tiny weights, ln_rows %d" % rpw)
        codes, qs = y8[i8], ysc[isc].double()
        assert G.untouched(torch, y8, i8)[0] == 0 and G.untouched(torch, ysc, isc)[0] == 0
        assert bool(((codes & 127) != 127).all()), "a finite row produced a NaN code"
        assert bool(((codes[:, ::4] & 127) == 0).all())
        ref, e = RB.ln_ref_err(case)
        live = ref.abs().amax(-1) > 0                          # (row 3 is constant: its finished values are zeros, its scale 1)
        assert bool((qs[live] == FB.FLOOR).all()) and bool(((qs == FB.FLOOR) | (qs == 1.0)).all()), qs.tolist()
        e = e + 2.0 ** -149                                    # the product with a subnormal weight rounds to a multiple of 2^-149
        t = ref / qs[:, None]
        e_t = e / qs[:, None] + RB.g(2) * (t.abs() + e / qs[:, None])
        r = RB.worst_ratio(RB.e4m3_decode(codes), t, RB.e4m3_half_ulp((t.abs() + e_t).clamp_max(448.0)) + e_t)
        report("fp8 edges: layernorm e4m3 codes under the floored scale, ln_rows %d (error / bound)" % rpw, r, 1.0)
        assert r <= 1.0, r


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_fp8_gemm_refusals(env):
    """every violation of the contract of include/r3g.h returns R3G_ERR_INVALID with the guarded C untouched and gemm_fp8 unmoved; m == 0
    and n == 0 return R3G_OK with nothing launched"""
    torch, L, ffi = env
    M, N, K = 17, 68, 256
    pr = prepared(torch, M, N, K, "random")
    ops = pr["ops"]
    before = ffi.counter("gemm_fp8")
    for epi, esz in FB.REFUSED_ENTRIES:
        flat, C, ldc, off = FB.c_buffer(ops, 7 if epi == "e4m3" else epi, "loose", "cuda")
        args = gemm_args(pr, epi, C.data_ptr(), ldc)
        for what, over in FB.gemm_refusals(epi, esz, args, N, K).items():
            G.refused(torch, L, FB.gemm_abi_call(L, epi, G.stream(torch), dict(args, **over)), (flat,), "gemm_fp8 epilogue %s, %s" % (epi, what))
        for what, over in FB.ADMITTED_EMPTY:
            keep = G.bits(torch, flat).clone()
            assert FB.gemm_abi_call(L, epi, G.stream(torch), dict(args, **over))() == 0, what
            torch.cuda.synchronize()
            assert torch.equal(keep, G.bits(torch, flat)), what
    assert ffi.counter("gemm_fp8") == before


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def _geo_model(width, heads):
    import torch
    from oracle import hy3d_torch as H
    from r3g import model as M
    from parity_support import bf16_round_matrices
    cfg = H.tiny_config()
    cfg["vae"].update(width=width, heads=heads)
    sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=3))
    gpu = M.ShapeModel(cfg, sd, 0, grid_chunk=4096)
    g = torch.Generator().manual_seed(7)
    gpu.vae_decode(torch.randn(cfg["vae"]["num_latents"], cfg["vae"]["embed_dim"], generator=g))
    return gpu


def test_geo_decoder_fp8_modes_move_the_counter(env):
    """a 17^3 grid in passes of 4096 points is two passes; per pass mode 1 (c_q + MLP) runs three fp8 GEMMs, mode 2 (MLP) two, mode 3 (c_q)
    one.  At width 128 (W % 256 != 0) the option is accepted and every GEMM stays on the bf16 kernels: the counter says so."""
    torch, L, ffi = env
    passes = (17 ** 3 + 4095) // 4096
    for width, heads, per_pass in ((256, 4, {1: 3, 2: 2, 3: 1}), (128, 2, {1: 0, 2: 0, 3: 0})):
        gpu = _geo_model(width, heads)
        plain = gpu.grid_query(1.01, 16).clone()
        for mode in (1, 2, 3):
            with switched(L, ffi, geo_fp8=mode):
                c0 = ffi.counter("gemm_fp8")
                grid = gpu.grid_query(1.01, 16)
                torch.cuda.synchronize()
                moved = ffi.counter("gemm_fp8") - c0
            assert moved == passes * per_pass[mode], "width %d geo_fp8 %d: gemm_fp8 moved by %d" % (width, mode, moved)
            assert bool(torch.isfinite(grid).all())
            assert torch.equal(grid, plain) == (per_pass[mode] == 0)
        c0 = ffi.counter("gemm_fp8")
        gpu.grid_query(1.01, 16)
        assert ffi.counter("gemm_fp8") == c0                  # the option is back at 0
