"""The row kernels of the shape models -- every LayerNorm form (layernorm_small_kernel and the instantiations of layernorm_kernel: run-time
count, fixed 1024 with MODE 1 / 2 / -1, fixed 1536, each with 1 and 4 rows per wave and f32 / bf16 / fp16 rows), ln_dot, qkv_split and swiglu --
through r3g_op_layernorm, r3g_op_ln_dot, r3g_op_qkv_split and r3g_op_swiglu alone.

Per launch:
  * the ELEMENT-WISE bound of tests/row_bounds.py at every output element (derived there; tests/test_row_bounds_cpu.py shows that an
    emulation of the kernel's arithmetic meets it and that the listed mutants do not);
  * the output sits in a larger buffer filled with a NaN bit pattern (tests/row_guard.py): eight elements in front, the columns between
    the width and the leading dimension, the gap between batches, two rows past the end -- for qkv_split every Q / K row and V^T column
    the call does not own.  Those keep their bits; an owned element that was never stored is a NaN.  The inputs sit in such buffers too;
  * the counters ln_rows1, ln_rows4, ln_fixed_count and ln_mode_inst move exactly as row_bounds.ln_form / ln_dot_form (the launchers'
    rules restated) say -- the scalar kernels move none.
The closing tests assert that every LayerNorm form was reached with a row tail, and that every contract violation of include/r3g.h is
refused with R3G_ERR_INVALID and nothing written.  All shapes are tiny: the file takes a few seconds on an MI355X.
"""
import pytest

import row_bounds as RB
import row_guard as G
from parity_support import report
from switch_table import switched

pytestmark = pytest.mark.gpu

OFF = G.OFF
_CASES, _LAYOUTS, _LN_RESULTS = {}, {}, {}
LN_REACHED = set()


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    ffi.context(0)
    return torch, ffi.lib(), ffi


ptr = G.ptr


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------
def ln_layout(torch, C, rows, rpb):
    """element indices [rows][C] of the rows inside a flat buffer: ld = C + 8, batch stride rows_per_batch * ld + 8, 8 in front, 2 rows behind"""
    key = (C, rows, rpb)
    if key not in _LAYOUTS:
        ld = C + RB.LN_PAD
        bs = rpb * ld + 8
        r = torch.arange(rows, device="cuda")
        idx = (OFF + (r // rpb) * bs + (r % rpb) * ld)[:, None] + torch.arange(C, device="cuda")[None]
        _LAYOUTS[key] = dict(ld=ld, bs=bs, idx=idx, total=OFF + ((rows + rpb - 1) // rpb) * bs + 2 * ld)
    return _LAYOUTS[key]


def ln_prepared(torch, C, xf, rc, combo, zero_row=None):
    """the operands of one case on the device, its reference and bound, memoised"""
    key = (C, xf, rc[0], combo, zero_row)
    if key not in _CASES:
        case = RB.ln_case(C, xf, rc, combo, "cuda", zero_row=zero_row)
        lay = ln_layout(torch, C, case["rows"], case["rpb"])
        xbuf = G.place(torch, G.guarded(torch, RB.XDTYPE[xf], lay["total"]), lay["idx"], case["x"])
        ms = C + 4                                                  # mod_stride != 0; the four floats between two batches' vectors are guards
        mod = {}
        for name in ("scale", "shift"):
            if case[name] is not None:
                nb = case["nbatch"]
                mi = (torch.arange(nb, device="cuda") * ms)[:, None] + torch.arange(C, device="cuda")[None]
                mod[name] = G.place(torch, G.guarded(torch, torch.float32, nb * ms), mi, case[name])
        ref_err = RB.ln_ref_err(case)
        _CASES[key] = dict(case=case, lay=lay, xbuf=xbuf, mod=mod, ms=ms, ref_err=ref_err, ref=ref_err[0], bound=RB.bf16_bound(*ref_err))
    return _CASES[key]


def ln_call(torch, L, pr, ybuf, y8=None, ldy8=0, yscale=None):
    case, lay = pr["case"], pr["lay"]
    seg2 = case["seg2"] or (0, 0)
    fp8 = y8 is not None
    return lambda: L.r3g_op_layernorm(
        ptr(pr["xbuf"], OFF), case["x_format"], lay["ld"], 0 if fp8 else lay["bs"], None if fp8 else ptr(ybuf, OFF), 0 if fp8 else lay["ld"],
        0 if fp8 else lay["bs"], ptr(y8, OFF) if fp8 else None, ldy8, ptr(yscale, 4) if fp8 else None, ptr(case["w"]), ptr(case["b"]),
        ptr(pr["mod"].get("scale")), ptr(pr["mod"].get("shift")), pr["ms"], seg2[0], seg2[1], ptr(case["scale2"]), ptr(case["shift2"]),
        case["rows"], case["C"], case["rpb"], case["eps"], G.stream(torch))


def counters(ffi):
    return {c: ffi.counter(c) for c in RB.LN_COUNTERS}


def run_layernorm(env, C):
    if C in _LN_RESULTS:
        return _LN_RESULTS[C]
    torch, L, ffi = env
    res = dict(worst={}, failures=[], launches=0)
    for C_, xf, (rpw, fixed, modes), rc, combo in RB.ln_plan():
        if C_ != C:
            continue
        pr = ln_prepared(torch, C, xf, rc, combo)
        case, lay = pr["case"], pr["lay"]
        form = RB.ln_form(C, xf, lay["ld"], lay["ld"], RB.combo_has(combo, rc[3]), case["rows"], rpw, fixed, modes, seg2=bool(rc[3]))
        tag = "layernorm C %d format %d ln_rows %d ln_fixed %d ln_modes %d %s %s" % (C, xf, rpw, fixed, modes, rc[0], combo)
        ybuf = G.guarded(torch, torch.bfloat16, lay["total"])
        with switched(L, ffi, ln_rows=rpw, ln_fixed=fixed, ln_modes=modes):
            c0 = counters(ffi)
            G.run(torch, ffi, ln_call(torch, L, pr, ybuf), tag)
            moved = {c: v - c0[c] for c, v in counters(ffi).items()}
        res["launches"] += 1
        if moved != form["counters"]:
            res["failures"].append("%s: counters moved %s, expected %s" % (tag, moved, form["counters"]))
        name = "%s nv %d mode %d rows/wave %d format %d" % (form["kernel"], form["nv"], form["mode"], form["rpw"], xf)
        r = RB.worst_ratio(ybuf[lay["idx"]], pr["ref"], pr["bound"])
        res["worst"][name] = max(res["worst"].get(name, 0.0), r)
        if not r <= 1.0:
            res["failures"].append("%s: error / bound %.3f" % (tag, r))
        n, first = G.untouched(torch, ybuf, lay["idx"])
        if n:
            res["failures"].append("%s: %d elements outside the rows were written, the first at element %d" % (tag, n, first - OFF))
        if moved == form["counters"] and r <= 1.0 and case["rows"] % (4 * form["rpw"]):
            LN_REACHED.add((form["kernel"], form["nv"], form["mode"], form["rpw"], xf))
    for name, r in sorted(res["worst"].items()):
        report("row kernels: layernorm C %d %s (error / bound)" % (C, name), r, 1.0)
    _LN_RESULTS[C] = res
    return res


@pytest.mark.parametrize("C", RB.LN_C)
def test_layernorm(env, C):
    res = run_layernorm(env, C)
    print("layernorm C %d: %d launches, worst error / bound per form %s" % (C, res["launches"], {k: round(v, 4) for k, v in sorted(res["worst"].items())}))
    assert not res["failures"], "%d findings, the first: %s" % (len(res["failures"]), "\n".join(res["failures"][:12]))


def test_layernorm_e4m3_output(env):
    """the e4m3 form (MODE -1 whatever the operands) at C = 256 and 1024: the row scales, every code, and the all-zero row (row 2: scale 1
    and zero codes where no additive term is given)"""
    torch, L, ffi = env
    worst_s = worst_c = 0.0
    for C in (256, 1024):
        for xf in (0, 1, 2):
            for rc in RB.LN_ROWCFGS[1:3]:
                for combo in ("none", "affine_mod"):
                    pr = ln_prepared(torch, C, xf, rc, combo, zero_row=2)
                    case, rows = pr["case"], rc[1]
                    ld8 = C + 8
                    i8 = (OFF + torch.arange(rows, device="cuda") * ld8)[:, None] + torch.arange(C, device="cuda")[None]
                    isc = 4 + torch.arange(rows, device="cuda")
                    for rpw in (1, 4):
                        for fixed in ((0, 1) if C == 1024 else (1,)):
                            tag = "layernorm e4m3 C %d format %d ln_rows %d ln_fixed %d %s %s" % (C, xf, rpw, fixed, rc[0], combo)
                            y8 = G.guarded(torch, torch.uint8, OFF + (rows + 2) * ld8)
                            ysc = G.guarded(torch, torch.float32, rows + 8)
                            form = RB.ln_form(C, xf, pr["lay"]["ld"], 0, RB.combo_has(combo, None), rows, rpw, fixed, 1, fp8=True)
                            with switched(L, ffi, ln_rows=rpw, ln_fixed=fixed):
                                c0 = counters(ffi)
                                G.run(torch, ffi, ln_call(torch, L, pr, None, y8, ld8, ysc), tag)
                                moved = {c: v - c0[c] for c, v in counters(ffi).items()}
                            assert moved == form["counters"] and form["mode"] == -1, tag
                            rs, rcodes, zeros_ok = RB.ln_fp8_check(case, y8[i8], ysc[isc], pr["ref_err"])
                            worst_s, worst_c = max(worst_s, rs), max(worst_c, rcodes)
                            assert rs <= 1.0 and rcodes <= 1.0 and zeros_ok, "%s: scale error / bound %.3f, code error / bound %.3f, zero rows %s" % (tag, rs, rcodes, zeros_ok)
                            if combo == "none":
                                assert float(ysc[4 + 2]) == 1.0 and int(y8[i8][2].max()) == 0, tag
                            assert G.untouched(torch, y8, i8)[0] == 0 and G.untouched(torch, ysc, isc)[0] == 0, tag
    report("row kernels: layernorm e4m3 row scale (error / bound)", worst_s, 1.0)
    report("row kernels: layernorm e4m3 codes (error / bound)", worst_c, 1.0)
    print("layernorm e4m3: worst scale error / bound %.4f, worst code error / bound %.4f" % (worst_s, worst_c))


def test_every_layernorm_form_was_reached_with_a_row_tail(env):
    """Reads what the tests above recorded: a form counts when its launch moved the counters the restated rule names, met the bound and
    ended in a partial workgroup.  A width that has not run yet in this session (the test selected alone) is run here."""
    for C in RB.LN_C:
        run_layernorm(env, C)
    missing = RB.ln_forms_required() - LN_REACHED
    assert not missing, "LayerNorm forms (kernel, nv, mode, rows per wave, x format) not reached: %s" % sorted(missing)


# ---- ln_dot -------------------------------------------------------------------------------------------------------------------------------
def test_ln_dot(env):
    torch, L, ffi = env
    worst, failures, reached = {}, [], set()
    for C in RB.LND_C:
        for xb in ((0, 1) if C % 256 == 0 else (0,)):
            for rows in RB.LND_ROWS:
                ld = C + RB.LND_PAD
                xi = (OFF + torch.arange(rows, device="cuda") * ld)[:, None] + torch.arange(C, device="cuda")[None]
                oi = 4 + torch.arange(rows, device="cuda")
                for do_ln in (0, 1):
                    for affine in ((0, 1) if do_ln else (0,)):
                        case = RB.lnd_case(C, xb, rows, do_ln, affine, "cuda")
                        ref, bound = RB.lnd_ref_bound(case)
                        xbuf = G.place(torch, G.guarded(torch, RB.XDTYPE[xb], OFF + (rows + 2) * ld), xi, case["x"])
                        vec = RB.ln_dot_form(C, xb, ld, rows)["kernel"] == "vec"
                        for rpw in ((1, 4) if vec else (1,)):
                            for fixed in ((0, 1) if (vec and C == 1024) else (1,)):
                                form = RB.ln_dot_form(C, xb, ld, rows, rpw, fixed)
                                tag = "ln_dot C %d bf16 %d rows %d do_ln %d affine %d ln_rows %d ln_fixed %d" % (C, xb, rows, do_ln, affine, rpw, fixed)
                                out = G.guarded(torch, torch.float32, rows + 8)
                                with switched(L, ffi, ln_rows=rpw, ln_fixed=fixed):
                                    c0 = counters(ffi)
                                    G.run(torch, ffi, lambda: L.r3g_op_ln_dot(ptr(xbuf, OFF), xb, ld, rows, C, do_ln, ptr(case["lnw"]), ptr(case["lnb"]),
                                                                              case["eps"], ptr(case["w"]), case["b"], ptr(out, 4), G.stream(torch)), tag)
                                    moved = {c: v - c0[c] for c, v in counters(ffi).items()}
                                if moved != form["counters"]:
                                    failures.append("%s: counters moved %s, expected %s" % (tag, moved, form["counters"]))
                                name = "%s nv %d rows/wave %d bf16 %d" % (form["kernel"], form["nv"], form["rpw"], xb)
                                r = RB.worst_ratio(out[oi], ref, bound)
                                worst[name] = max(worst.get(name, 0.0), r)
                                if not r <= 1.0:
                                    failures.append("%s: error / bound %.3f" % (tag, r))
                                if G.untouched(torch, out, oi)[0]:
                                    failures.append("%s: wrote outside its %d outputs" % (tag, rows))
                                reached.add((form["kernel"], form["nv"], form["rpw"], xb))
    for name, r in sorted(worst.items()):
        report("row kernels: ln_dot %s (error / bound)" % name, r, 1.0)
    print("ln_dot: worst error / bound per form %s" % {k: round(v, 4) for k, v in sorted(worst.items())})
    assert not failures, "%d findings, the first: %s" % (len(failures), "\n".join(failures[:12]))
    assert reached == {("small", 0, 1, 0)} | {("vec", nv, rpw, xb) for nv in (0, 4) for rpw in (1, 4) for xb in (0, 1)}


# ---- qkv_split ----------------------------------------------------------------------------------------------------------------------------
def test_qkv_split(env):
    torch, L, ffi = env
    worst, failures, launches = {}, [], 0
    for Lt in RB.QKV_L:
        for B, H in RB.QKV_BH:
            for dst in (0, 64):
                lk_pad = (dst + Lt + 63) // 64 * 64
                lq_pad = (dst + Lt + 127) // 128 * 128
                lq_pad += 128 if lq_pad == lk_pad else 0                       # Lq_pad != Lk_pad
                ar = lambda n: torch.arange(n, device="cuda")
                # owned elements: rows dst .. dst + l of every (batch, head) of Q / K; columns dst .. dst + the 64-token blocks of l of every V^T row
                qi = lambda pad: OFF + ((ar(B * H) * pad)[:, None, None] + (dst + ar(Lt))[None, :, None]) * 64 + ar(64)[None, None, :]
                nvt = (Lt + 63) // 64 * 64
                vi = OFF + (ar(B * H * 64) * lk_pad)[:, None] + (dst + ar(nvt))[None, :]
                for layout in RB.QKV_LAYOUTS:
                    for norm, weights in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
                        for q_scale in RB.QKV_QSCALE:
                            case = RB.qkv_case(Lt, B, H, layout, norm, weights, q_scale, "cuda")
                            tag = "qkv_split l %d batch %d heads %d dst_row0 %d %s norm %d weights %d q_scale %.3f" % (Lt, B, H, dst, layout, norm, weights, q_scale)
                            has = {w: case[w + "_off"] >= 0 for w in "qkv"}
                            src = G.guarded(torch, torch.bfloat16, OFF + B * Lt * case["ld"] + 16)
                            src[OFF:OFF + B * Lt * case["ld"]] = case["src"].reshape(-1)
                            Q = G.guarded(torch, torch.bfloat16, 2 * OFF + B * H * lq_pad * 64) if has["q"] else None
                            K = G.guarded(torch, torch.bfloat16, 2 * OFF + B * H * lk_pad * 64) if has["k"] else None
                            Vt = G.guarded(torch, torch.bfloat16, 2 * OFF + B * H * 64 * lk_pad) if has["v"] else None
                            G.run(torch, ffi, lambda: L.r3g_op_qkv_split(
                                ptr(src, OFF), case["ld"], Lt * case["ld"], case["q_off"], case["k_off"], case["v_off"], case["hs"], ptr(Q, OFF), ptr(K, OFF),
                                ptr(Vt, OFF), lq_pad, lk_pad, dst, B, H, Lt, norm, ptr(case["qw"]), ptr(case["qb"]), ptr(case["kw"]), ptr(case["kb"]),
                                case["eps"], q_scale, G.stream(torch)), tag)
                            launches += 1
                            for which, buf, pad in (("q", Q, lq_pad), ("k", K, lk_pad)):
                                if buf is None:
                                    continue
                                ref, bound = RB.qkv_norm_ref_bound(case, which)
                                idx = qi(pad)
                                r = RB.worst_ratio(buf[idx].view(B, H, Lt, 64), ref, bound)
                                name = "%s norm %d" % (which, norm)
                                worst[name] = max(worst.get(name, 0.0), r)
                                if not r <= 1.0:
                                    failures.append("%s: %s error / bound %.3f" % (tag, which, r))
                                n, first = G.untouched(torch, buf, idx)
                                if n:
                                    failures.append("%s: %d elements of %s outside the call's rows were written, the first at %d" % (tag, n, which.upper(), first - OFF))
                            if Vt is not None:
                                want = RB.qkv_vt_expected(case, dst)[1]
                                if not torch.equal(G.bits(torch, Vt[vi].view(B, H, 64, nvt)), G.bits(torch, want)):
                                    failures.append("%s: V^T differs from the transposed v in the kernel's key order (zeros past l)" % tag)
                                n, first = G.untouched(torch, Vt, vi)
                                if n:
                                    failures.append("%s: %d V^T elements outside the call's columns were written, the first at %d" % (tag, n, first - OFF))
    for name, r in sorted(worst.items()):
        report("row kernels: qkv_split %s (error / bound)" % name, r, 1.0)
    print("qkv_split: %d launches, worst error / bound %s" % (launches, {k: round(v, 4) for k, v in sorted(worst.items())}))
    assert not failures, "%d findings, the first: %s" % (len(failures), "\n".join(failures[:12]))


# ---- swiglu -------------------------------------------------------------------------------------------------------------------------------
def test_swiglu(env):
    G.glu_run(env, "swiglu", env[1].r3g_op_swiglu)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_layernorm_refuses_what_its_kernels_cannot_take(env):
    torch, L, ffi = env
    C, rows = 256, 5
    pr = ln_prepared(torch, C, 0, RB.LN_ROWCFGS[1], "affine_mod")
    pr16 = ln_prepared(torch, C, 1, RB.LN_ROWCFGS[1], "affine_mod")
    case, lay = pr["case"], pr["lay"]
    ybuf = G.guarded(torch, torch.bfloat16, lay["total"])
    y8 = G.guarded(torch, torch.uint8, OFF + (rows + 2) * (C + 8))
    ysc = G.guarded(torch, torch.float32, rows + 8)
    s2 = torch.zeros(C, device="cuda")
    base = dict(x=ptr(pr["xbuf"], OFF), xf=0, ldx=lay["ld"], xbs=lay["bs"], y=ptr(ybuf, OFF), ldy=lay["ld"], ybs=lay["bs"], y8=None, ldy8=0, ysc=None,
                w=ptr(case["w"]), b=ptr(case["b"]), sc=ptr(pr["mod"]["scale"]), sh=ptr(pr["mod"]["shift"]), ms=pr["ms"], s0=0, s1=0, sc2=None, sh2=None,
                rows=rows, C=C, rpb=rows, eps=case["eps"])
    fp8 = dict(base, y=None, ldy=0, xbs=0, ybs=0, y8=ptr(y8, OFF), ldy8=C + 8, ysc=ptr(ysc, 4))

    def call(a):
        return lambda: L.r3g_op_layernorm(a["x"], a["xf"], a["ldx"], a["xbs"], a["y"], a["ldy"], a["ybs"], a["y8"], a["ldy8"], a["ysc"], a["w"], a["b"],
                                          a["sc"], a["sh"], a["ms"], a["s0"], a["s1"], a["sc2"], a["sh2"], a["rows"], a["C"], a["rpb"], a["eps"], G.stream(torch))

    bad = {
        "x null": dict(base, x=None), "y null": dict(base, y=None), "rows 0": dict(base, rows=0), "rows_per_batch 0": dict(base, rpb=0),
        "c 2112": dict(base, C=2112), "c 32": dict(base, C=32), "c 96": dict(base, C=96), "x_format 3": dict(base, xf=3),
        "16-bit rows at c 192": dict(base, xf=1, x=ptr(pr16["xbuf"], OFF), C=192),
        "ldx < c": dict(base, ldx=C - 4), "ldy < c": dict(base, ldy=C - 4),
        "x_batch_stride % 4 on the vector kernel": dict(base, rpb=2, xbs=2 * lay["ld"] + 2),
        "y_batch_stride % 4": dict(base, rpb=2, ybs=2 * lay["ld"] + 2), "y batches overlap": dict(base, rpb=2, ybs=lay["ld"]),
        "x 4 bytes off": dict(base, x=ptr(pr["xbuf"], OFF + 1)), "y 4 bytes off": dict(base, y=ptr(ybuf, OFF + 2)),
        "bf16 x 4 bytes off": dict(base, xf=1, x=ptr(pr16["xbuf"], OFF + 2)), "bf16 ldx % 4": dict(base, xf=1, x=ptr(pr16["xbuf"], OFF), ldx=C + 2),
        "w 4 bytes off": dict(base, w=ptr(case["w"], 1)), "shift 8 bytes off": dict(base, sh=ptr(pr["mod"]["shift"], 2)), "mod_stride % 4": dict(base, ms=C + 2, rpb=2),
        "seg2 without scale2": dict(base, s0=1, s1=3, sh2=ptr(s2)), "seg2 without shift2": dict(base, s0=1, s1=3, sc2=ptr(s2)),
        "e4m3 with y": dict(fp8, y=ptr(ybuf, OFF)), "e4m3 without y_scale": dict(fp8, ysc=None), "e4m3 with rows_per_batch < rows": dict(fp8, rpb=2),
        "e4m3 with a y stride": dict(fp8, ldy=lay["ld"]), "e4m3 with batch strides": dict(fp8, xbs=lay["bs"]), "e4m3 ldy8 % 4": dict(fp8, ldy8=C + 6),
        "e4m3 ldy8 < c": dict(fp8, ldy8=C - 4), "e4m3 on the scalar kernel": dict(fp8, ldx=C + 2), "e4m3 at c 192": dict(fp8, C=192),
    }
    for what, a in bad.items():
        G.refused(torch, L, call(a), (ybuf, y8, ysc), "r3g_op_layernorm, " + what)
    for a in (base, fp8, dict(base, ldx=C + 10)):        # ... and the contract's loosest forms are accepted (ldx % 4 != 0: the scalar kernel)
        G.run(torch, ffi, call(a), "r3g_op_layernorm, an admitted call")


def test_ln_dot_refuses_what_its_kernels_cannot_take(env):
    torch, L, ffi = env
    C, rows = 256, 5
    case = RB.lnd_case(C, 0, rows, 1, 1, "cuda")
    x = torch.zeros(OFF + (rows + 1) * (C + 4), device="cuda")
    out = G.guarded(torch, torch.float32, rows + 8)
    base = dict(x=ptr(x, OFF), xb=0, ldx=C + 4, rows=rows, C=C, do_ln=1, lnw=ptr(case["lnw"]), lnb=ptr(case["lnb"]), w=ptr(case["w"]), out=ptr(out, 4))
    call = lambda a: (lambda: L.r3g_op_ln_dot(a["x"], a["xb"], a["ldx"], a["rows"], a["C"], a["do_ln"], a["lnw"], a["lnb"], case["eps"], a["w"], 0.5,
                                              a["out"], G.stream(torch)))
    bad = {"x null": dict(base, x=None), "w null": dict(base, w=None), "out null": dict(base, out=None), "lnw without lnb": dict(base, lnb=None),
           "rows 0": dict(base, rows=0), "c 96": dict(base, C=96), "c 2112": dict(base, C=2112), "ldx < c": dict(base, ldx=C - 4),
           "bf16 rows at c 192": dict(base, xb=1, C=192), "bf16 ldx % 4": dict(base, xb=1, ldx=C + 2), "x_bf16 2": dict(base, xb=2),
           "x 4 bytes off": dict(base, x=ptr(x, OFF + 1)), "w 4 bytes off": dict(base, w=ptr(case["w"], 1)), "lnb 8 bytes off": dict(base, lnb=ptr(case["lnb"], 2))}
    for what, a in bad.items():
        G.refused(torch, L, call(a), (out,), "r3g_op_ln_dot, " + what)
    for a in (base, dict(base, ldx=C + 2), dict(base, lnw=None, lnb=None)):
        G.run(torch, ffi, call(a), "r3g_op_ln_dot, an admitted call")


def test_qkv_split_refuses_what_its_kernel_cannot_take(env):
    torch, L, ffi = env
    B, H, Lt = 1, 2, 65
    case = RB.qkv_case(Lt, B, H, "khd", 2, 1, 0.0, "cuda")
    src = case["src"].contiguous()
    Q = G.guarded(torch, torch.bfloat16, B * H * 256 * 64)
    K = G.guarded(torch, torch.bfloat16, B * H * 128 * 64)
    Vt = G.guarded(torch, torch.bfloat16, B * H * 64 * 128)
    base = dict(src=ptr(src), ld=case["ld"], q_off=0, k_off=128, v_off=256, hs=64, Q=ptr(Q), K=ptr(K), Vt=ptr(Vt), lq_pad=256, lk_pad=128, dst=0, B=B, H=H,
                L=Lt, norm=2)
    call = lambda a: (lambda: L.r3g_op_qkv_split(a["src"], a["ld"], Lt * case["ld"], a["q_off"], a["k_off"], a["v_off"], a["hs"], a["Q"], a["K"], a["Vt"],
                                                 a["lq_pad"], a["lk_pad"], a["dst"], a["B"], a["H"], a["L"], a["norm"], ptr(case["qw"]), ptr(case["qb"]),
                                                 ptr(case["kw"]), ptr(case["kb"]), case["eps"], 0.0, G.stream(torch)))
    bad = {"src null": dict(base, src=None), "q_off without Q": dict(base, Q=None), "K without k_off": dict(base, k_off=-1),
           "nothing to do": dict(base, q_off=-1, k_off=-1, v_off=-1, Q=None, K=None, Vt=None), "l 0": dict(base, L=0), "heads 0": dict(base, H=0),
           "batch 0": dict(base, B=0), "norm 3": dict(base, norm=3), "dst_row0 % 64": dict(base, dst=32), "dst_row0 < 0": dict(base, dst=-64),
           "lq_pad % 128": dict(base, lq_pad=192), "lk_pad % 64": dict(base, lk_pad=96), "rows beyond lk_pad": dict(base, dst=64),
           "rows beyond lq_pad": dict(base, lq_pad=128, lk_pad=192, dst=64), "columns beyond ld": dict(base, ld=case["ld"] - 16),
           "head_stride < 0": dict(base, hs=-64)}
    for what, a in bad.items():
        G.refused(torch, L, call(a), (Q, K, Vt), "r3g_op_qkv_split, " + what)
    G.run(torch, ffi, call(base), "r3g_op_qkv_split, an admitted call")


def test_swiglu_refuses_what_its_kernel_cannot_take(env):
    G.glu_refusals(env, env[1].r3g_op_swiglu, "r3g_op_swiglu")
