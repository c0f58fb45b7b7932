"""The row kernels of the texture stage -- the three GroupNorm passes, softmax_rows and geglu (csrc/conv_kernels.hip) -- through
r3g_op_group_norm, r3g_op_softmax_rows and r3g_op_geglu alone.

Per launch: the ELEMENT-WISE bound of tests/row_bounds.py at every output element (tests/test_row_bounds_cpu.py shows that an emulation
of the kernel's arithmetic meets it and that the listed mutants do not), and the output inside a buffer filled with a NaN bit pattern
(tests/row_guard.py) -- eight elements in front, the columns between the width and the leading dimension, two rows past the end --
which keeps its bits outside the launch's elements.  The inputs sit in such buffers too (GroupNorm's addv with add_stride = C + 4).
The closing tests assert that every GroupNorm column regime (several row lanes; one, two, three float4 columns per thread) and the
256-block cap with empty trailing blocks were reached, and that every contract violation of include/r3g.h is refused with
R3G_ERR_INVALID and nothing written.  All shapes are tiny: the file takes a few seconds on an MI355X.
"""
import pytest

import row_bounds as RB
import row_guard as G
from parity_support import report

pytestmark = pytest.mark.gpu

OFF, ptr = G.OFF, G.ptr

GN_REACHED = []


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    ffi.context(0)
    return torch, ffi.lib(), ffi


def run_group_norm(env):
    if GN_REACHED:
        return GN_REACHED[0]
    torch, L, ffi = env
    res = dict(worst={}, failures=[], geos=[], launches=0)
    for rows, C, groups, _ in RB.GN_SHAPES:
        geo = RB.gn_geometry(rows, C)
        for nb in (1, 3):
            n = nb * rows * C
            for addv in (0, 1):
                case = RB.gn_case(rows, C, groups, nb, addv, "cuda")
                xbuf = G.guarded(torch, torch.float32, 2 * OFF + n)
                xbuf[OFF:OFF + n] = case["x"].reshape(-1)
                abuf = None
                if addv:
                    ai = (torch.arange(nb, device="cuda") * case["add_stride"])[:, None] + torch.arange(C, device="cuda")[None]
                    abuf = G.place(torch, G.guarded(torch, torch.float32, nb * case["add_stride"]), ai, case["addv"][:, :C])
                oi = OFF + torch.arange(n, device="cuda")
                for silu in (0, 1):
                    ref, bound = RB.gn_ref_bound(case, silu)
                    tag = "group_norm rows %d c %d groups %d nb %d addv %d silu %d" % (rows, C, groups, nb, addv, silu)
                    y = G.guarded(torch, torch.bfloat16, OFF + n + 2 * C)
                    G.run(torch, ffi, lambda: L.r3g_op_group_norm(ptr(xbuf, OFF), rows, C, groups, ptr(case["gamma"]), ptr(case["beta"]), case["eps"], silu,
                                                                 ptr(y, OFF), nb, ptr(abuf), case["add_stride"] if addv else 0, G.stream(torch)), tag)
                    res["launches"] += 1
                    r = RB.worst_ratio(y[oi].view(nb, rows, C), ref, bound)
                    name = "%d row lanes, %d columns per thread%s" % (geo["P"], geo["cols_per_thread"], ", block cap" if geo["capped"] else "")
                    res["worst"][name] = max(res["worst"].get(name, 0.0), r)
                    if not r <= 1.0:
                        res["failures"].append("%s: error / bound %.3f" % (tag, r))
                    else:
                        res["geos"].append(geo)
                    k, first = G.untouched(torch, y, oi)
                    if k:
                        res["failures"].append("%s: %d elements outside the samples were written, the first at %d" % (tag, k, first - OFF))
    for name, r in sorted(res["worst"].items()):
        report("tex row kernels: group_norm %s (error / bound)" % name, r, 1.0)
    GN_REACHED.append(res)
    return res


def test_group_norm(env):
    res = run_group_norm(env)
    print("group_norm: %d launches, worst error / bound per regime %s" % (res["launches"], {k: round(v, 4) for k, v in sorted(res["worst"].items())}))
    assert not res["failures"], "%d findings, the first: %s" % (len(res["failures"]), "\n".join(res["failures"][:12]))


def test_every_group_norm_regime_was_reached(env):
    """from the geometry (restated in row_bounds.gn_geometry) of the launches that met their bound"""
    geos = run_group_norm(env)["geos"]
    assert {g["cols_per_thread"] for g in geos} == {1, 2, 3}
    assert any(g["P"] > 1 for g in geos) and any(g["P"] == 1 for g in geos)
    assert any(g["capped"] and g["empty_blocks"] > 0 for g in geos)


def test_softmax_rows(env):
    torch, L, ffi = env
    worst, failures = 0.0, []
    for n in RB.SM_N:
        for rows in RB.SM_ROWS:
            case = RB.sm_case(rows, n, "cuda")
            ref, bound, zero = RB.sm_ref_bound(case)
            ld = n + RB.SM_PAD
            ar = lambda k: torch.arange(k, device="cuda")
            idx = (OFF + ar(rows) * ld)[:, None] + ar(n)[None]
            sbuf = G.place(torch, G.guarded(torch, torch.float32, OFF + (rows + 2) * ld), idx, case["s"])
            pbuf = G.guarded(torch, torch.bfloat16, OFF + (rows + 2) * ld)
            tag = "softmax_rows rows %d n %d" % (rows, n)
            G.run(torch, ffi, lambda: L.r3g_op_softmax_rows(ptr(sbuf, OFF), ld, ptr(pbuf, OFF), ld, rows, n, case["scale"], G.stream(torch)), tag)
            got = pbuf[idx]
            r = RB.worst_ratio(got, ref, bound)
            worst = max(worst, r)
            if not r <= 1.0:
                failures.append("%s: error / bound %.3f" % (tag, r))
            if not bool((G.bits(torch, got)[zero] == 0).all()):
                failures.append("%s: a probability below 2^-135 was not stored as zero" % tag)
            if rows == 3 and (n & (n - 1)) == 0 and not bool((got[1] == 1.0 / n).all()):
                failures.append("%s: equal scores with n a power of two did not give 1 / n to the bit" % tag)
            k, first = G.untouched(torch, pbuf, idx)
            if k:
                failures.append("%s: %d elements outside [rows) x [n) were written, the first at %d" % (tag, k, first - OFF))
    report("tex row kernels: softmax_rows (error / bound)", worst, 1.0)
    print("softmax_rows: worst error / bound %.4f" % worst)
    assert not failures, "\n".join(failures)


def test_geglu(env):
    G.glu_run(env, "geglu", env[1].r3g_op_geglu)


def test_geglu_refuses_what_its_kernel_cannot_take(env):
    G.glu_refusals(env, env[1].r3g_op_geglu, "r3g_op_geglu")


def test_group_norm_refuses_what_its_kernels_cannot_take(env):
    torch, L, ffi = env
    rows, C, groups, nb = 17, 64, 32, 2
    x = torch.zeros(OFF + nb * rows * C + 8, device="cuda")
    gb = torch.ones(C + 8, device="cuda")
    av = torch.zeros(nb * (C + 4) + 8, device="cuda")
    y = G.guarded(torch, torch.bfloat16, OFF + nb * rows * C + 2 * C)
    base = dict(x=ptr(x, OFF), rows=rows, C=C, groups=groups, g=ptr(gb), b=ptr(gb), y=ptr(y, OFF), nb=nb, a=ptr(av), ast=C + 4)
    call = lambda a: (lambda: L.r3g_op_group_norm(a["x"], a["rows"], a["C"], a["groups"], a["g"], a["b"], RB.GN_EPS, 1, a["y"], a["nb"], a["a"], a["ast"],
                                                  G.stream(torch)))
    bad = {"x null": dict(base, x=None), "gamma null": dict(base, g=None), "beta null": dict(base, b=None), "y null": dict(base, y=None),
           "rows 0": dict(base, rows=0), "nb 0": dict(base, nb=0), "c % 4": dict(base, C=66, groups=33), "c > 3072": dict(base, C=3200), "groups 0": dict(base, groups=0),
           "groups > 256": dict(base, C=2056, groups=257), "c % groups": dict(base, groups=24), "x 4 bytes off": dict(base, x=ptr(x, OFF + 1)),
           "gamma 8 bytes off": dict(base, g=ptr(gb, 2)), "y 4 bytes off": dict(base, y=ptr(y, OFF + 2)), "addv 4 bytes off": dict(base, a=ptr(av, 1)),
           "add_stride % 4": dict(base, ast=C + 2), "add_stride < c": dict(base, ast=C - 4)}
    for what, a in bad.items():
        G.refused(torch, L, call(a), (y,), "r3g_op_group_norm, " + what)
    for a in (base, dict(base, a=None, ast=0)):
        G.run(torch, ffi, call(a), "r3g_op_group_norm, an admitted call")


def test_softmax_rows_refuses_what_its_kernel_cannot_take(env):
    torch, L, ffi = env
    rows, n = 3, 1020
    s = torch.zeros(OFF + (rows + 1) * (n + 4), device="cuda")
    p = G.guarded(torch, torch.bfloat16, OFF + (rows + 2) * (n + 4))
    base = dict(s=ptr(s, OFF), lds=n + 4, p=ptr(p, OFF), ldp=n + 4, rows=rows, n=n, scale=RB.SM_SCALE)
    call = lambda a: (lambda: L.r3g_op_softmax_rows(a["s"], a["lds"], a["p"], a["ldp"], a["rows"], a["n"], a["scale"], G.stream(torch)))
    bad = {"s null": dict(base, s=None), "p null": dict(base, p=None), "rows 0": dict(base, rows=0), "n 0": dict(base, n=0), "n % 4": dict(base, n=1018),
           "lds < n": dict(base, lds=n - 4), "ldp < n": dict(base, ldp=n - 4), "lds % 4": dict(base, lds=n + 6), "ldp % 4": dict(base, ldp=n + 6),
           "s 4 bytes off": dict(base, s=ptr(s, OFF + 1)), "p 4 bytes off": dict(base, p=ptr(p, OFF + 2)), "scale 0": dict(base, scale=0.0),
           "scale < 0": dict(base, scale=-0.5), "scale nan": dict(base, scale=float("nan")), "scale inf": dict(base, scale=float("inf"))}
    for what, a in bad.items():
        G.refused(torch, L, call(a), (p,), "r3g_op_softmax_rows, " + what)
    G.run(torch, ffi, call(base), "r3g_op_softmax_rows, an admitted call")
