"""Guard buffers and launch handling shared by tests/test_row_kernels_gpu.py and tests/test_tex_row_kernels_gpu.py.

An output lives inside a larger flat buffer filled with a recognisable NaN bit pattern (those of tests/test_gemm_edges_gpu.py, plus 0x7F,
the NaN of e4m3): the elements a launch owns are named by an index tensor, every other element must keep its bits, and an owned element
that was never stored reads back as NaN.  Inputs sit in buffers filled the same way, so that a read outside the operand poisons the result.
A HIP error ends the session (pytest.exit): nothing more is started on a device that has faulted.
"""
import ctypes

import pytest

import row_bounds as RB
from parity_support import report

OFF = 8                       # guard elements in front of every buffer (16 bytes of a 16-bit type, 32 of float32)


def ptr(t, elem_off=0):
    """address of element elem_off of a tensor (None: a null pointer)"""
    return None if t is None else t.data_ptr() + elem_off * t.element_size()


GUARD_BITS = {"bf16": 0x7FA5, "f16": 0x7EA5, "f32": 0x7FA5A5A5, "u8": 0x7F}


def fmt_of(torch, dtype):
    return {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32", torch.uint8: "u8"}[dtype]


def bits(torch, t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def pattern(torch, dtype):
    b = GUARD_BITS[fmt_of(torch, dtype)]
    return b - 0x10000 if (dtype in (torch.bfloat16, torch.float16) and b >= 0x8000) else b


def guarded(torch, dtype, n):
    """a flat buffer of n elements holding the guard pattern"""
    flat = torch.empty(n, device="cuda", dtype=dtype)
    bits(torch, flat).fill_(pattern(torch, dtype))
    return flat


def place(torch, flat, idx, values):
    """values (any shape) into flat at the element indices idx (same shape)"""
    flat[idx.reshape(-1)] = values.reshape(-1).to(flat.dtype)
    return flat


def untouched(torch, flat, owned_idx):
    """number of elements outside owned_idx that lost the guard pattern, and the first such index (or -1)"""
    bad = bits(torch, flat) != pattern(torch, flat.dtype)
    bad[owned_idx.reshape(-1)] = False
    n = int(bad.sum())
    return n, (int(bad.nonzero()[0]) if n else -1)


def stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(torch, ffi, call, tag):
    """issue one launch and wait for it.  R3G_ERR_INVALID (the launch was refused, nothing ran) is an ordinary failure and is raised; any
    other error is a HIP error: nothing more is started on this device"""
    try:
        ffi.check(call())
        torch.cuda.synchronize()
    except Exception as e:
        if getattr(e, "code", None) == -1:
            raise
        pytest.exit("%s: %r" % (tag, e), returncode=3)


def refused(torch, L, call, buffers, what):
    """the call returns R3G_ERR_INVALID and not one bit of `buffers` changes"""
    before = [bits(torch, b).clone() for b in buffers]
    rc = call()
    torch.cuda.synchronize()
    assert rc == -1, "%s: returned %d, expected R3G_ERR_INVALID (%s)" % (what, rc, L.r3g_last_error().decode("utf-8", "replace"))
    for b, old in zip(buffers, before):
        assert torch.equal(bits(torch, b), old), "%s: a refused call wrote" % what


def glu_run(env, kind, fn):
    """geglu | swiglu through fn at every shape of row_bounds (rows x F, ldi = 2 F + 8, ldo = F + 8): bound, guards, report"""
    torch, L, ffi = env
    worst, failures = 0.0, []
    for rows in RB.GLU_ROWS:
        for F in RB.GLU_F:
            case = RB.glu_case(rows, F, "cuda")
            ref, bound = RB.glu_ref_bound(case, kind)
            ldi, ldo = 2 * F + RB.GLU_PAD, F + RB.GLU_PAD
            ar = lambda n: torch.arange(n, device="cuda")
            ii = (OFF + ar(rows) * ldi)[:, None] + ar(2 * F)[None]
            oi = (OFF + ar(rows) * ldo)[:, None] + ar(F)[None]
            xin = place(torch, guarded(torch, torch.bfloat16, OFF + (rows + 2) * ldi), ii, case["x"])
            out = guarded(torch, torch.bfloat16, OFF + (rows + 2) * ldo)
            tag = "%s rows %d f %d" % (kind, rows, F)
            run(torch, ffi, lambda: fn(ptr(xin, OFF), ldi, ptr(out, OFF), ldo, rows, F, stream(torch)), tag)
            r = RB.worst_ratio(out[oi], ref, bound)
            worst = max(worst, r)
            if not r <= 1.0:
                failures.append("%s: error / bound %.3f" % (tag, r))
            n, first = untouched(torch, out, oi)
            if n:
                failures.append("%s: %d elements outside [rows) x [f) were written, the first at %d" % (tag, n, first - OFF))
    report("row kernels: %s (error / bound)" % kind, worst, 1.0)
    print("%s: worst error / bound %.4f" % (kind, worst))
    assert not failures, "\n".join(failures)


def glu_refusals(env, fn, name):
    torch, L, ffi = env
    rows, F = 3, 72
    xin = torch.zeros(OFF + (rows + 1) * (2 * F + 8), device="cuda", dtype=torch.bfloat16)
    out = guarded(torch, torch.bfloat16, OFF + (rows + 2) * (F + 8))
    base = dict(i=ptr(xin, OFF), ldi=2 * F + 8, o=ptr(out, OFF), ldo=F + 8, rows=rows, F=F)
    call = lambda a: (lambda: fn(a["i"], a["ldi"], a["o"], a["ldo"], a["rows"], a["F"], stream(torch)))
    bad = {"in null": dict(base, i=None), "out null": dict(base, o=None), "rows 0": dict(base, rows=0), "f 0": dict(base, F=0), "f % 8": dict(base, F=68),
           "ldi < 2 f": dict(base, ldi=2 * F - 8), "ldo < f": dict(base, ldo=F - 8), "ldi % 8": dict(base, ldi=2 * F + 4), "ldo % 8": dict(base, ldo=F + 4),
           "in 8 bytes off": dict(base, i=ptr(xin, OFF + 4)), "out 8 bytes off": dict(base, o=ptr(out, OFF + 4))}
    for what, a in bad.items():
        refused(torch, L, call(a), (out,), "%s, %s" % (name, what))
    run(torch, ffi, call(base), name + ", an admitted call")
