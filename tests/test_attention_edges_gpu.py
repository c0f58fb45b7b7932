"""Every attention generation (7 = the default, 1, 2, 3, 4, 5, 6, 9 and the pipelined first-round kernel; register staging for 2 and 7;
"attn_variant" 0 and 1 for 2 and 6; 7 with "attn_wide_min" 1, where it takes 6) at short and tile-straddling sequences, through
r3g_op_attention alone.

Per launch:
  * the ELEMENT-WISE bound of tests/edge_bounds.py at every element of O, against a float64 softmax of the Q the MFMA sees (re-rounded
    q * 0.125 log2 e from generation 2 on, plain q for generation 1 and the pipelined kernel); tests/test_edge_bounds_cpu.py shows that a
    kernel with P in bf16 meets it and that an unmasked padded key, an unswapped V^T group and a row sum over Lk_pad do not;
  * padded Q rows and padded K rows hold large finite junk (+-1e4 in both, the sign alternating by row; a third fill keeps the +-7 keys of
    tests/test_ops_gpu.py), padded V^T keys are zero as include/r3g.h requires; the three fills give the SAME BITS: the junk decides
    nothing, and each is held to the bound;
  * O is followed by eight rows of a NaN bit pattern that keep their bits, and starts out as that pattern: a row that was never stored is
    a NaN.  (r3g_op_attention fixes O's batch stride at lq rows, so the guard rows can only follow the LAST batch entry; a store past lq
    of an earlier entry lands in the next entry's rows, where the bound sees it unless that entry overwrites it.  Each two-entry shape
    therefore has a one-entry shape with the same Lq beside it: (1, 2, 129, 65) and (1, 2, 129, 17) for Lq = 129, (1, 2, 33, 5) and
    (1, 1, 33, 65) for Lq = 33.)
  * with one key the output is the bf16 v[0] exactly, for every query;
  * the launch counters show that the intended kernel ran, and no other.
"""
import ctypes

import pytest

import edge_bounds as EB
from parity_support import report
from switch_table import switched

pytestmark = pytest.mark.gpu

GUARD_ROWS = 8
GUARD_BITS = 0x7FA5
COUNTERS = ("attn_gen1", "attn_pipelined", "attn_gen2", "attn_gen3", "attn_gen4", "attn_gen5", "attn_gen6", "attn_gen9", "attn_register_staged")
# id: (switches, use_lds_dma, Q re-rounded by the kernel, the counters that move)
CONFIGS = {
    "gen7": (dict(), 1, True, ("attn_gen2",)),                                   # 7 = 2 below attn_wide_min work items of 256 queries
    "gen7-wide_min1": (dict(attn_wide_min=1), 1, True, ("attn_gen6",)),          # ... and 6 from there on
    "gen7-reg": (dict(), 0, True, ("attn_gen2", "attn_register_staged")),
    "gen1": (dict(attn_generation=1), 1, False, ("attn_gen1",)),
    "pipelined": (dict(attn_pipelined=1), 1, False, ("attn_pipelined",)),
    "gen2-variant1": (dict(attn_generation=2, attn_variant=1), 1, True, ("attn_gen2",)),
    "gen2-variant0": (dict(attn_generation=2, attn_variant=0), 1, True, ("attn_gen2",)),
    "gen2-reg": (dict(attn_generation=2), 0, True, ("attn_gen2", "attn_register_staged")),
    "gen3": (dict(attn_generation=3), 1, True, ("attn_gen3",)),
    "gen4": (dict(attn_generation=4), 1, True, ("attn_gen4",)),
    "gen5": (dict(attn_generation=5), 1, True, ("attn_gen5",)),
    "gen6-variant1": (dict(attn_generation=6, attn_variant=1), 1, True, ("attn_gen6",)),
    "gen6-variant0": (dict(attn_generation=6, attn_variant=0), 1, True, ("attn_gen6",)),
    "gen9": (dict(attn_generation=9), 1, True, ("attn_gen9",)),
}

_CASES = {}


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    ffi.context(0)
    return torch, ffi.lib(), ffi


def _case(shape):
    """operands, the padded ABI operands under both junk fills, and (reference, bound) for both forms of Q: built once, never changed"""
    if shape not in _CASES:
        ops = EB.attn_operands(*shape, device="cuda")
        _CASES[shape] = (ops, [EB.attn_padded(ops, *f) for f in EB.JUNK_FILLS], {pre: EB.attn_ref_bound(ops, pre) for pre in (True, False)})
    return _CASES[shape]


def test_vt_layout_of_the_bounds_module_is_the_librarys(env):
    torch, L, ffi = env
    from r3g.layout import make_vt
    ops, padded, _ = _case(EB.ATTN_SHAPES[3][:5])
    assert torch.equal(padded[0][2], make_vt(ops["v"], padded[0][4]))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_attention_edges(env, name):
    torch, L, ffi = env
    switches, dma, prescaled, moves = CONFIGS[name]
    failures, worst = [], 0.0
    with switched(L, ffi, **switches):
        for shape in EB.ATTN_SHAPES:
            B, H, Lq, Lk, shared = shape[:5]
            ops, padded, refs = _case(shape[:5])
            ref, bound = refs[prescaled]
            outs = []
            for Q, K, Vt, lqp, lkp in padded:
                buf = torch.empty(B * Lq + GUARD_ROWS, H * 64, device="cuda", dtype=torch.bfloat16)
                buf.view(torch.int16).fill_(GUARD_BITS)
                c0 = {c: ffi.counter(c) for c in COUNTERS}
                try:
                    ffi.check(L.r3g_op_attention(Q.data_ptr(), K.data_ptr(), Vt.data_ptr(), buf.data_ptr(), B, H, Lq, lqp, Lk, lkp, shared, dma,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
                    torch.cuda.synchronize()
                except Exception as e:
                    if getattr(e, "code", None) == -1:       # R3G_ERR_INVALID: the launch was refused, nothing ran -- an ordinary failure
                        raise
                    pytest.exit("%s, %s: %r" % (name, shape[:5], e), returncode=3)   # a HIP error: nothing more is started on this device
                moved = {c: ffi.counter(c) - c0[c] for c in COUNTERS}
                if moved != {c: (1 if c in moves else 0) for c in COUNTERS}:
                    failures.append("%s: launch counters moved %s, expected %s" % (shape[:5], {c: v for c, v in moved.items() if v}, moves))
                if not bool((buf[B * Lq:].view(torch.int16) == GUARD_BITS).all()):
                    failures.append("%s: rows past Lq were written" % (shape[:5],))
                outs.append(buf[:B * Lq].view(B, Lq, H * 64))
            r = max(EB.worst_ratio(o, ref, bound) for o in outs)
            worst = max(worst, r)
            if not r <= 1.0:
                d = torch.stack([(o.double() - ref).abs() / bound for o in outs]).amax(0)
                d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
                i = int(d.argmax())
                failures.append("%s: error / bound %.3f at batch %d query %d column %d, %d of %d elements outside" % (
                    shape[:5], r, i // (Lq * H * 64), i // (H * 64) % Lq, i % (H * 64), int((d > 1.0).sum()), d.numel()))
            for o in outs[1:]:
                if not torch.equal(outs[0].view(torch.int16), o.view(torch.int16)):
                    failures.append("%s: the result depends on the junk in the padded rows (%d elements differ)" % (
                        shape[:5], int((outs[0].view(torch.int16) != o.view(torch.int16)).sum())))
            if Lk == 1:
                want = ops["v"].to(torch.bfloat16).expand(B, -1, -1, -1)[:, :, 0].reshape(B, 1, H * 64).expand(-1, Lq, -1)
                if not torch.equal(outs[0].view(torch.int16), want.contiguous().view(torch.int16)):
                    failures.append("%s: one key, but the output is not v[0] to the bit" % (shape[:5],))
    report("attention edges %s (error / bound)" % name, worst, 1.0)
    print("%s: worst error / bound %.6f" % (name, worst))
    assert not failures, "%d findings, the first: %s" % (len(failures), "\n".join(failures[:12]))
