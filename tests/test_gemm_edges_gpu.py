"""Every GEMM tile kernel (gemm_waves 0, 4, 8, 9, 10, 11, 12, 13, 16, 32 x LDS-DMA / register staging, and the narrow epilogues of
0, 8, 11) at the shapes where its edge logic is live, through r3g_op_gemm alone.

Per launch:
  * the ELEMENT-WISE bound of tests/edge_bounds.py at every element of C (derived there; tests/test_edge_bounds_cpu.py shows that a
    correctly rounding kernel meets it and that a swapped element, a dropped k-block, a truncating store, a wrong row clamp, a
    shifted bias and a read-after-store of the residual do not);
  * C sits in a larger buffer -- four or eight elements in front of it, ldc = N + 4 or N + 8, eight rows past M -- filled with a NaN
    bit pattern: every element outside [M) x [N) keeps its bits, and an element inside that was never stored is a NaN;
  * the launch counters say which kernel ran, and it is the one edge_bounds.gemm_expected_kernel (launch_epi restated, the silent
    reroutes included) names: a switch that fell back to the default kernel cannot pass for the kernel it asked for.
Two layouts of C per launch: "loose", the loosest alignment include/r3g.h admits (C four elements into the buffer, ldc = N + 4: the
16-bit outputs can only take their 8-byte stores), and "wide" (eight elements, ldc = N + 8: with N % 8 == 0 the LDS-transposed
16-byte stores).  The GELU epilogues run under "gelu_pk" 1 and 0, each against its own form term.
The closing test asserts that every launch counter was reached with an M tail, an N tail (not split-K: it needs N % 256 == 0) and at
the kernel's smallest admitted K.  gemm_waves 12 runs with gemm_num_cu = 2, so that a workgroup of the four-tile shapes walks two tiles.
"""
import ctypes

import pytest

import edge_bounds as EB
from parity_support import report
from switch_table import switched

pytestmark = pytest.mark.gpu

LAYOUTS = (("loose", 4), ("wide", 8))          # (name, elements in front of C = columns between N and ldc)
GUARD_ROWS = 8
GUARD_BITS = {"bf16": 0x7FA5, "f16": 0x7EA5, "f32": 0x7FA5A5A5}      # quiet NaNs with a recognisable payload
COUNTERS = EB.GEMM_COUNTERS + ("gemm_register_staged",)
CONFIGS = [(w, dma, 1) for w in EB.GEMM_WAVES for dma in (1, 0)] + [(w, 1, 0) for w in (0, 8, 11)]

_SHAPES, _REFS, _RESULTS = {}, {}, {}


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    ffi.context(0)
    return torch, ffi.lib(), ffi


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _shape(M, N, K):
    if (M, N, K) not in _SHAPES:
        ops = EB.gemm_operands(M, N, K, "cuda")
        _SHAPES[(M, N, K)] = (ops, EB.gemm_lin(ops))
    return _SHAPES[(M, N, K)]


def _ref(M, N, K, epi, pk):
    key = (M, N, K, epi, pk)
    if key not in _REFS:
        ops, lte = _shape(M, N, K)
        _REFS[key] = EB.gemm_ref_bound(ops, epi, gelu_pk=bool(pk), lin_t_e=lte)
    return _REFS[key]


def _int_view(torch, t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _guarded(torch, ops, epi, off):
    """(flat buffer, C view [M + 8][ldc], ldc): the guard pattern everywhere, the old values inside for the residual epilogues"""
    fmt = EB.OUT_FMT[epi]
    M, N = ops["M"], ops["N"]
    ldc = N + off
    flat = torch.empty(off + (M + GUARD_ROWS) * ldc, device="cuda", dtype=EB.TORCH_DTYPE[fmt])
    bits = GUARD_BITS[fmt]
    _int_view(torch, flat).fill_(bits if fmt == "f32" or bits < 0x8000 else bits - 0x10000)
    C = flat[off:].view(M + GUARD_ROWS, ldc)
    if epi in (3, 6, 8):
        C[:M, :N] = ops["c0"][fmt]
    return flat, C, ldc


def _launch(torch, L, ops, C, ldc, epi, dma):
    return L.r3g_op_gemm(ops["a"].data_ptr(), ops["K"], ops["w"].data_ptr(), ops["K"], ops["bias"].data_ptr(), C.data_ptr(), ldc,
                         ops["gate"].data_ptr() if epi in (3, 6, 8) else None, ops["M"], ops["N"], ops["K"], epi, dma, _stream(torch))


def run_config(env, waves, dma, wide):
    """all shapes x epilogues x layouts of one kernel configuration; memoised (the closing test reads the results of the others)"""
    key = (waves, dma, wide)
    if key in _RESULTS:
        return _RESULTS[key]
    torch, L, ffi = env
    res = dict(worst={}, reached=set(), failures=[], launches=0)
    switches = dict(gemm_waves=waves, **EB.gemm_switches(waves))
    if not wide:
        switches["gemm_wide_epilogue"] = 0
    num_cu = switches.get("gemm_num_cu", 256)
    with switched(L, ffi, **switches):
        for M, N, K, _ in EB.GEMM_SHAPES:
            ops, _lte = _shape(M, N, K)
            for epi in EB.GEMM_EPILOGUES:
                want = EB.gemm_expected_kernel(waves, M, N, K, epi, num_cu)
                for pk in ((1, 0) if epi in (1, 2) else (1,)):
                    ref, bound = _ref(M, N, K, epi, pk)
                    for lname, off in LAYOUTS:
                        tag = "%s epilogue %d gelu_pk %d %s" % ((M, N, K), epi, pk, lname)
                        flat, C, ldc = _guarded(torch, ops, epi, off)
                        before = _int_view(torch, flat).clone()
                        c0 = {c: ffi.counter(c) for c in COUNTERS}
                        try:
                            with switched(L, ffi, gelu_pk=pk):
                                ffi.check(_launch(torch, L, ops, C, ldc, epi, dma))
                            torch.cuda.synchronize()
                        except Exception as e:
                            if getattr(e, "code", None) == -1:   # R3G_ERR_INVALID: the launch was refused, nothing ran -- an ordinary failure
                                raise
                            # a HIP error: nothing more is started on this device
                            pytest.exit("gemm_waves %d, lds_dma %d, wide %d, %s: %r" % (waves, dma, wide, tag, e), returncode=3)
                        res["launches"] += 1
                        moved = {c: ffi.counter(c) - c0[c] for c in COUNTERS}
                        expect = {c: 0 for c in COUNTERS}
                        expect[want] = 1
                        expect["gemm_register_staged"] = 1 if (dma == 0 and want in EB.REGISTER_STAGED) else 0
                        if moved != expect:
                            res["failures"].append("%s: launch counters moved %s, expected %s" % (
                                tag, {c: v for c, v in moved.items() if v}, {c: v for c, v in expect.items() if v}))
                        for c, v in moved.items():
                            if v:
                                res["reached"].add((c, M, N, K))
                        r = EB.worst_ratio(C[:M, :N], ref, bound)
                        res["worst"][epi] = max(res["worst"].get(epi, 0.0), r)
                        if not r <= 1.0:
                            d = ((C[:M, :N].double() - ref).abs() / bound)
                            d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
                            i = int(d.argmax())
                            res["failures"].append("%s: error / bound %.3f at (%d, %d), %d of %d elements outside" % (
                                tag, r, i // N, i % N, int((d > 1.0).sum()), M * N))
                        after = _int_view(torch, flat).clone()
                        for t in (before, after):
                            t[off:].view(M + GUARD_ROWS, ldc)[:M, :N] = 0
                        if not torch.equal(before, after):
                            bad = (before != after).nonzero().flatten()
                            j = int(bad[0]) - off
                            res["failures"].append("%s: %d elements outside [M) x [N) were written, the first at row %d column %d" % (
                                tag, bad.numel(), j // ldc, j % ldc))
    for epi, r in sorted(res["worst"].items()):
        report("gemm edges waves=%d dma=%d wide=%d epilogue %d (error / bound)" % (waves, dma, wide, epi), r, 1.0)
    _RESULTS[key] = res
    return res


@pytest.mark.parametrize("waves,dma,wide", CONFIGS, ids=["waves%d-%s-%s" % (w, "dma" if d else "reg", "wide" if e else "narrow") for w, d, e in CONFIGS])
def test_gemm_edges(env, waves, dma, wide):
    res = run_config(env, waves, dma, wide)
    print("gemm_waves %d, lds_dma %d, wide epilogue %d: %d launches, worst error / bound per epilogue %s" % (
        waves, dma, wide, res["launches"], {e: round(r, 6) for e, r in sorted(res["worst"].items())}))
    assert not res["failures"], "%d findings, the first: %s" % (len(res["failures"]), "\n".join(res["failures"][:12]))


def test_every_gemm_kernel_was_reached_at_ragged_shapes_and_its_smallest_k(env):
    """Reads what the tests above recorded from the launch counters.  A configuration that has not run yet in this session (the test
    selected alone) is run here: 162 launches of at most 512 x 512 x 512 with their checks take about 30 ms each configuration on an
    MI355X, the whole file about two seconds."""
    reached = set()
    for cfg in CONFIGS:
        reached |= run_config(env, *cfg)["reached"]
    assert EB.gemm_coverage(reached) == []
    staged = [(M, N, K) for c, M, N, K in reached if c == "gemm_register_staged"]
    assert any(M % 256 and N % 256 and K == 64 for M, N, K in staged)
    for line in sorted("%s: %s" % (k, sorted((M, N, K) for c, M, N, K in reached if c == k)) for k in COUNTERS):
        print(line)


def test_gemm_refused_epilogues_and_the_store_contract(env):
    """Epilogues 7 and 9-11 are refused (they need operands r3g_op_gemm cannot carry), and so is every C the narrow stores cannot
    take: ldc % 4 != 0, a C that is not aligned to four elements, ldc < n; nothing is written by a refused call."""
    torch, L, ffi = env
    M, N, K = 17, 68, 64
    ops, _ = _shape(M, N, K)
    for epi in EB.GEMM_REFUSED:
        flat, C, ldc = _guarded(torch, ops, 0, 4)
        before = _int_view(torch, flat).clone()
        assert _launch(torch, L, ops, C, ldc, epi, 1) != 0, "epilogue %d was accepted" % epi
        torch.cuda.synchronize()
        assert torch.equal(before, _int_view(torch, flat))
    for epi in (0, 4, 8):
        esz = 4 if epi == 4 else 2
        flat, C, ldc = _guarded(torch, ops, epi, 4)
        before = _int_view(torch, flat).clone()
        call = lambda ptr, ld: L.r3g_op_gemm(ops["a"].data_ptr(), K, ops["w"].data_ptr(), K, ops["bias"].data_ptr(), ptr, ld,
                                             ops["gate"].data_ptr() if epi == 8 else None, M, N, K, epi, 1, _stream(torch))
        assert call(C.data_ptr() + 2 * esz, ldc) == -1          # two elements off: R3G_ERR_INVALID
        assert call(C.data_ptr(), ldc + 2) == -1                # ldc % 4 == 2
        assert call(C.data_ptr(), N - 4) == -1                  # ldc < n
        assert call(None, ldc) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, _int_view(torch, flat))
        ffi.check(call(C.data_ptr(), ldc))                      # ... and the loosest admitted layout is accepted
        torch.cuda.synchronize()
