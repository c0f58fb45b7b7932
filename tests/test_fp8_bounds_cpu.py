"""The checks of tests/fp8_bounds.py are neither vacuous nor unreachable -- shown without a GPU.

REACHABLE: a float32 emulation of gemm8f_kernel written here (the decoded codes multiplied in float32 in 128-wide k blocks, last block
first -- another order than the float64 reference's --, then fl(sw * sa), the product with the accumulator, the bias and the epilogue as
the kernel writes them, round-to-nearest-even to the output type) stays inside the bound at EVERY element of every shape, operand set,
epilogue and layout of the GPU test, matches the exact operand set bit for bit where the GPU test asks for bits, and leaves the guards
alone.  That also shows that the reference alone stays inside its own tolerance.  The largest error / bound is printed.
NOT VACUOUS: each mutant below, applied to the emulation, is reported by fp8_bounds.verdict -- the function the GPU test calls -- at every
shape where it is live, by BOTH operand sets unless stated:
    drop_k            the last 128-byte k-block of both operands is not accumulated
    scale_a_prev      row m is scaled by scale_a[m - 1] (row 0 keeps its own); live for M >= 2
    scale_w_rot       scale_w rotated by one inside every group of four columns
    scale_after_bias  (acc + bias) * s instead of acc * s + bias
    truncate          the e4m3 conversion of epilogue 7 rounds toward zero.  An element shows it with probability about one half, so the
                      four-element shape is held against the bound over up to 16 independent draws (edge_bounds' device): the
                      emulation is inside in all of them, the mutant outside in at least one.
    out_scale         epilogue 7 multiplies by out_scale instead of its inverse
    row_clamp_store   row M - 1 is stored a second time into row M: caught by the guard rows, not by the bound
    resid_after_store epilogues 3 and 6 read the old values after the new ones were stored
The quantiser restatement is checked against the decoder of tests/test_fp8_gpu.py, the e4m3 table of tests/row_bounds.py, and the rule
include/r3g.h states; the row with amax = 2^-130 has no NaN code under the floored scale and has them without the floor.
"""
import pytest
import torch

import edge_bounds as EB
import fp8_bounds as FB
import row_bounds as RB

MUTANTS = ("drop_k", "scale_a_prev", "scale_w_rot", "scale_after_bias", "truncate", "out_scale", "row_clamp_store", "resid_after_store")


def emulate(ops, epi, layout, mutant=None):
    """the guarded C after a float32 restatement of one launch: (flat, C, off)"""
    M, N, K = ops["M"], ops["N"], ops["K"]
    A, W = FB.e4m3_decode(ops["a8"]).float(), FB.e4m3_decode(ops["w8"]).float()
    blocks = list(range(K // 128))
    if mutant == "drop_k":
        blocks = blocks[:-1]
    acc = torch.zeros(M, N)
    for kb in reversed(blocks):
        acc = acc + A[:, kb * 128:kb * 128 + 128] @ W[:, kb * 128:kb * 128 + 128].t()
    sa, sw = ops["sa"], ops["sw"]
    if mutant == "scale_a_prev":
        sa = torch.cat([sa[:1], sa[:-1]])
    if mutant == "scale_w_rot":
        sw = sw.view(-1, 4).roll(1, dims=1).reshape(-1)
    s = sw[None, :] * sa[:, None]
    x = (acc + ops["bias"]) * s if mutant == "scale_after_bias" else acc * s + ops["bias"]
    fmt = FB.OUT_FMT[epi]
    rnd = lambda y: y.to(FB.TORCH_DTYPE[fmt])
    if epi == 0:
        out = rnd(x)
    elif epi in (1, 2):
        out = rnd(EB.gelu64(x.double(), epi == 1).float())
    elif epi == 7:
        q = torch.tensor(FB.OUT_SCALE, dtype=torch.float32)
        inv = q if mutant == "out_scale" else 1.0 / q
        out = FB.e4m3_encode(EB.gelu64(x.double(), False).float() * inv, truncate=mutant == "truncate")
    else:
        d = ops["gate"] * x
        old = ops["c0"][fmt].float()
        if mutant == "resid_after_store":
            old = rnd(old + d).float()
        out = rnd(old + d)
    flat, C, ldc, off = FB.c_buffer(ops, epi, layout)
    C[:M, :N] = out
    if mutant == "row_clamp_store":
        C[M, :N] = out[M - 1]
    return flat, C, off


def _live(mutant, M, epi):
    return {"scale_a_prev": M >= 2, "truncate": epi == 7, "out_scale": epi == 7, "resid_after_store": epi in (3, 6)}.get(mutant, True)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for M, N, K, _ in FB.GEMM_SHAPES:
        for kind in FB.KINDS:
            ops = FB.gemm_operands(M, N, K, kind)
            lte = FB.gemm_lin(ops)
            out[(M, N, K, kind)] = (ops, {epi: FB.gemm_ref_bound(ops, epi, lte) for epi in FB.GEMM_EPILOGUES})
    return out


def test_e4m3_encode_inverts_the_table_and_rounds_ties_to_even():
    codes = torch.arange(256, dtype=torch.uint8)
    finite = (codes & 127) != 127
    vals = FB.e4m3_decode(codes).float()
    assert torch.equal(FB.e4m3_encode(vals)[finite], codes[finite])
    assert int(FB.e4m3_encode(torch.tensor([float("nan")]))[0]) & 127 == 127
    pos = RB.E4M3[:127]
    mid = (0.5 * (pos[:-1] + pos[1:])).float()
    up = FB.e4m3_encode(mid).long()
    assert bool((up % 2 == 0).all()) and bool(((up - torch.arange(126)) >= 0).all()) and bool(((up - torch.arange(126)) <= 1).all())
    assert torch.equal(FB.e4m3_encode(mid, truncate=True).long(), torch.arange(126))
    big = torch.tensor([448.0, 449.0, 1e30, -500.0])
    assert FB.e4m3_encode(big).tolist() == [126, 126, 126, 254]                   # saturating, never the NaN code
    assert FB.e4m3_encode(torch.tensor([2.0 ** -10, 2.0 ** -10 * 1.001, -2.0 ** -11])).tolist() == [0, 1, 128]


def test_exact_codes_are_the_integers():
    ops = FB.gemm_operands(17, 68, 256, "exact")
    v = FB.e4m3_decode(ops["a8"])
    assert torch.equal(v, v.round()) and float(v.abs().max()) == 4.0 and float(v.min()) == -4.0
    assert len(set(ops["sa"].tolist())) == 3 and len(set(ops["sw"].tolist())) == 3


def test_quantiser_restatement_against_the_independent_decoder():
    from test_fp8_gpu import _e4m3_to_float
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(37, 1024, generator=g) * torch.logspace(-3, 2, 37)[:, None]).to(torch.bfloat16)
    x[5] = 0
    q, sc = FB.quant_ref(x)
    amax = x.float().abs().amax(1)
    assert torch.equal(sc, torch.where(amax > 0, amax * torch.tensor(FB.INV448), torch.ones_like(amax)))   # far above the floor
    dec = _e4m3_to_float(torch, q)
    assert torch.equal(dec.double(), FB.e4m3_decode(q))
    y = x.double() / sc.double()[:, None]
    err = (dec.double() - y).abs()
    # half an e4m3 step of the scaled value, plus the two float32 roundings (1 / sc, x * inv) in front of the conversion
    assert bool((err <= RB.e4m3_half_ulp(y) + RB.g(2) * y.abs()).all())
    assert float(dec.abs().max()) == 448.0 and float(dec[5].abs().max()) == 0.0


def test_quantiser_cases_hold_every_row_kind_and_a_finite_row_has_no_nan_code():
    seen = set()
    for rows in FB.QUANT_ROWS:
        for K in FB.QUANT_K:
            case = FB.quant_case(rows, K)
            seen |= set(case["kinds"])
            x = case["x"]
            q, sc = FB.quant_ref(x)
            assert bool(torch.isfinite(x.float()).all())
            assert bool(((q & 127) != 127).all()), (rows, K)
            assert bool(torch.isfinite(sc).all()) and bool((sc >= FB.FLOOR).all()) and bool(torch.isfinite(1.0 / sc).all())
            y = x.double() / sc.double()[:, None]
            assert bool(((FB.e4m3_decode(q) - y).abs() <= RB.e4m3_half_ulp(y) + RB.g(2) * y.abs()).all()), (rows, K)
            for r, kind in enumerate(case["kinds"]):
                if kind == "zero":
                    assert float(sc[r]) == 1.0 and int(q[r].max()) == 0
                if kind == "tiny":      # 2^-130 * 2^126 = 2^-4: code 0x18 (2^-5: 0x10, -2^-7: 0x84); the zeros stay zeros
                    assert float(sc[r]) == FB.FLOOR and set(q[r].tolist()) <= {0x18, 0x98, 0x10, 0x84, 0x00}
                    nz = x[r].float() != 0
                    assert bool((q[r][~nz] == 0).all()) and bool((q[r][nz] & 127 != 0).all())
                if kind in ("sat", "ties"):
                    e = 3 if kind == "sat" else -7
                    assert float(sc[r]) == 2.0 ** e and int(q[r][0]) == 0x7E and int(q[r][1]) == 0xFE
                if kind == "sat":
                    assert torch.equal(FB.e4m3_decode(q[r]) * 8.0, x[r].double())
                if kind == "ties" and K >= 126:
                    assert bool((q[r][2:] % 2 == 0).all())                   # every tie went to the even code
    assert seen == set(FB.QUANT_KINDS)
    # without the floor the tiny row is what the issue describes: 1 / sc = +inf and every zero becomes 0 * inf = NaN
    x = FB.quant_row("tiny", 16, None).float()
    sc = x.abs().amax() * torch.tensor(FB.INV448)
    assert float(1.0 / sc) == float("inf") and bool(torch.isnan(x * (1.0 / sc)).any())


def test_nonfinite_rows_as_the_header_states():
    x = FB.quant_nonfinite_case()
    q, sc = FB.quant_ref(x)
    assert bool(torch.isfinite(sc[0])) and int(q[0, 3]) & 127 == 127 and int(((q[0] & 127) == 127).sum()) == 1
    clean = x[0:1].clone()
    clean[0, 3] = 0
    qc, scc = FB.quant_ref(clean)
    keep = torch.arange(16) != 3
    assert float(scc[0]) == float(sc[0]) and torch.equal(qc[0][keep], q[0][keep])
    for r, c in ((1, 5), (2, 9)):
        assert float(sc[r]) == float("inf") and int(q[r, c]) & 127 == 127
        assert bool(((q[r][torch.arange(16) != c] & 127) == 0).all())


@pytest.mark.parametrize("epi", FB.GEMM_EPILOGUES)
def test_the_emulation_is_inside_every_bound_and_exact_where_bits_are_asked(cases, epi):
    worst = {k: 0.0 for k in FB.KINDS}
    saturated = 0
    for (M, N, K, kind), (ops, rb) in cases.items():
        ref, bound = rb[epi]
        for layout in FB.LAYOUTS:
            flat, C, off = emulate(ops, epi, layout)
            r, complaints = FB.verdict(ops, epi, flat, C, off, ref, bound)
            assert not complaints, "%s %s epilogue %d %s: %s" % ((M, N, K), kind, epi, layout, complaints)
            worst[kind] = max(worst[kind], r)
        if epi == 7:
            saturated += int((ref.abs() == 448.0).sum())
    print("epilogue %d: largest error / bound of the emulation %s" % (epi, worst))
    if epi != 3:
        assert worst["random"] > 0.5                   # a rounding tie is near: the 16-bit and e4m3 bounds are met tightly
    if epi == 7:
        assert saturated > 0                           # OUT_SCALE puts some elements past 448


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_are_reported(cases, mutant):
    ran = 0
    for (M, N, K, kind), (ops, rb) in cases.items():
        for epi in FB.GEMM_EPILOGUES:
            if not _live(mutant, M, epi):
                continue
            ref, bound = rb[epi]
            flat, C, off = emulate(ops, epi, "loose", mutant)
            r, complaints = FB.verdict(ops, epi, flat, C, off, ref, bound)
            if not complaints and mutant == "truncate" and M * N < 64:       # module docstring: pooled over further draws
                for draw in range(1, 16):
                    o2 = FB.gemm_operands(M, N, K, kind, draw=draw)
                    ref2, bound2 = FB.gemm_ref_bound(o2, epi)
                    assert not FB.verdict(o2, epi, *emulate(o2, epi, "loose"), ref2, bound2)[1]
                    complaints = FB.verdict(o2, epi, *emulate(o2, epi, "loose", mutant), ref2, bound2)[1]
                    if complaints:
                        break
            assert complaints, "%s is invisible at %s, %s operands, epilogue %d (error / bound %.3f)" % (mutant, (M, N, K), kind, epi, r)
            ran += 1
    assert ran >= len(FB.GEMM_SHAPES)



def test_contract_violations_are_refused_before_anything_touches_the_gpu():
    """r3g_op_gemm_fp8 / r3g_op_gemm_fp8_e4m3 check their whole contract on the host: every violation is R3G_ERR_INVALID here too, the
    empty problems are R3G_OK, and gemm_fp8 counts no launch.  (An admitted call is not made: it would launch.)"""
    from r3g import ffi
    L = ffi.lib()
    M, N, K = 17, 68, 256
    ops = FB.gemm_operands(M, N, K, "random")
    lda, ldw = K + FB.LDA_PAD, K + FB.LDW_PAD
    hold = dict(a=torch.zeros((M + 8) * lda, dtype=torch.uint8), w=torch.zeros((N + 8) * ldw, dtype=torch.uint8), sa=torch.zeros(M + 8),
                sw=torch.zeros(N + 8), bias=torch.zeros(N + 8), gate=torch.zeros(N + 8))
    before, ran = ffi.counter("gemm_fp8"), 0
    for epi, esz in FB.REFUSED_ENTRIES:
        flat, C, ldc, off = FB.c_buffer(ops, 7 if epi == "e4m3" else epi, "loose")
        base = C.data_ptr() - C.data_ptr() % 16 + 16 + 4 * esz          # four elements past a 16-byte boundary, as on the GPU
        args = dict({k: v.data_ptr() - v.data_ptr() % 16 + 16 for k, v in hold.items()}, lda=lda, ldw=ldw, c=base, ldc=ldc, m=M, n=N, k=K)
        if epi not in (3, 6):
            args["gate"] = None
        for what, over in FB.gemm_refusals(epi, esz, args, N, K).items():
            assert FB.gemm_abi_call(L, epi, None, dict(args, **over))() == -1, "epilogue %s, %s was not refused" % (epi, what)
            ran += 1
        for what, over in FB.ADMITTED_EMPTY:
            assert FB.gemm_abi_call(L, epi, None, dict(args, **over))() == 0, "epilogue %s, %s" % (epi, what)
    assert ran >= 4 * 27 and ffi.counter("gemm_fp8") == before


def test_the_plan_reaches_every_epilogue_at_every_edge():
    reached = set()
    for M, N, K, _ in FB.GEMM_SHAPES:
        for epi in FB.GEMM_EPILOGUES:
            for layout in FB.LAYOUTS:
                for wide in (1, 0):
                    reached.add((epi, M, N, K, FB.store_path(epi, N, layout, wide)))
    assert FB.gemm_coverage(reached) == []
    assert FB.store_path(7, 144, "wide", 1) == "wide" and FB.store_path(7, 136, "wide", 1) == "narrow" and FB.store_path(0, 136, "wide", 1) == "wide"
    assert FB.store_path(0, 136, "loose", 1) == "narrow" and FB.store_path(6, 68, "wide", 1) == "narrow" and FB.store_path(0, 256, "wide", 0) == "narrow"
    assert all(M * N <= 6 * 65536 and ((M + 255) // 256) * ((N + 255) // 256) <= 6 for M, N, K, _ in FB.GEMM_SHAPES)
