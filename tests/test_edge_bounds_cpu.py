"""The element-wise bounds of tests/edge_bounds.py are neither vacuous nor unreachable -- shown without a GPU.

REACHABLE: an "ideal kernel" written here in float32 torch (accumulation in 32-wide k blocks, last block first -- another order than
the float64 reference's --, the epilogue in float32, round-to-nearest-even to the output type; attention with P rounded to bf16)
stays inside the bound at EVERY element of every shape of the GPU lists.  The largest error / bound ratio is printed.
NOT VACUOUS: each mutant below, applied to the ideal kernel, breaks the bound at at least one element at every shape where it applies.

Where a mutant applies, and what is out of reach:
  * row_clamp needs M >= 2, bias_off4 needs N > 4 (at N = 4 "four columns off" is the same column), resid_after_store the
    read-modify-write epilogues (3, 6, 8), truncate a 16-bit output (0, 1, 2, 6, 8).
  * truncate under the packed-fp16 GELU's bound: that form's own error, 1e-3 |x|, is a quarter of a bf16 ulp at |x| ~ 1, so an element
    shows a truncation only when it cuts off more than ~0.8 ulp -- one element in four or five.  It is asserted against the fp32 forms'
    bound ("gelu_pk" 0, which the GPU test runs as well) at every shape, and against the packed form's from 256 outputs on; a truncating
    packed-GELU epilogue on the four-element shape alone is out of reach of any bound that admits the form's stated error.
  * the 4-element shape (1, 4, 64): an element shows a truncation with probability about one half, so whether ONE operand set of four
    outputs shows it in every 16-bit epilogue is a property of the draw, not of the bound.  For shapes with fewer than 64 outputs the
    truncate mutant is therefore held against the bound over 16 independent operand sets of the shape (edge_bounds.gemm_operands' draw):
    the ideal kernel is inside the bound in all of them, the mutant outside in at least one.  Every other mutant is visible in draw 0.
  * attention, no_swap (the two middle 4-key blocks of a 16-key group not swapped) needs Lk > 4: with fewer keys no valid key sits in
    a swapped block.  unmasked_pad and sum_over_pad need a padded key (Lk % 64 != 0).  A junk key's score has the sign of -+7 sum(q), so
    for a single query a +-7 fill can hide it below the maximum; the +-1e4 fills of opposite sign cannot both.  A mutant counts as
    visible when one of the junk fills shows it -- the GPU test runs every fill and applies the bound to each.
"""
import pytest
import torch

import edge_bounds as EB


def test_the_relative_bf16_unit_is_2_to_the_minus_8():
    """bf16 has an 8-bit significand: round-to-nearest errs by up to 2^-8 |x| (a tie just above a power of two), never by more than
    half_ulp, and half_ulp <= 2^-8 |x|.  A relative 2^-9 is not met by exact rounding."""
    x = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)
    err = (x.float().to(torch.bfloat16).double() - x).abs()
    assert float(err) == 2.0 ** -8 and float(err) > 2.0 ** -9 * float(x)
    g = torch.Generator().manual_seed(0)
    v = (torch.randn(1 << 16, generator=g) * 4).double()
    for fmt in ("bf16", "f16"):
        e = (v.float().to(EB.TORCH_DTYPE[fmt]).double() - v).abs()
        h = EB.half_ulp(v, fmt)
        assert bool((e <= h).all()) and float((e / h).max()) > 0.99           # met, and met tightly
        assert bool((h <= 2.0 ** -(8 if fmt == "bf16" else 11) * v.abs()).all())


def test_vt_positions_are_the_layout_modules():
    from r3g import layout
    for n in (1, 5, 16, 17, 64, 129, 192):
        assert torch.equal(EB.vt_positions(n), layout.vt_key_positions(n, "cpu").cpu())


# ---- GEMM -----------------------------------------------------------------------------------------------------------------------
def _truncate(y32, fmt):
    """float32 -> 16-bit type, rounding toward zero"""
    if fmt == "bf16":
        return (y32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    h = y32.to(torch.float16)
    over = h.float().abs() > y32.abs()                      # rounded away from zero: one step back (sign-magnitude bits)
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)


def ideal_gemm(ops, epi, mutant=None):
    fmt = EB.OUT_FMT[epi]
    a, w, K = ops["a"].float(), ops["w"].float(), ops["K"]
    blocks = list(range(K // 32))
    if mutant == "drop_last_k":
        blocks = blocks[:-1]
    acc = torch.zeros(ops["M"], ops["N"])
    for kb in reversed(blocks):
        acc = acc + a[:, kb * 32:kb * 32 + 32] @ w[:, kb * 32:kb * 32 + 32].t()
    bias = torch.roll(ops["bias"], -4) if mutant == "bias_off4" else ops["bias"]
    x = acc + bias
    rnd = (lambda y: _truncate(y, fmt)) if (mutant == "truncate" and fmt != "f32") else (lambda y: y.to(EB.TORCH_DTYPE[fmt]))
    if epi in (0, 4):
        out = rnd(x)
    elif epi in (1, 2):
        out = rnd(EB.gelu64(x.double(), epi == 1).float())
    else:
        d = ops["gate"] * x
        old = ops["c0"][fmt].float()
        if mutant == "resid_after_store":
            old = rnd(old + d).float()                      # the old values read back after the new ones were stored
        out = rnd(old + d)
    out = out.clone()
    if mutant == "swap":
        out[-1, -1], out[-1, -2] = out[-1, -2].clone(), out[-1, -1].clone()
    if mutant == "row_clamp":
        out[-1] = out[-2]
    return out


GEMM_MUTANTS = ("swap", "drop_last_k", "truncate", "row_clamp", "bias_off4", "resid_after_store")


def _applies(mutant, M, N, epi):
    return {"swap": True, "drop_last_k": True, "truncate": EB.OUT_FMT[epi] != "f32", "row_clamp": M >= 2, "bias_off4": N > 4,
            "resid_after_store": epi in (3, 6, 8)}[mutant]


@pytest.fixture(scope="module")
def gemm_cases():
    out = []
    for M, N, K, _ in EB.GEMM_SHAPES:
        ops = EB.gemm_operands(M, N, K)
        out.append((ops, EB.gemm_lin(ops)))
    return out


@pytest.mark.parametrize("epi", EB.GEMM_EPILOGUES)
def test_gemm_ideal_kernel_is_inside_the_bound_everywhere(gemm_cases, epi):
    worst = 0.0
    for ops, lte in gemm_cases:
        got = ideal_gemm(ops, epi)
        for pk in ((True, False) if epi in (1, 2) else (True,)):
            ref, bound = EB.gemm_ref_bound(ops, epi, gelu_pk=pk, lin_t_e=lte)
            r = EB.worst_ratio(got, ref, bound)
            worst = max(worst, r)
            assert r <= 1.0, "epilogue %d at %s (gelu_pk %d): error / bound %.3f" % (epi, (ops["M"], ops["N"], ops["K"]), pk, r)
    print("epilogue %d: largest error / bound of the ideal kernel %.3f" % (epi, worst))
    assert worst > (0.5 if EB.OUT_FMT[epi] != "f32" else 1e-3)       # the 16-bit bounds are met tightly: a rounding tie is near


@pytest.mark.parametrize("mutant", GEMM_MUTANTS)
def test_gemm_mutants_break_the_bound(gemm_cases, mutant):
    ran = 0
    for ops, lte in gemm_cases:
        M, N, K = ops["M"], ops["N"], ops["K"]
        for epi in EB.GEMM_EPILOGUES:
            if not _applies(mutant, M, N, epi):
                continue
            got = ideal_gemm(ops, epi, mutant)
            forms = (True, False) if epi in (1, 2) else (True,)
            if mutant == "truncate" and epi in (1, 2) and M * N < 256:
                forms = (False,)                               # module docstring: out of reach of the packed form's bound there
            for pk in forms:
                ref, bound = EB.gemm_ref_bound(ops, epi, gelu_pk=pk, lin_t_e=lte)
                r = EB.worst_ratio(got, ref, bound)
                if mutant == "truncate" and M * N < 64:        # module docstring: pooled over 16 operand sets of the shape
                    for draw in range(1, 16):
                        o2 = EB.gemm_operands(M, N, K, draw=draw)
                        ref2, bound2 = EB.gemm_ref_bound(o2, epi, gelu_pk=pk)
                        assert EB.worst_ratio(ideal_gemm(o2, epi), ref2, bound2) <= 1.0
                        r = max(r, EB.worst_ratio(ideal_gemm(o2, epi, mutant), ref2, bound2))
                assert r > 1.0, "%s is invisible at %s, epilogue %d (gelu_pk %d): error / bound %.3f" % (mutant, (M, N, K), epi, pk, r)
                ran += 1
    assert ran >= len(EB.GEMM_SHAPES)


def test_gemm_plan_reaches_every_kernel_at_ragged_shapes_and_at_its_smallest_k():
    """the selection rule restated in edge_bounds.gemm_expected_kernel (which the GPU test holds against the launch counters) reaches
    every tile kernel with an M tail, an N tail and at its smallest K over the fixed shape list -- and the silent reroutes are in it"""
    reached = set()
    for waves in EB.GEMM_WAVES:
        cu = EB.gemm_switches(waves).get("gemm_num_cu", 256)
        for M, N, K, _ in EB.GEMM_SHAPES:
            for epi in EB.GEMM_EPILOGUES:
                reached.add((EB.gemm_expected_kernel(waves, M, N, K, epi, cu), M, N, K))
    assert EB.gemm_coverage(reached) == []
    assert EB.gemm_expected_kernel(11, 127, 252, 192, 0) == "gemm_w8_128"            # K % 128 != 0
    assert EB.gemm_expected_kernel(12, 129, 132, 128, 0, 2) == "gemm_phased"          # K < 256
    assert EB.gemm_expected_kernel(13, 257, 260, 256, 6) == "gemm_phased"             # K < 512, N % 256 != 0
    assert EB.gemm_expected_kernel(13, 257, 512, 512, 1) == "gemm_phased"             # a GELU epilogue has no split-K form
    assert EB.gemm_expected_kernel(13, 257, 512, 512, 8) == "gemm_splitk2"


# ---- attention ------------------------------------------------------------------------------------------------------------------
def ideal_attention(ops, prescaled, mutant=None, fill=EB.JUNK_FILLS[0]):
    B, H, Lq, Lk = ops["B"], ops["H"], ops["Lq"], ops["Lk"]
    Q, K, Vt, lqp, lkp = EB.attn_padded(ops, *fill)
    q = Q[:, :, :Lq].float()
    sc = torch.tensor(EB.SM_SCALE32, dtype=torch.float32)
    if prescaled:
        q, sc = (q * sc).to(torch.bfloat16).float(), torch.tensor(1.0)
    k = K.float().expand(B, -1, -1, -1)
    s = torch.zeros(B, H, Lq, lkp)
    for db in (1, 0):                                          # 32-wide blocks of the head dimension, last first
        s = s + q[..., db * 32:db * 32 + 32] @ k[..., db * 32:db * 32 + 32].transpose(-1, -2)
    s = s * sc
    masked = torch.arange(lkp) >= Lk
    if mutant == "unmasked_pad":
        masked[Lk] = False
    sm = s.masked_fill(masked, float("-inf"))
    m = sm.max(-1, keepdim=True).values
    p = torch.exp2(sm - m)
    l = p.sum(-1, keepdim=True)
    if mutant == "sum_over_pad":
        l = torch.exp2(s - m).sum(-1, keepdim=True)            # the sum runs over Lk_pad: the junk keys' exponentials are in it
    pos = torch.arange(lkp) if mutant == "no_swap" else EB.vt_positions(lkp)
    v = Vt.float().expand(B, -1, -1, -1)[..., pos].transpose(-1, -2)         # row j = what the kernel multiplies p_j with
    pb = p.to(torch.bfloat16).float()
    o = torch.zeros(B, H, Lq, 64)
    for j0 in reversed(range(0, lkp, 16)):
        o = o + pb[..., j0:j0 + 16] @ v[..., j0:j0 + 16, :]
    return (o / l).to(torch.bfloat16).permute(0, 2, 1, 3).reshape(B, Lq, H * 64)


ATTN_MUTANTS = ("unmasked_pad", "no_swap", "sum_over_pad")


@pytest.fixture(scope="module")
def attn_cases():
    out = []
    for B, H, Lq, Lk, shared, _ in EB.ATTN_SHAPES:
        ops = EB.attn_operands(B, H, Lq, Lk, shared)
        out.append((ops, {pre: EB.attn_ref_bound(ops, pre) for pre in (True, False)}))
    return out


@pytest.mark.parametrize("prescaled", [True, False])
def test_attention_ideal_kernel_is_inside_the_bound_everywhere(attn_cases, prescaled):
    worst = 0.0
    for ops, rb in attn_cases:
        ref, bound = rb[prescaled]
        outs = [ideal_attention(ops, prescaled, fill=f) for f in EB.JUNK_FILLS]
        assert all(torch.equal(outs[0], o) for o in outs[1:])   # the junk in the padded rows decides nothing
        r = EB.worst_ratio(outs[0], ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, "%s: error / bound %.3f" % ((ops["B"], ops["H"], ops["Lq"], ops["Lk"]), r)
        if ops["Lk"] == 1:
            want = ops["v"].to(torch.bfloat16).expand(ops["B"], -1, -1, -1)[:, :, 0]          # [B][H][64]
            assert torch.equal(outs[0], want.reshape(ops["B"], 1, -1).expand(-1, ops["Lq"], -1))
    print("attention (Q re-rounded: %s): largest error / bound of the ideal kernel %.3f" % (prescaled, worst))
    assert worst > 0.3


@pytest.mark.parametrize("mutant", ATTN_MUTANTS)
def test_attention_mutants_break_the_bound(attn_cases, mutant):
    ran = 0
    for ops, rb in attn_cases:
        Lk = ops["Lk"]
        if (mutant == "no_swap" and Lk <= 4) or (mutant != "no_swap" and Lk % 64 == 0):
            continue
        for prescaled in (True, False):
            ref, bound = rb[prescaled]
            # (a junk key's score has the sign of -+7 sum(q): the GPU test runs both fills, and one of them shows the key)
            r = max(EB.worst_ratio(ideal_attention(ops, prescaled, mutant, fill=f), ref, bound) for f in EB.JUNK_FILLS)
            assert r > 1.0, "%s is invisible at %s: error / bound %.3f" % (mutant, (ops["B"], ops["H"], ops["Lq"], Lk), r)
            ran += 1
    assert ran >= 8
