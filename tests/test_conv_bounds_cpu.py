"""The element-wise bound of tests/conv_bounds.py is neither unreachable nor vacuous -- shown without a GPU.

REACHABLE: conv_bounds.emulate -- every window gathered by plain indexing, fp32 products, fp32 accumulation per slice in k-steps of 64,
the slices added in the order 0 .. S-1, then the bias and the old value -- stays inside the bound at EVERY element of every shape of
conv_bounds.SHAPES, both epilogues, with the slices the restated rule gives (and the cin = 256 shape once more as one launch), and keeps
every bit outside [M) x [cout).  The largest error / bound is printed.

NOT VACUOUS: each mutant of conv_bounds.MUTANTS exceeds the bound (or writes outside [M) x [cout)) at every shape listed for it in
conv_bounds.LIVE, under both epilogues; at every shape NOT listed it writes the emulation's own bits, which is why that shape cannot
show it.  A mutant with an empty list fails.
"""
import pytest
import torch

import conv_bounds as CB

_CASES = {}


def case(i):
    """operands, (lin, t, E) and the slices of shape i; memoised"""
    if i not in _CASES:
        ops = CB.operands(CB.SHAPES[i])
        S = CB.splitk128_factor(ops["M"], ops["N"], ops["K"])
        _CASES[i] = (ops, CB.conv_lin(ops), S)
    return _CASES[i]


def test_restated_geometry_and_slice_rule():
    want_S = (1, 1, 1, 1, 1, 1, 1, 1, 4, 5, 9, 18)
    want_M = (1, 2, 35, 189, 24, 24, 24, 12, 70, 135, 8, 9)
    for i, shape in enumerate(CB.SHAPES):
        geo = CB.geometry(shape)
        assert geo["M"] == want_M[i], (shape, geo["M"])
        assert CB.splitk128_factor(geo["M"], geo["N"], geo["K"]) == want_S[i], shape
        assert (geo["K"] // want_S[i]) >= 512 and want_S[i] <= 2 * geo["K"] * (1 - 1 / max(want_S[i], 2))     # E covers the split launch
        assert CB.expected_implicit(1, geo["M"], geo["N"], geo["K"]) and not CB.expected_implicit(0, geo["M"], geo["N"], geo["K"])
        assert CB.expected_slices(geo["M"], geo["N"], geo["K"], 0) == 1
        assert CB.expected_slices(geo["M"], geo["N"], geo["K"], want_S[i] * geo["M"] * geo["N"]) == want_S[i]
        assert CB.expected_slices(geo["M"], geo["N"], geo["K"], want_S[i] * geo["M"] * geo["N"] - 1) == 1
    # the rule away from the table: two slices only from K = 4096, no split of a grid that half fills the chip, the 256-tile kernels' share
    assert CB.splitk128_factor(128, 128, 2048) == 4 and CB.splitk128_factor(128, 128, 1984) == 1
    assert CB.splitk128_factor(128 * 129, 128 * 2, 4608) == 1 and CB.splitk128_factor(128 * 128, 128 * 2, 4608) == 2
    assert CB.splitk128_factor(128 * 128, 128 * 2, 2304) == 1
    assert CB.auto_takes_256(8192, 1280, 11520) and not CB.auto_takes_256(8192, 1284, 11520) and not CB.auto_takes_256(4096, 1280, 11520)
    # what the shapes are for
    mid = {i for i in range(len(CB.SHAPES)) if CB.mid_tap(CB.geometry(CB.SHAPES[i])["K"], want_S[i], CB.SHAPES[i][3])}
    assert mid == {8, 9, 11}
    assert [i for i in range(len(CB.SHAPES)) if CB.crosses_sample(CB.geometry(CB.SHAPES[i]))] == [3, 4, 5, 6, 7, 8, 10]
    assert CB.SHAPES[CB.NO_WORKSPACE][3] == 256


def test_out_hw_is_conv2d_s():
    for H in range(1, 8):
        for W in (1, 2, 5):
            for stride in (1, 2):
                for pad in (0, 1):
                    if H + pad < 2 or W + pad < 2:
                        continue
                    x = torch.zeros(1, 1, H, W, dtype=torch.float64)
                    if pad == 0:
                        x = torch.nn.functional.pad(x, (0, 1, 0, 1))
                    y = torch.nn.functional.conv2d(x, torch.zeros(1, 1, 3, 3, dtype=torch.float64), stride=stride, padding=pad)
                    assert tuple(y.shape[2:]) == CB.out_hw(H, W, stride, pad), (H, W, stride, pad)


def test_emulation_is_inside_the_bound_everywhere():
    worst = {}
    for i in range(len(CB.SHAPES)):
        ops, lte, S = case(i)
        for slices in ((S, 1) if i == CB.NO_WORKSPACE else (S,)):
            for epi in CB.EPILOGUES:
                ref, bound = CB.ref_bound(ops, epi, lte)
                assert bool((bound > 0).all())
                flat, C = CB.emulate(ops, epi, slices)
                r, complaints = CB.verdict(ops, flat, C, ref, bound)
                assert not complaints, "%s epilogue %d S %d: %s" % (CB.SHAPES[i][:7], epi, slices, complaints)
                worst[(i, slices, epi)] = r
    top = max(worst, key=worst.get)
    print("fp32 emulation: worst error / bound %.4f at %s" % (worst[top], top))
    assert 0.0 < worst[top] <= 1.0


@pytest.mark.parametrize("mutant", CB.MUTANTS)
def test_mutant_exceeds_the_bound_where_it_is_live(mutant):
    live = CB.LIVE[mutant]
    assert live, "no shape shows " + mutant
    for i in range(len(CB.SHAPES)):
        ops, lte, S = case(i)
        for epi in CB.EPILOGUES:
            ref, bound = CB.ref_bound(ops, epi, lte)
            flat, C = CB.emulate(ops, epi, S, mutant)
            if i in live:
                r, _ = CB.verdict(ops, flat, C, ref, bound)
                assert r > 1.0, "%s at %s epilogue %d: error / bound %.4g, inside the bound" % (mutant, CB.SHAPES[i][:7], epi, r)
            else:
                ideal, _ = CB.emulate(ops, epi, S)
                assert torch.equal(flat.view(torch.int32), ideal.view(torch.int32)), "%s is live at %s" % (mutant, CB.SHAPES[i][:7])
