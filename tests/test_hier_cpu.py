"""Hierarchical volume decoding, host side (no GPU): the level rule, the public switches (enable_flashvdm, R3G_VOLUME_DECODER,
the stage's `r3g_volume_decoder` key) and a guard on the fixtures the GPU tests rely on -- the numpy restatement of the planner
(tests/hier_ref.py) on the five analytic 257^3 fields must leave 0 missed and 0 unsafe cells."""
import importlib.util
import inspect
import os

import numpy as np
import pytest

import hier_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rule(R, min_res=63):
    out = [R]
    while out[-1] % 2 == 0 and out[-1] // 2 >= min_res:
        out.append(out[-1] // 2)
    return out[::-1]


@pytest.mark.parametrize("R,expect", [(256, [64, 128, 256]), (380, [95, 190, 380]), (512, [64, 128, 256, 512]), (257, [257]),
                                      (64, [64]), (100, [100]), (126, [63, 126])])
def test_levels(R, expect):
    from r3g import hier
    assert hier.levels(R) == expect == _rule(R) == hier_ref.levels(R)
    assert hier.levels(R, min_resolution=63) == expect
    assert hier.levels(R, 10 ** 6) == [R]


class _StubModel:
    num_latents, in_channels = 8, 4

    def __init__(self):
        self.calls = []

    def grid_query(self, bound, R):
        self.calls.append(("vanilla", bound, R))
        return "dense-grid"

    def grid_query_hier(self, bound, R, mc_level, band, min_resolution):
        self.calls.append(("hierarchical", bound, R, mc_level, band, min_resolution))
        return "hier-grid", {"levels": [R // 2, R], "evaluated_per_level": [5, 7], "evaluated": 12, "dense_points": (R + 1) ** 3,
                             "unsafe_cells": 0}


def _pipeline():
    import hy3dgen.shapegen.pipelines as pl

    class P(pl.Hunyuan3DDiTFlowMatchingPipeline):
        def _make_model(self, cfg, state_dict, grid_chunk):
            return _StubModel()
    return P(pl.builtin_config("full"), {}, "cuda:0")


def test_enable_flashvdm_signature_and_toggle(monkeypatch):
    monkeypatch.delenv("R3G_VOLUME_DECODER", raising=False)
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    sig = inspect.signature(Hunyuan3DDiTFlowMatchingPipeline.enable_flashvdm)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("enabled", True), ("adaptive_kv_selection", True), ("topk_mode", "mean"), ("mc_algo", "mc"), ("replace_vae", True)]
    p = _pipeline()
    assert p.volume_decoder == "vanilla" and p.last_hier_stats is None
    assert p._query_grid(1.01, 128, 0.0) == "dense-grid"
    assert p.model.calls[-1] == ("vanilla", 1.01, 128)
    assert p.timings["grid_points_evaluated"] == 129 ** 3 and p.last_hier_stats is None
    p.enable_flashvdm()
    assert p.volume_decoder == "hierarchical"
    assert p._query_grid(1.01, 128, 0.25) == "hier-grid"
    assert p.model.calls[-1] == ("hierarchical", 1.01, 128, 0.25, 0.95, 63)
    assert p.timings["grid_points_evaluated"] == 12 and p.last_hier_stats["levels"] == [64, 128]
    p.enable_flashvdm(adaptive_kv_selection=False, topk_mode="merge", replace_vae=False)     # accepted, ignored
    assert p.volume_decoder == "hierarchical"
    p.enable_flashvdm(False)
    assert p.volume_decoder == "vanilla"
    assert p._query_grid(1.01, 128, 0.0) == "dense-grid" and p.last_hier_stats is None
    with pytest.raises(NotImplementedError):
        p.enable_flashvdm(mc_algo="dmc")
    assert p.volume_decoder == "vanilla"


def test_environment_variable_selects_the_decoder(monkeypatch):
    monkeypatch.setenv("R3G_VOLUME_DECODER", "hierarchical")
    assert _pipeline().volume_decoder == "hierarchical"
    monkeypatch.setenv("R3G_VOLUME_DECODER", "vanilla")
    assert _pipeline().volume_decoder == "vanilla"
    monkeypatch.setenv("R3G_VOLUME_DECODER", "octree")
    with pytest.raises(ValueError):
        _pipeline()
    monkeypatch.delenv("R3G_VOLUME_DECODER")
    assert _pipeline().volume_decoder == "vanilla"


def test_stage_yaml_key(monkeypatch):
    monkeypatch.delenv("R3G_VOLUME_DECODER", raising=False)
    spec = importlib.util.spec_from_file_location("r3g_stage_run_hier", os.path.join(ROOT, "3d-re-gen_amd", "stage", "run.py"))
    stage = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stage)
    assert stage.volume_decoder({}) is None
    assert stage.volume_decoder({"r3g_volume_decoder": "hierarchical"}) == "hierarchical"
    with pytest.raises(ValueError):
        stage.volume_decoder({"r3g_volume_decoder": "flash"})
    p = _pipeline()
    assert stage.apply_volume_decoder({}, p).volume_decoder == "vanilla"
    assert stage.apply_volume_decoder({"r3g_volume_decoder": "hierarchical"}, p).volume_decoder == "hierarchical"
    assert stage.apply_volume_decoder({}, p).volume_decoder == "hierarchical"          # an absent key changes nothing
    assert stage.apply_volume_decoder({"r3g_volume_decoder": "vanilla"}, p).volume_decoder == "vanilla"
    with pytest.raises(ValueError):
        stage.apply_volume_decoder({"r3g_volume_decoder": "dense"}, p)


def test_reference_planner_edge_cases():
    """n_coarse 2 and 3, a field without a candidate, NaN / inf samples: the rule is well defined"""
    for nc in (2, 3):
        G = np.full((nc, nc, nc), -1, np.float32)
        G[0, 0, 0] = 1
        for last in (True, False):
            F = hier_ref.plan(G, 0.0, 0.95, last)
            assert F.shape == (2 * nc - 1,) * 3 and F[0, 0, 0] and F.sum() > 1
    assert hier_ref.plan(np.full((5, 5, 5), 7.0, np.float32), 0.0, 0.95, True).sum() == 0
    G = np.full((4, 4, 4), 7.0, np.float32)
    G[1, 1, 1], G[2, 2, 2], G[0, 3, 0] = np.nan, np.inf, -np.inf
    F = hier_ref.plan(G, 0.0, 0.95, True)
    assert F[2, 2, 2] and F[0, 6, 0] and not F[6, 6, 6]   # NaN and -inf are "not above": they and their neighbours are candidates; +inf is not
    assert np.array_equal(hier_ref.active_indices(F), np.flatnonzero(F.ravel()))


# evaluated shares of the prototype the issue was written with (recorded there; the condition asserted is 0 missed / 0 unsafe)
SHARES = {"sphere": 0.0939, "ellipsoid": 0.1087, "blobs_sharp": 0.0562, "blobs_soft": 0.0565, "thin_rod": 0.0487}


@pytest.mark.parametrize("name", hier_ref.ANALYTIC)
def test_fixture_guard_reference_planner_misses_nothing(name):
    dense, lam = hier_ref.analytic_field(name)
    assert dense.shape == (257, 257, 257) and dense.dtype == np.float32
    if name == "sphere":
        from mc_volumes import golden_volume
        assert np.array_equal(dense, golden_volume("D")[0])
    G, F, per_level = hier_ref.hier(hier_ref.strided(dense), 256, lam, 0.95)
    missed, unsafe = hier_ref.missed_and_unsafe(dense, G, F, lam)
    share = sum(per_level) / dense.size
    print("%s: evaluated share %.4f, missed %d, unsafe %d" % (name, share, missed, unsafe))
    assert missed == 0 and unsafe == 0
    assert np.array_equal(hier_ref.mixed_cells(G, lam), hier_ref.mixed_cells(dense, lam))
    assert np.array_equal(G[F], dense[F])
    assert abs(share - SHARES[name]) < 5e-4
