"""Adaptive top-k KV selection, host side (no GPU): the -1 rule, the restatement the GPU tests rely on (tests/kvsel_ref.py) against
the oracle's exact geo decoder, and the public switches (pipeline.kv_selection, R3G_KV_SELECTION, the stage's `r3g_kv_selection`
key).  enable_flashvdm's `adaptive_kv_selection` argument stays accepted and ignored."""
import importlib.util
import os

import numpy as np
import pytest

import kvsel_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,expect", [(3072, 1024), (512, 256), (256, 85)])
def test_upstream_rule(n, expect):
    from r3g import model as M
    assert M.kv_topk(-1, n) == expect == kvsel_ref.upstream_topk(n)
    assert M.kv_topk(0, n) == 0                                   # exact
    assert M.kv_topk(100, n) == 100 and M.kv_topk(10 ** 6, n) == n   # a key count, clamped to the latents
    with pytest.raises(ValueError):
        M.kv_topk(-2, n)


def test_reference_selection_rules():
    """ties go to the lower index, a NaN ranks below every number, the result is ascending"""
    s = np.array([1.0, 3.0, 3.0, np.nan, 3.0, -np.inf, 0.0, -0.0])
    assert kvsel_ref.select(s, 1).tolist() == [1]
    assert kvsel_ref.select(s, 2).tolist() == [1, 2]
    assert kvsel_ref.select(s, 4).tolist() == [0, 1, 2, 4]
    assert kvsel_ref.select(s, 5).tolist() == [0, 1, 2, 4, 6]         # +0 and -0 are equal: the lower index
    assert kvsel_ref.select(s, 7).tolist() == [0, 1, 2, 4, 5, 6, 7]   # -inf is a number: before the NaN
    assert kvsel_ref.select(s, 8).tolist() == list(range(8))
    assert kvsel_ref.select(np.array([np.nan, 1.0, np.nan]), 2).tolist() == [0, 1]
    assert kvsel_ref.groups(2500, 1024) == [(0, 1024), (1024, 1024), (2048, 452)]
    assert kvsel_ref.sample_rows(452, 64) == [0, 64, 128, 192, 256, 320, 384, 448] and kvsel_ref.sample_rows(30, 64) == [0]


def test_restatement_with_every_key_is_the_exact_decoder():
    """k = N_lat: the selection is the identity and the restated decoder is the oracle's own (fp32 SDPA per group of queries
    instead of over all of them: the same sums, compared to 1e-6 of the logits' scale)"""
    import torch
    from oracle import hy3d_torch as H
    cfg = H.tiny_config()
    vae = H.ShapeVAE(**cfg["vae"]).eval()
    sd = H.synthetic_state_dict(cfg, seed=3)
    vae.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("vae.")}, strict=True)
    g = torch.Generator().manual_seed(5)
    N, heads = cfg["vae"]["num_latents"], cfg["vae"]["heads"]
    with torch.no_grad():
        z = vae(torch.randn(1, N, cfg["vae"]["embed_dim"], generator=g))
        pts = torch.rand(1, 700, 3, generator=g) * 2 - 1
        want = vae.geo_decoder(queries=pts, latents=z)
        table = np.broadcast_to(np.arange(N), (3, heads, N))
        got = kvsel_ref.topk_geo_decoder(vae.geo_decoder, table, 256)(queries=pts, latents=z)
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
        # and a real selection changes the result (the table is used)
        q, k = kvsel_ref.oracle_qk(vae.geo_decoder, pts[0], z)
        s, _, _ = kvsel_ref.scores(q, k, 256, 64)
        idx = kvsel_ref.select(s, 85)
        assert idx.shape == (3, heads, 85)
        part = kvsel_ref.topk_geo_decoder(vae.geo_decoder, idx, 256)(queries=pts, latents=z)
        assert torch.isfinite(part).all() and float((part - want).abs().max()) > 0


class _StubModel:
    num_latents, in_channels = 3072, 4

    def __init__(self):
        self.calls = []

    def set_kv_selection(self, topk=0, group=None, stride=None):
        from r3g import model as M
        self.calls.append(("kv", topk, group, stride))
        return M.kv_topk(topk, self.num_latents)

    def grid_query(self, bound, R):
        self.calls.append(("vanilla", bound, R))
        return "dense-grid"

    def grid_query_hier(self, bound, R, mc_level, band, min_resolution):
        self.calls.append(("hierarchical", bound, R))
        return "hier-grid", {"levels": [R // 2, R], "evaluated_per_level": [5, 7], "evaluated": 12, "dense_points": (R + 1) ** 3,
                             "unsafe_cells": 0}


def _pipeline():
    import hy3dgen.shapegen.pipelines as pl

    class P(pl.Hunyuan3DDiTFlowMatchingPipeline):
        def _make_model(self, cfg, state_dict, grid_chunk):
            return _StubModel()
    return P(pl.builtin_config("full"), {}, "cuda:0")


def test_pipeline_attribute_is_applied_before_every_grid_query(monkeypatch):
    monkeypatch.delenv("R3G_KV_SELECTION", raising=False)
    monkeypatch.delenv("R3G_VOLUME_DECODER", raising=False)
    p = _pipeline()
    assert p.kv_selection == "exact" and p.kv_topk is None and p.kv_group is None and p.kv_stride is None
    assert p._query_grid(1.01, 128, 0.0) == "dense-grid"
    assert p.model.calls == [("kv", 0, None, None), ("vanilla", 1.01, 128)] and p.timings["kv_selection"] == "exact"
    p.kv_selection = "topk"
    p._query_grid(1.01, 128, 0.0)
    assert p.model.calls[-2:] == [("kv", -1, None, None), ("vanilla", 1.01, 128)]      # upstream's rule unless kv_topk says otherwise
    assert p.timings["kv_selection"] == "topk:1024"
    p.kv_topk, p.kv_group, p.kv_stride = 512, 4096, 32
    p.enable_flashvdm()                                             # both volume decoders
    assert p._query_grid(1.01, 128, 0.0) == "hier-grid"
    assert p.model.calls[-2:] == [("kv", 512, 4096, 32), ("hierarchical", 1.01, 128)] and p.timings["kv_selection"] == "topk:512"
    p.kv_selection = "exact"
    p._query_grid(1.01, 128, 0.0)
    assert p.model.calls[-2][:2] == ("kv", 0) and p.timings["kv_selection"] == "exact"
    p.kv_selection = "top-k"
    with pytest.raises(ValueError):
        p._query_grid(1.01, 128, 0.0)


def test_enable_flashvdm_leaves_the_selection_exact(monkeypatch):
    monkeypatch.delenv("R3G_KV_SELECTION", raising=False)
    monkeypatch.delenv("R3G_VOLUME_DECODER", raising=False)
    p = _pipeline()
    p.enable_flashvdm(adaptive_kv_selection=True)
    assert p.volume_decoder == "hierarchical" and p.kv_selection == "exact"
    p.enable_flashvdm(adaptive_kv_selection=True, topk_mode="mean")
    p._query_grid(1.01, 128, 0.0)
    assert p.kv_selection == "exact" and p.timings["kv_selection"] == "exact" and ("kv", 0, None, None) in p.model.calls
    p.kv_selection = "topk"
    p.enable_flashvdm(adaptive_kv_selection=False)                  # ... and does not switch it off either
    assert p.kv_selection == "topk"


def test_environment_variable_selects_the_mode(monkeypatch):
    monkeypatch.setenv("R3G_KV_SELECTION", "topk")
    assert _pipeline().kv_selection == "topk"
    monkeypatch.setenv("R3G_KV_SELECTION", "exact")
    assert _pipeline().kv_selection == "exact"
    monkeypatch.setenv("R3G_KV_SELECTION", "adaptive")
    with pytest.raises(ValueError):
        _pipeline()
    monkeypatch.delenv("R3G_KV_SELECTION")
    assert _pipeline().kv_selection == "exact"


def test_stage_yaml_key(monkeypatch):
    monkeypatch.delenv("R3G_KV_SELECTION", raising=False)
    spec = importlib.util.spec_from_file_location("r3g_stage_run_kvsel", os.path.join(ROOT, "3d-re-gen_amd", "stage", "run.py"))
    stage = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stage)
    assert stage.kv_selection({}) is None
    assert stage.kv_selection({"r3g_kv_selection": "topk"}) == "topk" and stage.kv_selection({"r3g_kv_selection": "exact"}) == "exact"
    with pytest.raises(ValueError):
        stage.kv_selection({"r3g_kv_selection": "mean"})
    p = _pipeline()
    assert stage.apply_kv_selection({}, p).kv_selection == "exact"
    assert stage.apply_kv_selection({"r3g_kv_selection": "topk"}, p).kv_selection == "topk"
    assert stage.apply_kv_selection({}, p).kv_selection == "topk"             # an absent key changes nothing
    assert stage.apply_kv_selection({"r3g_kv_selection": "exact"}, p).kv_selection == "exact"
    with pytest.raises(ValueError):
        stage.apply_kv_selection({"r3g_kv_selection": "TOPK"}, p)


def test_option_ranges_are_checked_without_a_gpu():
    """plain host state of the library: refused values change nothing"""
    from r3g import ffi
    L = ffi.lib()
    try:
        assert L.r3g_set_option(b"geo_kv_group", 1000) != 0 and L.r3g_set_option(b"geo_kv_group", 128) != 0
        assert L.r3g_set_option(b"geo_kv_group", 0) != 0
        assert L.r3g_set_option(b"geo_kv_stride", 0) != 0 and L.r3g_set_option(b"geo_kv_topk", -2) != 0
        assert L.r3g_set_option(b"geo_kv_mode", 1) != 0
        assert L.r3g_set_option(b"geo_kv_group", 1024) == 0 and L.r3g_set_option(b"geo_kv_stride", 1) == 0
        assert L.r3g_set_option(b"geo_kv_topk", -1) == 0
    finally:
        assert L.r3g_set_option(b"geo_kv_topk", 0) == 0
        assert L.r3g_set_option(b"geo_kv_group", 8192) == 0 and L.r3g_set_option(b"geo_kv_stride", 64) == 0
    assert ffi.counter("geo_kv_groups") >= 0
