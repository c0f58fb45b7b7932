"""Dual marching cubes (mc_algo="dmc"), host side (no GPU): the generated case table against the
numpy restatement (tests/dmc_ref.py), the literal facts about the 256 cases, the host emulation of the product's per-cell
code (csrc/dmc_cell.h through tests/emu/dmc_emu.cpp) against the restatement bit for bit, restatement-independent mesh
properties on the golden volumes, and the plumbing of the public switches (call keyword, pipeline attribute, stage key)."""
import importlib.util
import os
import re

import numpy as np
import pytest

import dmc_ref
from mc_volumes import golden_volume, small_volumes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "3d-re-gen_amd", "csrc", "dmc_luts.h")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def padded(vol):
    """one layer of -1 around the volume: below every level used here, so the surface closes inside the grid"""
    return np.pad(np.asarray(vol, np.float32), 1, constant_values=-1.0)


# ---- the case table -------------------------------------------------------------------------------------------
def test_committed_header_is_the_generators_output():
    gen = _load("gen_dmc_luts", os.path.join(ROOT, "tools", "gen_dmc_luts.py"))
    with open(HEADER) as f:
        assert f.read() == gen.render()


def header_words():
    with open(HEADER) as f:
        txt = f.read()
    body = txt[txt.index("R3G_DMC_CASE[256]"):]
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", body)]
    assert len(words) == 256
    return words


def test_header_decodes_to_the_restatements_tables():
    T = dmc_ref.tables()
    for case, w in enumerate(header_words()):
        patch = [(w >> (4 * e)) & 0xF for e in range(12)]
        assert [p if p != 15 else -1 for p in patch] == list(T["patch"][case]), case
        assert (w >> 48) & 0x7 == T["count"][case], case
        tunnel = (w >> 52) & 0x7
        assert (tunnel if tunnel != 7 else -1) == T["tunnel"][case], case
        assert w >> 55 == 0 and (w >> 51) & 1 == 0, case


def test_literal_facts_about_the_256_cases():
    T = dmc_ref.tables()
    assert {k: int((T["count"] == k).sum()) for k in range(5)} == {0: 2, 1: 162, 2: 82, 3: 8, 4: 2}
    for case in range(256):
        for p in range(T["count"][case]):
            assert int((T["patch"][case] == p).sum()) >= 3, case
        # patches are ordered by their smallest edge
        firsts = [int(np.flatnonzero(T["patch"][case] == p)[0]) for p in range(T["count"][case])]
        assert firsts == sorted(firsts), case
    tun = np.flatnonzero(T["tunnel"] >= 0)
    assert len(tun) == 36
    assert np.all(T["n_ambiguous"][tun] == 1)
    inside = np.array([bin(int(c)).count("1") for c in tun])
    assert int((inside == 5).sum()) == 24 and int((inside == 6).sum()) == 12
    assert np.all(T["count"][tun] == 1)
    assert np.all(T["count"][tun ^ 255] == 2) and np.all(T["tunnel"][tun ^ 255] == -1)


# ---- the product's per-cell code on the host --------------------------------------------------------------------
def abi_result(vol, level, manifold=True, xform=None):
    """the emulation's arrays behind the error rules of r3g_dmc_count"""
    import emu_dmc
    v, f, flags, flipped = emu_dmc.dual_marching_cubes(vol, level, manifold, xform)
    if not (flags & 4) and (not (flags & 1) or not (flags & 2)):
        raise dmc_ref.DmcError(dmc_ref.R3G_ERR_LEVEL_RANGE)
    if len(f) == 0:
        raise dmc_ref.DmcError(dmc_ref.R3G_ERR_NO_SURFACE)
    return v, f, flipped


def assert_emulation_equals_restatement(vol, level, tag):
    n = np.array(vol.shape, np.float64)
    xf = (n - 1.0, np.array([2.02, 2.0, 1.5]), np.array([-1.01, -1.0, 0.3]))
    for manifold in (True, False):
        for xform in (None, xf):
            try:
                rv, rf, info = dmc_ref.dual_marching_cubes(vol, level, manifold, xform)
            except dmc_ref.DmcError as want:
                with pytest.raises(dmc_ref.DmcError) as got:
                    abi_result(vol, level, manifold, xform)
                assert got.value.code == want.code, tag
                continue
            v, f, flipped = abi_result(vol, level, manifold, xform)
            assert f.dtype == np.int32 and np.array_equal(f, rf), (tag, manifold, xform is not None)
            assert bits_equal(v, rv), (tag, manifold, xform is not None)
            assert flipped == info["n_flipped"], tag


def test_emulation_equals_the_restatement_on_the_small_volumes():
    vols = small_volumes()
    names = [k for k in vols if not k.startswith("level_")]
    assert {"noise_ragged", "nan", "plane", "two_blobs", "minimal", "outside_level", "lone_equal_below"} <= set(names)
    for k in names:
        assert_emulation_equals_restatement(vols[k], float(vols["level_" + k]), k)
    errors = {}
    for k in ("outside_level", "lone_equal_below", "minimal"):
        with pytest.raises(dmc_ref.DmcError) as e:
            dmc_ref.dual_marching_cubes(vols[k], float(vols["level_" + k]))
        errors[k] = e.value.code
    assert errors == {"outside_level": -10, "lone_equal_below": -11, "minimal": -11}


@pytest.mark.parametrize("name", ["A", "B", "C", "B-padded"])
def test_emulation_equals_the_restatement_on_the_goldens(name):
    vol, level = golden_volume(name[0])
    assert_emulation_equals_restatement(padded(vol) if name.endswith("padded") else vol, level, name)


# ---- restatement-independent properties -----------------------------------------------------------------------------
SPHERES = {"A": dict(V=7472, F=14940, r2=399.5, c=32.0, below=0.03), "D": dict(V=188384, F=376764, r2=9999.5, c=128.0, below=0.01)}


def check_sphere(name, v, f):
    g = SPHERES[name]
    assert (len(v), len(f)) == (g["V"], g["F"])
    key, cnt = dmc_ref.edge_face_counts(f, len(v))
    assert np.all(cnt == 2)
    assert len(v) - len(key) + len(f) == 2
    assert not np.any((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0]))
    r = np.sqrt(g["r2"])
    vol = dmc_ref.signed_volume(v.astype(np.float64) - g["c"], f)
    assert vol > 0 and abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 0.005
    rad = np.linalg.norm(v.astype(np.float64) - g["c"], axis=1)
    assert rad.min() >= r - g["below"] and rad.max() <= r + 1e-3


def check_padded_b(run):
    """run(vol, level, manifold) -> (verts, faces, cells that took the complemented case or None)"""
    vol, level = golden_volume("B")
    p = padded(vol)
    assert p.shape == (35, 35, 35)
    v, f, flipped = run(p, level, True)
    key, cnt = dmc_ref.edge_face_counts(f, len(v))
    assert np.all(cnt == 2)
    assert (len(v), len(f)) == (54572, 2 * 56582)
    assert flipped in (None, 788)
    v0, f0, _ = run(p, level, False)
    key0, cnt0 = dmc_ref.edge_face_counts(f0, len(v0))
    assert int((cnt0 == 4).sum()) == 394 and not np.any(cnt0 % 2 == 1) and set(np.unique(cnt0)) == {2, 4}


def check_padded_small(run):
    vols = small_volumes()
    for k in ("noise_9", "noise_ragged", "ints", "ints_level", "smooth_12"):
        v, f, _ = run(padded(vols[k]), float(vols["level_" + k]), True)
        key, cnt = dmc_ref.edge_face_counts(f, len(v))
        assert len(f) > 0 and np.all(cnt == 2), k


def _ref_run(vol, level, manifold):
    v, f, info = dmc_ref.dual_marching_cubes(vol, level, manifold)
    return v, f, info["n_flipped"]


def _emu_run(vol, level, manifold):
    return abi_result(vol, level, manifold)


@pytest.mark.parametrize("name", ["A", "D"])
def test_golden_spheres_restatement(name):
    vol, level = golden_volume(name)
    v, f, _ = dmc_ref.dual_marching_cubes(vol, level)
    check_sphere(name, v, f)


@pytest.mark.parametrize("name", ["A", "D"])
def test_golden_spheres_emulation(name):
    vol, level = golden_volume(name)
    v, f, _ = abi_result(vol, level)
    check_sphere(name, v, f)


@pytest.mark.parametrize("run", [_ref_run, _emu_run], ids=["restatement", "emulation"])
def test_manifold_rule_on_padded_noise(run):
    check_padded_b(run)
    check_padded_small(run)


# ---- plumbing: call keyword, pipeline attribute, stage key ------------------------------------------------------------
class _StubModel:
    num_latents, in_channels = 8, 4
    ctx = None

    def vae_decode(self, latents):
        pass

    def grid_query(self, bound, R):
        return "grid"


def _pipeline():
    import hy3dgen.shapegen.pipelines as pl

    class P(pl.Hunyuan3DDiTFlowMatchingPipeline):
        def __init__(self, *a, **k):
            self.calls = []
            super().__init__(*a, **k)

        def _make_model(self, cfg, state_dict, grid_chunk):
            return _StubModel()

        def _device_ctx(self):
            import contextlib
            return contextlib.nullcontext()

        def generate_latents(self, images, *a, **k):
            return ["latents"] * len(images)

        def _extract_mesh(self, grid, mc_level, box_v, octree_resolution):
            self.calls.append(("mc", grid, mc_level, box_v, octree_resolution))
            return "v-mc", "f-mc"

        def _extract_mesh_dmc(self, grid, mc_level, octree_resolution):
            self.calls.append(("dmc", grid, mc_level, octree_resolution))
            if mc_level == 99.0:
                raise RuntimeError("No surface found at the given iso value.")
            return "v-dmc", "f-dmc"
    return P(pl.builtin_config("full"), {}, "cuda:0")


def test_call_keyword_and_attribute_select_the_extractor():
    import inspect
    import hy3dgen.shapegen.pipelines as pl
    sig = inspect.signature(pl.Hunyuan3DDiTFlowMatchingPipeline._extract_mesh)
    assert list(sig.parameters) == ["self", "grid", "mc_level", "box_v", "octree_resolution"]
    sig = inspect.signature(pl.Hunyuan3DDiTFlowMatchingPipeline._extract_mesh_dmc)
    assert list(sig.parameters) == ["self", "grid", "mc_level", "octree_resolution"]
    p = _pipeline()
    assert p.mc_algo == "mc"
    kw = dict(num_inference_steps=2, octree_resolution=32, output_type="raw")
    assert p(image="img", **kw) == [("v-mc", "f-mc")]
    assert p(image="img", mc_algo="mc", **kw) == [("v-mc", "f-mc")]
    assert [c[0] for c in p.calls] == ["mc", "mc"]
    assert p(image="img", mc_algo="dmc", mc_level=0.25, **kw) == [("v-dmc", "f-dmc")]
    assert p.calls[-1] == ("dmc", "grid", 0.25, 32)
    with pytest.raises(NotImplementedError):
        p(image="img", mc_algo="foo", **kw)
    assert len(p.calls) == 3
    # the attribute serves a call that passes None; an explicit keyword wins
    p.mc_algo = "dmc"
    assert p(image="img", **kw) == [("v-dmc", "f-dmc")]
    assert p(image="img", mc_algo="mc", **kw) == [("v-mc", "f-mc")]
    assert p(image=["a", "b"], **kw) == [("v-dmc", "f-dmc")] * 2
    p.mc_algo = "foo"
    with pytest.raises(NotImplementedError):
        p(image="img", **kw)
    # a failed extraction yields None for that object
    p.mc_algo = "mc"
    assert p(image="img", mc_algo="dmc", mc_level=99.0, **kw) == [None]
    # enable_flashvdm keeps refusing an extractor choice, and says where the choice lives
    with pytest.raises(NotImplementedError):
        p.enable_flashvdm(mc_algo="dmc")
    assert "mc_algo" in p.enable_flashvdm.__doc__ and "per call" in p.enable_flashvdm.__doc__


def test_stage_yaml_key():
    stage = _load("r3g_stage_run_dmc", os.path.join(ROOT, "3d-re-gen_amd", "stage", "run.py"))
    assert stage.mc_algo({}) is None
    assert stage.mc_algo({"r3g_mc_algo": "dmc"}) == "dmc" and stage.mc_algo({"r3g_mc_algo": "mc"}) == "mc"
    with pytest.raises(ValueError) as e:
        stage.mc_algo({"r3g_mc_algo": "diso"})
    assert "mc, dmc" in str(e.value)
    p = _pipeline()
    assert stage.apply_mc_algo({}, p).mc_algo == "mc"
    assert stage.apply_mc_algo({"r3g_mc_algo": "dmc"}, p).mc_algo == "dmc"
    assert stage.apply_mc_algo({}, p).mc_algo == "dmc"                     # an absent key changes nothing
    assert stage.apply_mc_algo({"r3g_mc_algo": "mc"}, p).mc_algo == "mc"
    with pytest.raises(ValueError):
        stage.apply_mc_algo({"r3g_mc_algo": "DMC"}, p)


def test_python_entry_points_refuse_what_r3g_mc_refuses():
    import torch
    from r3g import dmc
    with pytest.raises(ValueError):
        dmc.dual_marching_cubes(torch.zeros(4, 4, 4), 0.0)          # CPU tensor: refused, not silently handled
    with pytest.raises(ValueError):
        dmc.dual_marching_cubes(torch.zeros(4, 4), 0.0)
    with pytest.raises(ValueError):
        dmc.dual_marching_cubes(np.zeros((4, 4, 4), np.float32), 0.0)
    with pytest.raises(ValueError):
        dmc.extract_mesh(torch.zeros(4, 4, 4), 0.0)
