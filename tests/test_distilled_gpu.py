"""Guidance-distilled shape models (upstream's -fast / -turbo checkpoints) on the GPU: r3g_flow_sample_sigmas and the CFG-free form
of the grouped DiT engine against the test-side restatement tests/distilled_ref.py ([UPSTREAM-RECALLED], parity unpinned: DESIGN.md
section 4b), on identical seeded synthetic weights.  Tolerances are tests/parity_support.py's; tests/test_distilled_cpu.py proves
that every wiring hazard of what a distilled model adds lies >= 5 x outside them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import distilled_ref as R
from parity_support import TOL, bf16_round_matrices, rel_l2, report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 5.0


class DSetup:
    def __init__(self, cfg, seed, with_ref=True):
        from r3g import model as M
        self.cfg = R.distilled_cfg(cfg)
        self.sd = bf16_round_matrices(R.synthetic_state_dict(self.cfg, seed))
        self.ref = R.load_dit(self.cfg, self.sd) if with_ref else None
        self.gpu = M.ShapeModel(self.cfg, self.sd, 0, grid_chunk=4096)


def _cfg(which):
    from oracle import hy3d_torch as H
    if which == "tiny":
        return H.tiny_config(), 3
    if which == "mini-dims":
        cfg = H.mini_config()
        cfg["dit"].update(depth=1, depth_single_blocks=2)
        cfg["vae"].update(num_decoder_layers=1)
        cfg["cond"].update(num_hidden_layers=1)
        return cfg, 41
    return H.wide_config(depth=1, depth_single=1, vae_layers=1, cond_layers=1), 11


_SETUPS = {}


@pytest.fixture
def setup(request):
    which = request.param
    if which not in _SETUPS:
        _SETUPS[which] = DSetup(*_cfg(which))
    return which, _SETUPS[which]


def _inputs(s, seed, n=1):
    """latents f32 [n, N, C], cond2 [n, 2, Lc, D] whose UNCONDITIONAL half is NaN: a distilled model never reads it"""
    import torch
    from parity_support import dit_inputs
    xs, cs = [], []
    for o in range(n):
        x, _, cond = dit_inputs(s.cfg, seed + 101 * o, batch=1)
        xs.append(x[0])
        cs.append(torch.stack([cond[0], torch.full_like(cond[0], float("nan"))]))
    return torch.stack(xs), torch.stack(cs)


CASES = [("one evaluation", None, 1), ("consistency", True, 5), ("consistency", True, 8), ("linspace", False, 5),
         ("linspace", False, 8), ("linspace", False, 50)]


@pytest.mark.parametrize("setup", ["tiny", "mini-dims", "wide"], indirect=True)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d" % (c[0].replace(" ", "_"), c[2]))
def test_sampler_matches_the_restatement(setup, case):
    import torch
    which, s = setup
    name, consistency, steps = case
    sig = np.array([0.37, 0.62], np.float32) if consistency is None else R.table(steps, consistency)
    x, cond2 = _inputs(s, 2)
    ref = R.sample(s.ref, cond2[:, 0], x.clone(), sig, G)
    out = s.gpu.flow_sample_sigmas(x.clone(), cond2, sig, G).cpu()
    assert torch.isfinite(out).all()
    tol = TOL["flow_sample_50"] if steps == 50 else TOL["flow_sample"]
    err, moved = rel_l2(out, ref), rel_l2(ref, x)
    report("distilled %s: %s table, %d steps (latents moved by %.2f)" % (which, name, steps, moved), err, tol)
    print("distilled %s %s %d: rel-L2 %.3e (tolerance %.1e), moved %.3f" % (which, name, steps, err, tol, moved))
    assert err <= tol
    assert rel_l2(out, x) > 0.3                       # the tolerance is not met by standing still (all six cases)


@pytest.mark.parametrize("setup", ["tiny", "wide"], indirect=True)
def test_zero_guidance_in_is_the_established_forward(setup):
    """guidance_in's weights AND biases zero: vec = time_in(t), and the one-step result, turned back into v, is r3g_dit_forward at
    B = 1 on the same weights (the engine the per-block parity tests pin)"""
    import torch
    from r3g import model as M
    which, s = setup
    sd0 = dict(s.sd)
    for k in R.GUIDANCE_KEYS:
        sd0[k] = torch.zeros_like(sd0[k])
    gpu0 = M.ShapeModel(s.cfg, sd0, 0, grid_chunk=4096)
    x, cond2 = _inputs(s, 7)
    s0, s1 = 0.37, 0.62
    out = gpu0.flow_sample_sigmas(x.clone(), cond2, np.array([s0, s1], np.float32), G).cpu()
    v = (out - x) / (np.float32(s1) - np.float32(s0))
    fwd = gpu0.dit_forward(x, torch.full((1,), s0), cond2[:, 0]).cpu()
    err = rel_l2(v, fwd)
    report("distilled %s: zero guidance_in, one step as v against r3g_dit_forward" % which, err, TOL["same_function"])
    assert err <= TOL["same_function"]
    # and with the real guidance_in the same step is a different function
    real = s.gpu.flow_sample_sigmas(x.clone(), cond2, np.array([s0, s1], np.float32), G).cpu()
    assert rel_l2(real, out) > 5 * TOL["same_function"] * rel_l2(out, x)


@pytest.mark.parametrize("setup,n", [("tiny", 2), ("tiny", 3), ("tiny", 5), ("tiny", 8), ("tiny", 9), ("wide", 2), ("wide", 8)],
                         indirect=["setup"])
def test_objects_sharing_a_launch_are_bit_identical_to_single_runs(setup, n):
    """up to 8 objects per launch group (9: a group of 8 and one of 1); a GEMM row does not know which object it belongs to"""
    import torch
    from r3g import ffi
    which, s = setup
    sig = R.table(3 if which == "tiny" else 2, True)
    x, cond2 = _inputs(s, 13, n)
    g0 = ffi.counter("dit_groups")
    out = s.gpu.flow_sample_sigmas(x.clone(), cond2, sig, G).clone()
    assert ffi.counter("dit_groups") - g0 == (n + 7) // 8
    assert torch.isfinite(out).all()
    for o in range(n):
        one = s.gpu.flow_sample_sigmas(x[o:o + 1].clone(), cond2[o:o + 1], sig, G)
        assert torch.equal(out[o], one[0]), (which, n, o)
    assert not torch.equal(out[0], out[1])


@pytest.mark.parametrize("setup", ["tiny"], indirect=True)
def test_latents_need_no_particular_alignment(setup):
    """the Euler update uses float4 accesses on 16-byte aligned latents and a per-element kernel otherwise: same bits"""
    import torch
    _, s = setup
    x, cond2 = _inputs(s, 17, 2)
    sig = R.table(3, True)
    want = s.gpu.flow_sample_sigmas(x.clone(), cond2, sig, G).clone()
    flat = torch.empty(x.numel() + 1, dtype=torch.float32, device=s.gpu.device)
    un = flat[1:].view(x.shape)
    un.copy_(x)
    assert un.data_ptr() % 16 == 4 and un.is_contiguous()
    got = s.gpu.flow_sample_sigmas(un, cond2, sig, G)
    assert got.data_ptr() == un.data_ptr() and torch.equal(got, want)


def test_wrappers_are_the_same_function_on_a_cfg_model():
    """r3g_flow_sample / r3g_flow_sample_batch build the linspace table and call r3g_flow_sample_sigmas: on a CFG model (no
    guidance_in) the explicit table gives the same bits, on the fp32 stream (tiny) and on the fp16 stream (256 wide)"""
    import torch
    from oracle import hy3d_torch as H
    from parity_support import dit_inputs
    from r3g import ffi, flow
    from r3g import model as M
    for hidden in (128, 256):
        cfg = H.tiny_config()
        if hidden == 256:
            cfg["dit"].update(hidden_size=256, num_heads=4, depth=1, depth_single_blocks=1)
        sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=9))
        gpu = M.ShapeModel(cfg, sd, 0, grid_chunk=4096)
        assert not gpu.guidance_embed
        N = 6
        xs, cs = [], []
        for o in range(3):
            x, _, cond = dit_inputs(cfg, 3 + o)
            xs.append(x[0])
            cs.append(cond)
        x, cond2 = torch.stack(xs), torch.stack(cs)
        sig = flow.euler_sigmas(N)
        e0 = ffi.counter("dit_evals")
        a = gpu.flow_sample(x[0].clone(), cond2[0], N, G).clone()
        assert ffi.counter("dit_evals") - e0 == N - 1                      # the zero step is skipped
        e0 = ffi.counter("dit_evals")
        b = gpu.flow_sample_sigmas(x[:1].clone(), cond2[:1], sig, G).clone()
        assert ffi.counter("dit_evals") - e0 == N - 1
        assert torch.equal(a, b[0])
        c = gpu.flow_sample_batch(x.clone(), cond2, N, G).clone()
        e0 = ffi.counter("dit_evals")
        d = gpu.flow_sample_sigmas(x.clone(), cond2, sig, G).clone()
        assert ffi.counter("dit_evals") - e0 == N - 1                      # one launch group
        assert torch.equal(c, d) and torch.equal(c[0], a)
        # another table is another function (the table is really read)
        e = gpu.flow_sample_sigmas(x[:1].clone(), cond2[:1], flow.consistency_sigmas(N), G)
        assert not torch.equal(e, b)


@pytest.mark.parametrize("setup", ["tiny"], indirect=True)
def test_dit_evals_counts_every_step_of_the_consistency_table(setup):
    from r3g import ffi
    _, s = setup
    x, cond2 = _inputs(s, 5, 9)
    for n_obj, groups in ((1, 1), (8, 1), (9, 2)):
        e0 = ffi.counter("dit_evals")
        s.gpu.flow_sample_sigmas(x[:n_obj].clone(), cond2[:n_obj], R.table(5, True), G)
        assert ffi.counter("dit_evals") - e0 == 5 * groups
    e0 = ffi.counter("dit_evals")
    s.gpu.flow_sample_sigmas(x[:1].clone(), cond2[:1], R.table(5, False), G)
    assert ffi.counter("dit_evals") - e0 == 4                                # linspace: the zero step is skipped


def test_fp16_stream_overflow_of_a_cfg_free_group_runs_again_on_the_fp32_stream():
    """the guard of the fp16 residual stream on a CFG-free group (recipe of tests/test_model_gpu.py::
    test_fp16_stream_overflow_runs_the_group_again_on_the_fp32_stream: the input projection scaled by 1e5 on a 256-wide model): the
    result IS the fp32 stream's, bit for bit, and dit_f16_fallbacks moves by one"""
    import torch
    from oracle import hy3d_torch as H
    from r3g import ffi
    from r3g import model as M
    L = ffi.lib()
    cfg = H.tiny_config()
    cfg["dit"].update(hidden_size=256, num_heads=4, depth=1, depth_single_blocks=1)
    cfg = R.distilled_cfg(cfg)
    sd = bf16_round_matrices(R.synthetic_state_dict(cfg, 9))
    sd["model.latent_in.weight"] = sd["model.latent_in.weight"] * 1e5
    s = DSetup.__new__(DSetup)
    s.cfg = cfg
    gpu = M.ShapeModel(cfg, sd, 0, grid_chunk=4096)
    x, cond2 = _inputs(s, 3, 2)
    sig = R.table(3, True)
    f0 = ffi.counter("dit_f16_fallbacks")
    guarded = gpu.flow_sample_sigmas(x.clone(), cond2, sig, G).clone()
    assert ffi.counter("dit_f16_fallbacks") - f0 == 1
    try:
        ffi.check(L.r3g_set_option(b"dit_resid_f16", 0))
        f32 = gpu.flow_sample_sigmas(x.clone(), cond2, sig, G).clone()
    finally:
        ffi.check(L.r3g_set_option(b"dit_resid_f16", 1))
    try:
        ffi.check(L.r3g_set_option(b"dit_f16_guard", 0))
        raw = gpu.flow_sample_sigmas(x.clone(), cond2, sig, G).clone()
    finally:
        ffi.check(L.r3g_set_option(b"dit_f16_guard", 1))
    assert torch.isfinite(f32).all() and torch.equal(guarded, f32)
    assert not torch.isfinite(raw).all()                         # so this input does force the branch
    assert ffi.counter("dit_f16_fallbacks") - f0 == 1


# ---- public surface ------------------------------------------------------------------------------------------------------
def _crops(n):
    sys.path.insert(0, ROOT)
    from bench import synthetic_crop
    return [synthetic_crop(i) for i in range(n)]


def _check_meshes(meshes, n):
    assert len(meshes) == n
    for m in meshes:
        assert m is not None and len(m.faces) > 0
        assert np.isfinite(np.asarray(m.vertices)).all()


def test_from_pretrained_synthetic_mini_turbo():
    import torch
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    from r3g import ffi
    pipe = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained("synthetic:mini-turbo")
    assert pipe.model.guidance_embed and pipe.cfg["sched"]["kind"] == "ConsistencyFlowMatchEulerDiscreteScheduler"
    imgs = _crops(3)
    kw = dict(num_inference_steps=5, octree_resolution=64, output_type="trimesh")
    e0, g0 = ffi.counter("dit_evals"), ffi.counter("dit_groups")
    dense = pipe(image=imgs, generator=torch.manual_seed(7), **kw)
    assert ffi.counter("dit_evals") - e0 == 5 and ffi.counter("dit_groups") - g0 == 1       # 3 objects, one group, 5 evaluations
    _check_meshes(dense, 3)
    grid_dense = pipe.last_grid.clone()
    assert torch.isfinite(grid_dense).all()
    pipe.enable_flashvdm()
    hier = pipe(image=imgs, generator=torch.manual_seed(7), **kw)
    _check_meshes(hier, 3)
    assert torch.isfinite(pipe.last_grid).all() and pipe.last_hier_stats is not None
    pipe.enable_flashvdm(False)
    one = pipe(image=imgs[0], generator=torch.manual_seed(7), **kw)
    _check_meshes(one, 1)
    # the sigmas= keyword is honoured (another table, another grid) and validated
    pipe(image=imgs[2], generator=torch.manual_seed(7), sigmas=[0.0, 0.3, 0.6], **kw)
    assert not torch.equal(pipe.last_grid, grid_dense)
    with pytest.raises(ValueError):
        pipe(image=imgs[0], sigmas=[0.6, 0.3], **kw)


def _write_snapshot(tmp_path, sub_name, drop=None):
    import yaml
    from safetensors.torch import save_file
    from oracle import hy3d_torch as H
    from test_host_cpu import _snapshot_doc
    cfg = R.distilled_cfg(H.tiny_config())
    sd = {k: v.contiguous() for k, v in bf16_round_matrices(R.synthetic_state_dict(cfg, 5)).items() if k != drop}
    doc = _snapshot_doc(cfg)
    doc["scheduler"] = {"target": "hy3dgen.shapegen.schedulers.ConsistencyFlowMatchEulerDiscreteScheduler",
                        "params": {"num_train_timesteps": 1000, "pcm_timesteps": 100}}
    sub = tmp_path / sub_name
    sub.mkdir(parents=True)
    (sub / "config.yaml").write_text(yaml.safe_dump(doc))
    save_file(sd, str(sub / "model.fp16.safetensors"))
    return cfg, sd


def test_from_pretrained_turbo_snapshot_directory(tmp_path):
    import torch
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    cfg, sd = _write_snapshot(tmp_path, "hunyuan3d-dit-v2-0-turbo")
    pipe = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained(str(tmp_path), subfolder="hunyuan3d-dit-v2-0-turbo", variant="fp16")
    assert pipe.model.guidance_embed and pipe.cfg["sched"]["kind"] == "ConsistencyFlowMatchEulerDiscreteScheduler"
    imgs = _crops(3)
    kw = dict(num_inference_steps=5, octree_resolution=64, output_type="trimesh")
    _check_meshes(pipe(image=imgs, generator=torch.manual_seed(7), **kw), 3)
    grid = pipe.last_grid.clone()
    # the latents behind that grid are the restatement's sampler on the same tensors (third object of the list)
    ref = R.load_dit(cfg, sd)
    cond2 = pipe._encode_prepared(pipe._prepared([imgs[2]])[0])
    lat0 = pipe._latents_for(torch.manual_seed(7), 3)[2:3]
    want = R.sample(ref, cond2[:1].float().cpu(), lat0.cpu().clone(), R.consistency_sigmas(5), 5.0)
    got = pipe.model.flow_sample_sigmas(lat0.clone(), cond2[None], R.consistency_sigmas(5), 5.0).cpu()
    assert rel_l2(got, want) <= TOL["flow_sample"]
    pipe.model.vae_decode(got[0])
    assert torch.equal(pipe.model.grid_query(1.01, 64), grid)
    pipe.enable_flashvdm()
    _check_meshes(pipe(image=imgs, generator=torch.manual_seed(7), **kw), 3)
    assert torch.isfinite(pipe.last_grid).all()


def test_snapshot_with_a_missing_guidance_tensor_names_it(tmp_path):
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    from r3g import ffi
    from r3g import model as M
    _write_snapshot(tmp_path, "hunyuan3d-dit-v2-0-turbo", drop="model.guidance_in.out_layer.bias")
    with pytest.raises(KeyError, match="model.guidance_in.out_layer.bias"):
        Hunyuan3DDiTFlowMatchingPipeline.from_pretrained(str(tmp_path), subfolder="hunyuan3d-dit-v2-0-turbo", variant="fp16")
    # and the library itself, given a partial set, fails at the first forward with the key in its message
    s = DSetup.__new__(DSetup)
    s.cfg, _ = _cfg("tiny")
    s.cfg = R.distilled_cfg(s.cfg)
    sd = bf16_round_matrices(R.synthetic_state_dict(s.cfg, 5))
    gpu = M.ShapeModel(s.cfg, sd, 0, grid_chunk=4096)
    del gpu._w["model.guidance_in.out_layer.bias"]
    gpu._install()
    x, cond2 = _inputs(s, 1)
    with pytest.raises(ffi.R3GError, match="model.guidance_in.out_layer.bias"):
        gpu.flow_sample_sigmas(x.clone(), cond2, R.table(2, True), G)


def test_stage_script_writes_glbs_with_the_turbo_variant(tmp_path):
    import yaml
    from r3g.mesh import load_glb
    inp, out = tmp_path / "prepped", tmp_path / "out"
    inp.mkdir()
    for i, im in enumerate(_crops(3)):
        im.save(inp / ("obj__(%d, %d).png" % (i, i)))
    cfg = {"mini": True, "num_inf_steps_hy": 5, "octree_resolution_hy": 64, "num_chunks_hy": 16000, "seed": 1234567,
           "remesh": False, "input_folder_hy": str(inp), "output_folder_hy": str(out), "use_banana": False,
           "prepped_for_hunyuan": str(tmp_path / "unused"), "jobs_per_gpu": 1, "use_all_available_cuda": False,
           "r3g_weights": "synthetic:{model}", "r3g_shape_variant": "turbo"}
    cfgp = tmp_path / "config.yaml"
    cfgp.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "3d-re-gen_amd", "stage", "run.py"), "--config", str(cfgp)],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert sorted(os.listdir(out)) == ["obj__(%d, %d)" % (i, i) for i in range(3)]
    rep = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"stage"')][-1])
    assert rep["ok"] == 3
    for stem in os.listdir(out):
        m = load_glb(str(out / stem / (stem + ".glb")))
        assert len(m.faces) > 0 and np.isfinite(m.vertices).all()
