"""Host side of the guidance-distilled shape models (upstream's -fast / -turbo checkpoints; DESIGN.md section 4b,
[UPSTREAM-RECALLED], parity unpinned): sigma tables, config parsing, checkpoint layout, the stage's `r3g_shape_variant`, the
`sigmas=` keyword -- and the proof that the tolerance the GPU tests apply (tests/parity_support.py TOL["flow_sample"]) is not
vacuous for what a distilled model adds: every wiring hazard of guidance_in / the consistency table moves the restatement's latents
by at least MARGIN x that tolerance."""
import numpy as np
import pytest
import torch
import yaml

import distilled_ref as R
from parity_support import MARGIN, TOL, bf16_round_matrices, dit_inputs, rel_l2


# ---- sigma tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 8, 30, 100])
def test_sigma_tables_equal_the_restatement(n):
    from oracle import hy3d_torch as H
    from r3g import flow
    a = flow.consistency_sigmas(n)
    assert a.dtype == np.float32 and a.shape == (n + 1,)
    assert np.array_equal(a, R.consistency_sigmas(n))
    assert a[-1] == 1.0 and (np.diff(a) > 0).all()              # no step with d_sigma = 0: n steps are n evaluations
    b = flow.euler_sigmas(n)
    assert b.dtype == np.float32 and np.array_equal(b, H.flow_sigmas(n)) and np.array_equal(b, R.linspace_sigmas(n))
    for shift in (1.0, 3.0):
        assert np.array_equal(flow.euler_sigmas(n, shift), H.flow_sigmas(n, shift))
    sched = dict(kind="ConsistencyFlowMatchEulerDiscreteScheduler", num_train_timesteps=1000, pcm_timesteps=100, shift=1.0)
    assert np.array_equal(flow.scheduler_sigmas(sched, n), a)
    assert np.array_equal(flow.scheduler_sigmas(dict(shift=1.0), n), b)           # no kind: the Euler scheduler, as before


def test_consistency_table_worked_examples():
    from r3g import flow
    want = np.array([0, 199 / 999, 399 / 999, 599 / 999, 799 / 999, 1], np.float64).astype(np.float32)
    assert np.array_equal(flow.consistency_sigmas(5), want)
    full = np.linspace(0, 1, 1000)
    idx = np.array([0, 12, 25, 37, 50, 62, 75, 87])
    euler = np.array([0] + [10 * k - 1 for k in range(1, 100)])
    assert euler[1] == 9 and euler[2] == 19 and euler[-1] == 989
    assert np.array_equal(flow.consistency_sigmas(8)[:-1], full[euler[idx]].astype(np.float32))
    with pytest.raises(ValueError):
        flow.consistency_sigmas(0)
    with pytest.raises(ValueError):
        flow.scheduler_sigmas(dict(kind="DDIMScheduler"), 5)


# ---- config ------------------------------------------------------------------------------------------------------------
TURBO_YAML = """
model:
  target: hy3dgen.shapegen.models.Hunyuan3DDiT
  params:
    in_channels: 64
    context_in_dim: 1536
    hidden_size: 1024
    mlp_ratio: 4.0
    num_heads: 16
    depth: 16
    depth_single_blocks: 32
    qkv_bias: true
    time_factor: 1000
    guidance_embed: true
scheduler:
  target: hy3dgen.shapegen.schedulers.ConsistencyFlowMatchEulerDiscreteScheduler
  params:
    num_train_timesteps: 1000
    pcm_timesteps: 100
"""


def test_turbo_config_yaml_is_parsed():
    from hy3dgen.shapegen.pipelines import builtin_config, config_from_yaml
    from r3g import model as M
    cfg = config_from_yaml(yaml.safe_load(TURBO_YAML))
    assert cfg["dit"]["guidance_embed"] is True
    assert cfg["sched"]["kind"] == "ConsistencyFlowMatchEulerDiscreteScheduler"
    assert cfg["sched"]["pcm_timesteps"] == 100 and cfg["sched"]["num_train_timesteps"] == 1000
    assert cfg == builtin_config("full-turbo")
    M.make_config(cfg)                                               # no longer refused
    # the default documents keep today's scheduler; an unknown scheduler class is refused by name
    assert config_from_yaml({})["sched"]["kind"] == "FlowMatchEulerDiscreteScheduler"
    assert config_from_yaml({"scheduler": {"target": "a.b.FlowMatchEulerDiscreteScheduler"}})["sched"]["kind"] == \
        "FlowMatchEulerDiscreteScheduler"
    with pytest.raises(ValueError, match="DDIMScheduler"):
        config_from_yaml({"scheduler": {"target": "diffusers.DDIMScheduler"}})


def test_builtin_distilled_configs():
    from hy3dgen.shapegen.pipelines import builtin_config
    full, mini = builtin_config("full"), builtin_config("mini")
    assert not full["dit"]["guidance_embed"] and full["sched"]["kind"] == "FlowMatchEulerDiscreteScheduler"
    for name, base, kind in (("full-fast", full, "FlowMatchEulerDiscreteScheduler"),
                             ("full-turbo", full, "ConsistencyFlowMatchEulerDiscreteScheduler"),
                             ("mini-turbo", mini, "ConsistencyFlowMatchEulerDiscreteScheduler")):
        c = builtin_config(name)
        assert c["dit"]["guidance_embed"] is True and c["sched"]["kind"] == kind
        c["dit"]["guidance_embed"] = False
        c["sched"]["kind"] = base["sched"]["kind"]
        assert c == base                                              # nothing else differs
    for bad in ("mini-fast", "turbo", "full-"):
        with pytest.raises(KeyError):
            builtin_config(bad)


# ---- checkpoint layout -------------------------------------------------------------------------------------------------
def test_guidance_keys_come_after_every_existing_key():
    """synthetic_state_dict draws from one generator in param_shapes' order: a distilled synthetic checkpoint minus
    guidance_in.* IS the undistilled one of the same seed"""
    from oracle import hy3d_torch as H
    from r3g import model as M
    from r3g import weights as W
    cfg = H.tiny_config()
    dcfg = R.distilled_cfg(cfg)
    a, b = W.param_shapes(cfg), W.param_shapes(dcfg)
    assert list(b)[:len(a)] == list(a) and tuple(list(b)[len(a):]) == W.GUIDANCE_KEYS == R.GUIDANCE_KEYS
    Hd = cfg["dit"]["hidden_size"]
    assert [b[k] for k in W.GUIDANCE_KEYS] == [(Hd, 256), (Hd,), (Hd, Hd), (Hd,)]
    sa, sb = W.synthetic_state_dict(cfg, 7, device="cpu"), W.synthetic_state_dict(dcfg, 7, device="cpu")
    assert set(sb) - set(sa) == set(W.GUIDANCE_KEYS)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(float(sb[k].abs().max()) > 0 for k in W.GUIDANCE_KEYS)
    # the restatement loads the product's distilled checkpoint key for key
    R.load_dit(dcfg, sb)
    # config and checkpoint must agree, and a partial set names the missing key
    M.check_guidance_keys(cfg, sa)
    M.check_guidance_keys(dcfg, sb)
    part = {k: v for k, v in sb.items() if k != "model.guidance_in.out_layer.bias"}
    with pytest.raises(KeyError, match="model.guidance_in.out_layer.bias"):
        M.check_guidance_keys(dcfg, part)
    with pytest.raises(ValueError, match="guidance_embed"):
        M.check_guidance_keys(cfg, sb)


# ---- stage ---------------------------------------------------------------------------------------------------------------
def test_stage_shape_variant():
    from stage import run
    key, model = run.select_model({"mini": True})
    assert key == "mini" and model["args"] == {"subfolder": "hunyuan3d-dit-v2-mini", "variant": "fp16"}
    assert run.select_model({"mini": False})[1]["args"] == {}
    key, model = run.select_model({"mini": True, "r3g_shape_variant": "turbo"})
    assert key == "mini" and model["args"] == {"subfolder": "hunyuan3d-dit-v2-mini-turbo", "variant": "fp16"}
    assert run.select_model({"mini": False, "r3g_shape_variant": "turbo"})[1]["args"] == {"subfolder": "hunyuan3d-dit-v2-0-turbo"}
    assert run.select_model({"mini": False, "r3g_shape_variant": "fast"})[1]["args"] == {"subfolder": "hunyuan3d-dit-v2-0-fast"}
    for bad in ({"mini": True, "r3g_shape_variant": "fast"}, {"mini": False, "r3g_shape_variant": "lightning"}):
        with pytest.raises(ValueError, match="r3g_shape_variant"):
            run.select_model(bad)
    cfg = {"mini": True, "r3g_shape_variant": "turbo", "r3g_weights": "synthetic:{model}"}
    assert run.resolve_weights(cfg, *run.select_model(cfg)) == "synthetic:mini-turbo"
    cfg = {"mini": False, "r3g_weights": "synthetic:{model}"}
    assert run.resolve_weights(cfg, *run.select_model(cfg)) == "synthetic:full"
    # a distilled model lifts the default group to 8; an explicit key wins; absent means today's behaviour
    assert run.objects_per_launch({}) == 4
    assert run.objects_per_launch({"r3g_shape_variant": "turbo"}) == 8
    assert run.objects_per_launch({"r3g_shape_variant": "turbo", "r3g_objects_per_launch": 3}) == 3


# ---- sigmas= --------------------------------------------------------------------------------------------------------------
def test_sigmas_keyword_is_validated():
    from hy3dgen.shapegen.pipelines import Hunyuan3DDiTPipeline, builtin_config
    from r3g import flow
    got = flow.explicit_sigmas([0.0, 0.25, 0.5])
    assert got.dtype == np.float32 and np.array_equal(got, np.array([0, 0.25, 0.5, 1], np.float32))
    assert np.array_equal(flow.explicit_sigmas(np.linspace(0, 1, 6)), flow.euler_sigmas(6))       # ending AT 1: 1, 1 as upstream
    assert np.array_equal(flow.explicit_sigmas(np.linspace(0, 1, 6), 3.0), flow.euler_sigmas(6, 3.0))
    for bad in ([], [0.5, 0.2], [0.0, 0.5, 0.5], [0.0, 1.5], [-0.1, 0.5], [0.0, float("nan")], [[0.0, 0.5]], "abc", [0.0, None]):
        with pytest.raises(ValueError):
            flow.explicit_sigmas(bad)
    # the pipeline refuses a bad table before it touches the device
    pipe = Hunyuan3DDiTPipeline.__new__(Hunyuan3DDiTPipeline)
    pipe.cfg = builtin_config("mini-turbo")
    with pytest.raises(ValueError, match="ascending"):
        pipe(image=object(), sigmas=[0.5, 0.2])


# ---- the tolerance is not vacuous ----------------------------------------------------------------------------------------
def _mutation_setup(which):
    from oracle import hy3d_torch as H
    if which == "tiny":
        cfg, seed = H.tiny_config(), 3
    else:
        cfg, seed = H.mini_config(), 41
        cfg["dit"].update(depth=1, depth_single_blocks=2)
        cfg["vae"].update(num_decoder_layers=1)
        cfg["cond"].update(num_hidden_layers=1)
    cfg = R.distilled_cfg(cfg)
    sd = bf16_round_matrices(R.synthetic_state_dict(cfg, seed))
    return cfg, R.load_dit(cfg, sd)


@pytest.mark.parametrize("which", ["tiny", "mini-dims"])
def test_every_distillation_hazard_is_outside_the_tolerance(which):
    """5 consistency steps, g = 5, unit-scale checkpoints: guidance_in dropped, g - 1 instead of g, time_factor not applied to g,
    the linspace table instead of the consistency table -- each must move the latents by >= 5 x TOL["flow_sample"] = 0.1 (measured
    when this was written, tiny / mini-dims: 0.53 / 0.65, 0.99 / 0.78, 1.08 / 0.86, 0.32 / 0.35; the sampler itself moves them by
    1.1 - 1.4)"""
    cfg, model = _mutation_setup(which)
    x, _, cond = dit_inputs(cfg, 2, batch=1)
    ref = R.sample(model, cond, x.clone(), R.table(5, True), 5.0)
    assert torch.isfinite(ref).all() and rel_l2(ref, x) > 0.3
    for mut in R.MUTATIONS:
        model.mutate = mut if mut != "linspace_table" else None
        got = R.sample(model, cond, x.clone(), R.table(5, True, mut), 5.0)
        model.mutate = None
        d = rel_l2(got, ref)
        print("%s %-22s rel-L2 %.3f" % (which, mut, d))
        assert d >= MARGIN * TOL["flow_sample"], (which, mut, d)


# ---- out of scope, said where a user meets it ---------------------------------------------------------------------------
def test_verify_checkpoint_declines_a_distilled_snapshot(tmp_path):
    """tools/verify_checkpoint.py on a snapshot whose config.yaml says guidance_embed: true: one clear sentence and a non-zero
    exit, not a traceback"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sub = tmp_path / "hunyuan3d-dit-v2-0-turbo"
    sub.mkdir()
    (sub / "config.yaml").write_text(TURBO_YAML)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "verify_checkpoint.py"), str(tmp_path), "--subfolder",
                        "hunyuan3d-dit-v2-0-turbo", "--keys-only"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "guidance-distilled" in r.stderr and "Traceback" not in r.stderr and len(r.stderr.strip().splitlines()) == 1
