"""Host side of the turbo shape VAE (a narrow geo decoder behind latents_proj, and the VAE swap; DESIGN.md section 4e,
[UPSTREAM-RECALLED], parity unpinned): config parsing, checkpoint layout, the VAE-only snapshot loader, the key check -- and the proof
that the tolerance the GPU tests apply (tests/parity_support.py TOL["grid_logits"]) is not vacuous for what the narrow decoder adds:
each wiring hazard of latents_proj / heads_g moves the restatement's logits by at least MARGIN x that tolerance."""
import contextlib
import os

import pytest
import torch
import yaml

import turbo_vae_ref as R
from parity_support import MARGIN, TOL, bf16_round_matrices

G = "vae.geo_decoder."
X = G + "cross_attn_decoder."


def _full_turbo():
    from hy3dgen.shapegen import pipelines as P
    from r3g import weights as W
    cfg = P.builtin_config("full")
    cfg["vae"] = W.turbo_vae_config(cfg["vae"])
    return cfg


# ---- config ------------------------------------------------------------------------------------------------------------
def test_config_from_yaml_carries_the_ratio():
    from hy3dgen.shapegen import pipelines as P
    doc = yaml.safe_load("""
vae:
  target: hy3dgen.shapegen.models.ShapeVAE
  params:
    num_latents: 3072
    width: 1024
    heads: 16
    geo_decoder_downsample_ratio: 4
    geo_decoder_mlp_expand_ratio: 1
    geo_decoder_ln_post: false
""")
    v = P.config_from_yaml(doc)["vae"]
    assert v["geo_decoder_downsample_ratio"] == 4 and v["geo_decoder_mlp_expand_ratio"] == 1 and v["geo_decoder_ln_post"] is False
    # absent in the yaml: absent in the config (every existing config stays as it was), and that means ratio 1
    from r3g import weights as W
    plain = P.config_from_yaml({"vae": {"params": {"width": 1024}}})["vae"]
    assert "geo_decoder_downsample_ratio" not in plain and W.geo_decoder_ratio(plain) == 1 and W.geo_decoder_width(plain) == 1024
    bad = dict(plain, geo_decoder_downsample_ratio=3)
    with pytest.raises(ValueError):
        W.geo_decoder_ratio(bad)


def test_param_shapes_of_the_turbo_decoder():
    from r3g import weights as W
    s = W.param_shapes(_full_turbo())
    assert s[G + "query_proj.weight"] == (256, 51)
    assert s[G + "latents_proj.weight"] == (256, 1024) and s[G + "latents_proj.bias"] == (256,)
    assert s[X + "attn.c_kv.weight"] == (512, 256) and s[X + "attn.c_q.weight"] == (256, 256)
    assert s[X + "mlp.c_fc.weight"] == (256, 256) and s[X + "mlp.c_proj.weight"] == (256, 256)
    assert s[X + "ln_1.weight"] == s[X + "ln_2.weight"] == s[X + "ln_3.weight"] == (256,)
    assert s[G + "output_proj.weight"] == (1, 256)
    assert not any("ln_post" in k for k in s)
    assert not any(k.startswith(G) and ("q_norm" in k or "k_norm" in k) for k in s)
    assert list(s)[-2:] == [G + "latents_proj.weight", G + "latents_proj.bias"]           # after EVERY other key
    # the transformer keeps the VAE's own width
    assert s["vae.transformer.resblocks.0.attn.c_qkv.weight"] == (3072, 1024) and s["vae.post_kl.weight"] == (1024, 64)


# what param_shapes returned for the geo decoder before the ratio existed (literal: the parent's rule, W everywhere)
def _parent_geo_shapes(v):
    Wd, e, hd = v["width"], v.get("geo_decoder_mlp_expand_ratio", 4), v["width"] // v["heads"]
    out = [(G + "query_proj.weight", (Wd, 51)), (G + "query_proj.bias", (Wd,)), (X + "attn.c_q.weight", (Wd, Wd)),
           (X + "attn.c_kv.weight", (2 * Wd, Wd)), (X + "attn.c_proj.weight", (Wd, Wd)), (X + "attn.c_proj.bias", (Wd,))]
    for n in ("q_norm", "k_norm"):
        out += [(X + "attn.attention.%s.weight" % n, (hd,)), (X + "attn.attention.%s.bias" % n, (hd,))]
    for n in ("ln_1", "ln_2", "ln_3"):
        out += [(X + n + ".weight", (Wd,)), (X + n + ".bias", (Wd,))]
    out += [(X + "mlp.c_fc.weight", (e * Wd, Wd)), (X + "mlp.c_fc.bias", (e * Wd,)), (X + "mlp.c_proj.weight", (Wd, e * Wd)),
            (X + "mlp.c_proj.bias", (Wd,)), (G + "ln_post.weight", (Wd,)), (G + "ln_post.bias", (Wd,)),
            (G + "output_proj.weight", (1, Wd)), (G + "output_proj.bias", (1,))]
    return out


@pytest.mark.parametrize("name", ["full", "tiny"])
def test_ratio_one_is_the_parents_checkpoint(name):
    """r = 1 (key absent, or written as 1): the same keys in the same order and, for a seed, the same synthetic tensors -- and the keys
    are exactly the oracle's (which knows no ratio), in its order"""
    from hy3dgen.shapegen import pipelines as P
    from oracle import hy3d_torch as H
    from r3g import weights as W
    cfg = P.builtin_config("full") if name == "full" else H.tiny_config()
    one = dict(cfg, vae=dict(cfg["vae"], geo_decoder_downsample_ratio=1))
    a, b = W.param_shapes(cfg), W.param_shapes(one)
    assert list(a.items()) == list(b.items())
    assert not any("latents_proj" in k for k in a)
    geo = [(k, v) for k, v in a.items() if k.startswith(G)]
    assert geo == _parent_geo_shapes(cfg["vae"])
    if name == "tiny":
        ref = H.ShapePipeline(cfg)
        vae_keys = ["vae." + k for k in ref.vae.state_dict()]
        assert sorted(k for k in a if k.startswith("vae.")) == sorted(vae_keys)
        sa, sb = W.synthetic_state_dict(cfg, 5, device="cpu"), W.synthetic_state_dict(one, 5, device="cpu")
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
        # ... and a ratio changes nothing in front of the geo decoder: same generator, same order, same draws
        two = dict(cfg, vae=dict(cfg["vae"], geo_decoder_downsample_ratio=2))
        sc = W.synthetic_state_dict(two, 5, device="cpu")
        first_geo = list(sa).index(G + "query_proj.weight")
        for k in list(sa)[:first_geo]:
            assert torch.equal(sa[k], sc[k]), k
        assert list(sc)[-2:] == [G + "latents_proj.weight", G + "latents_proj.bias"]


def test_restatement_names_equal_vae_param_shapes():
    from oracle import hy3d_torch as H
    from r3g import weights as W
    for vcfg in (R.turbo_vae_cfg(H.tiny_config()["vae"], ratio=2), W.turbo_vae_config(H.wide_config()["vae"]), H.tiny_config()["vae"]):
        shapes = W.vae_param_shapes(vcfg)
        vae = R.TurboShapeVAE(**vcfg)
        want = {"vae." + k: tuple(p.shape) for k, p in vae.state_dict().items()}
        assert shapes == want
        sd = W.synthetic_vae_state_dict(vcfg, 3, device="cpu")
        R.load_vae(vcfg, sd)                                                  # strict
        again = W.synthetic_vae_state_dict(vcfg, 3, device="cpu")
        assert all(torch.equal(sd[k], again[k]) for k in sd)
    # 'synthetic:turbo-vae' is the pipeline's own VAE dims with r = 4, e = 1, no ln_post
    t = W.turbo_vae_config(H.wide_config()["vae"])
    assert (t["geo_decoder_downsample_ratio"], t["geo_decoder_mlp_expand_ratio"], t["geo_decoder_ln_post"]) == (4, 1, False)
    assert t["width"] == 1024 and t["num_latents"] == 3072


# ---- the VAE-only snapshot folder ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,spelling", [("safetensors", "params"), ("ckpt", "params"), ("safetensors", "vae.params"), ("ckpt", "vae.params")])
def test_load_vae_dir_round_trip(tmp_path, fmt, spelling):
    from oracle import hy3d_torch as H
    from r3g import weights as W
    vcfg = R.turbo_vae_cfg(H.tiny_config()["vae"], ratio=2)
    sd = R.synthetic_vae_state_dict(vcfg, 11)
    bare = {k[4:]: v.contiguous() for k, v in sd.items()}                     # a VAE-only snapshot's keys carry no prefix
    bare["encoder.cross_attn.ln_1.weight"] = torch.ones(8)                    # the encoder side travels with it and is ignored
    bare["pre_kl.weight"] = torch.ones(4, 4)
    d = tmp_path / "hunyuan3d-vae-v2-0-turbo"
    d.mkdir()
    doc = {"target": "hy3dgen.shapegen.models.ShapeVAE", "params": dict(vcfg)}
    (d / "config.yaml").write_text(yaml.safe_dump(doc if spelling == "params" else {"vae": doc}))
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(bare, str(d / "model.fp16.safetensors"))
    else:
        torch.save(bare, str(d / "model.fp16.ckpt"))
    params, got = W.load_vae_dir(str(d), "fp16", use_safetensors=(fmt == "safetensors"))
    assert params == vcfg
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert set(got) == set(W.vae_param_shapes(params))
    R.load_vae(params, got)
    if fmt == "ckpt":                                                         # no safetensors file there: the .ckpt is found anyway
        assert sorted(W.load_vae_dir(str(d), "fp16", use_safetensors=True)[1]) == sorted(sd)
    with pytest.raises(FileNotFoundError):
        W.load_vae_dir(str(tmp_path), "fp16")


def test_check_geo_decoder_keys_each_way():
    from oracle import hy3d_torch as H
    from r3g import model as M
    cfg = H.tiny_config()
    narrow = dict(cfg, vae=R.turbo_vae_cfg(cfg["vae"], ratio=2))
    sd = R.synthetic_vae_state_dict(narrow["vae"], 1)
    M.check_geo_decoder_keys(narrow, sd)
    M.check_geo_decoder_keys(cfg, {k: v for k, v in sd.items() if "latents_proj" not in k})
    with pytest.raises(KeyError) as e:
        M.check_geo_decoder_keys(narrow, {k: v for k, v in sd.items() if "latents_proj" not in k})
    assert "vae.geo_decoder.latents_proj.weight" in str(e.value)
    with pytest.raises(KeyError) as e:
        M.check_geo_decoder_keys(narrow, {k: v for k, v in sd.items() if k != G + "latents_proj.bias"})
    assert "vae.geo_decoder.latents_proj.bias" in str(e.value)
    with pytest.raises(ValueError) as e:
        M.check_geo_decoder_keys(cfg, sd)
    assert "latents_proj" in str(e.value) and "geo_decoder_downsample_ratio" in str(e.value)


# ---- the tolerance of the GPU tests is not vacuous ----------------------------------------------------------------------------
def test_wiring_hazards_of_the_narrow_decoder_are_detectable():
    """tiny VAE, r = 2 (width_g 64, one head), e = 1, no ln_post -- the smallest case of the GPU test -- on bf16-representable weights:
    each hazard moves max|d| / max|logit| of a 500-point slice by >= MARGIN x TOL["grid_logits"]"""
    from oracle import hy3d_torch as H
    vcfg = R.turbo_vae_cfg(H.tiny_config()["vae"], ratio=2)
    vae = R.load_vae(vcfg, bf16_round_matrices(R.synthetic_vae_state_dict(vcfg, 4)))
    lat = torch.randn(vcfg["num_latents"], vcfg["embed_dim"], generator=torch.Generator().manual_seed(2))
    z = R.decode(vae, lat)
    ref = R.logits(vae, z, 1.01, 24, 5000, 500)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    dec = vae.geo_decoder
    for hazard in ("mut_skip_bias", "mut_proj_after_ln2", "mut_full_heads"):
        setattr(dec, hazard, True)
        try:
            got = R.logits(vae, z, 1.01, 24, 5000, 500)
        finally:
            setattr(dec, hazard, False)
        d = float((got - ref).abs().max() / ref.abs().max())
        assert d >= MARGIN * TOL["grid_logits"], (hazard, d)
    assert torch.equal(R.logits(vae, z, 1.01, 24, 5000, 500), ref)            # the switches restore what they touch


# ---- enable_flashvdm keeps its hands off the VAE ------------------------------------------------------------------------------
def test_enable_flashvdm_replace_vae_leaves_the_vae_alone():
    import ref_shim
    from hy3dgen.shapegen import pipelines as pl
    from oracle import hy3d_torch as H

    class CpuPipeline(pl.Hunyuan3DDiTFlowMatchingPipeline):
        def _make_model(self, cfg, state_dict, grid_chunk):
            return ref_shim.OracleModel(cfg, state_dict, grid_chunk)

        def _device_ctx(self):
            return contextlib.nullcontext()

    cfg = H.tiny_config()
    p = CpuPipeline(cfg, H.synthetic_state_dict(cfg, seed=2), "cuda:0")
    before = {k: v.clone() for k, v in p.model.pipe.vae.state_dict().items()}
    vcfg = dict(p.cfg["vae"])
    p.enable_flashvdm(replace_vae=True)
    p.enable_flashvdm(enabled=False, replace_vae=True)
    after = p.model.pipe.vae.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert p.cfg["vae"] == vcfg and "vae" not in p.timings
    # the swap is a method of its own, and the switch's docstring says so
    assert callable(getattr(p, "replace_vae", None))
    assert "replace_vae(" in pl.Hunyuan3DDiTFlowMatchingPipeline.enable_flashvdm.__doc__
    with pytest.raises(KeyError):
        p.replace_vae("synthetic:no-such-vae")
    with pytest.raises(FileNotFoundError):
        p.replace_vae(os.path.join(os.sep, "no", "such", "snapshot"))


def test_stage_keys(monkeypatch):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("r3g_stage_run_turbo", os.path.join(root, "3d-re-gen_amd", "stage", "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    monkeypatch.delenv("R3G_TURBO_VAE", raising=False)
    assert run.turbo_vae({}) is None

    class P:
        calls = []

        def replace_vae(self, path, subfolder="x"):
            self.calls.append((path, subfolder))
    p = P()
    run.apply_turbo_vae({}, p)
    assert p.calls == []                                                      # without the key nothing changes
    run.apply_turbo_vae({"r3g_turbo_vae": "synthetic:turbo-vae"}, p)
    run.apply_turbo_vae({"r3g_turbo_vae": "/snap", "r3g_turbo_vae_subfolder": "hunyuan3d-vae-v2-mini-turbo"}, p)
    monkeypatch.setenv("R3G_TURBO_VAE", "/from-env")
    run.apply_turbo_vae({}, p)
    assert p.calls == [("synthetic:turbo-vae", "hunyuan3d-vae-v2-0-turbo"), ("/snap", "hunyuan3d-vae-v2-mini-turbo"),
                       ("/from-env", "hunyuan3d-vae-v2-0-turbo")]
    with pytest.raises(ValueError):
        run.turbo_vae({"r3g_turbo_vae": 4})
