"""The turbo shape VAE on the GPU: a geo decoder at width // r behind latents_proj -- the generic launches
for any width_g that is a multiple of 64, the fused tail (csrc/geo_narrow.hip) for width_g 256 -- and the VAE swap of the pipeline,
against the PyTorch restatement tests/turbo_vae_ref.py on bf16-representable weights.  Tolerances are the suite's
(tests/parity_support.py); tests/test_turbo_vae_cpu.py shows that the hazards of the new pieces move the same metric by >= 5x of them.
The bit-equalities (query-side cache, listed points, top-k with every key, the swap) are the existing invariants at heads_g.
"""
import ctypes

import pytest

import turbo_vae_ref as R
from parity_support import TOL, bf16_round_matrices, rel_l2, report

pytestmark = pytest.mark.gpu

BOUND = 1.01


@pytest.fixture(scope="module")
def base():
    """DiT + conditioner of the tiny config (the DiT never runs here except in the pipeline test)"""
    from oracle import hy3d_torch as H
    cfg = H.tiny_config()
    sd = {k: v for k, v in H.synthetic_state_dict(cfg, seed=3).items() if not k.startswith("vae.")}
    return cfg, sd


class Case:
    def __init__(self, base, vae_update, seed, grid_chunk=4096):
        import torch
        from r3g import model as M
        cfg0, sd0 = base
        cfg = dict(cfg0, vae=dict(cfg0["vae"], **vae_update))
        if cfg["vae"].get(R.RATIO_KEY, 1) == 1:
            cfg["vae"].pop(R.RATIO_KEY, None)
        sd = dict(sd0)
        sd.update(R.synthetic_vae_state_dict(cfg["vae"], seed))
        self.cfg, self.sd = cfg, bf16_round_matrices(sd)
        self.vae = R.load_vae(cfg["vae"], self.sd)
        self.gpu = M.ShapeModel(cfg, self.sd, 0, grid_chunk=grid_chunk)
        self.N, self.C = cfg["vae"]["num_latents"], cfg["vae"]["embed_dim"]
        self.torch = torch

    def latents(self, seed):
        return self.torch.randn(self.N, self.C, generator=self.torch.Generator().manual_seed(seed))

    def slice_error(self, z_ref, R_, start, count):
        ref = R.logits(self.vae, z_ref, BOUND, R_, start, count)
        out = self.torch.zeros((R_ + 1) ** 3, device="cuda")
        self.gpu.grid_query(BOUND, R_, out=out, start=start, count=count)
        got = out[start:start + count].cpu()
        assert self.torch.isfinite(got).all()
        return (got - ref).abs().max().item() / ref.abs().max().item(), got


def _opt(name, value):
    from r3g import ffi
    ffi.check(ffi.lib().r3g_set_option(name.encode(), int(value)))


# ---- the generic path at its smallest -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,update", [
    ("r=2 e=1 no ln_post (width_g 64, one head)", {R.RATIO_KEY: 2, "geo_decoder_mlp_expand_ratio": 1, "geo_decoder_ln_post": False}),
    ("r=1 e=4 ln_post, 200 latents (keys padded to 256)", {R.RATIO_KEY: 1, "geo_decoder_mlp_expand_ratio": 4, "geo_decoder_ln_post": True,
                                                         "num_latents": 200}),
])
def test_generic_path_smallest(base, tag, update):
    c = Case(base, update, 21)
    lat = c.latents(7)
    z_ref = R.decode(c.vae, lat)
    z = c.gpu.vae_decode(lat, return_z=True)
    err = rel_l2(z, z_ref[0])
    report("turbo vae: latents, " + tag, err, TOL["vae_latents"])
    assert err <= TOL["vae_latents"]
    d, _ = c.slice_error(z_ref, 24, 25 * 25 * 9 + 123, 3000)
    report("turbo vae: grid logits (24^3 slice), " + tag, d, TOL["grid_logits"])
    assert d <= TOL["grid_logits"]


# ---- the fused tail in isolation ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_weights():
    """per hidden size: unit-scale bf16 weights and fp32 vectors of the chain, on the device, and float64 copies"""
    import torch
    out = {}
    for hidden in (256, 1024):
        g = torch.Generator().manual_seed(100 + hidden)

        def mat(n, k):
            return (torch.randn(n, k, generator=g) / k ** 0.5).to(torch.bfloat16)

        def vec(n, scale=0.1, mean=0.0):
            return mean + scale * torch.randn(n, generator=g)
        w = dict(w_proj=mat(256, 256), b_proj=vec(256), ln3_w=vec(256, 0.1, 1.0), ln3_b=vec(256), w_fc=mat(hidden, 256), b_fc=vec(hidden),
                 w_fp=mat(256, hidden), b_fp=vec(256), lnp_w=vec(256, 0.1, 1.0), lnp_b=vec(256), out_w=vec(256, 1 / 16.0), out_b=0.173)
        out[hidden] = (w, {k: (v.cuda().contiguous() if torch.is_tensor(v) else v) for k, v in w.items()})
    return out


def _tail_reference(w, cat, x0, ln_post):
    """the chain in float64 from the same bf16 inputs, no rounding in between"""
    import torch
    import torch.nn.functional as F
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in w.items()}
    x1 = x0.double() + F.linear(cat.double(), d["w_proj"], d["b_proj"])
    h = F.gelu(F.linear(F.layer_norm(x1, (256,), d["ln3_w"], d["ln3_b"], 1e-6), d["w_fc"], d["b_fc"]))
    x2 = x1 + F.linear(h, d["w_fp"], d["b_fp"])
    if ln_post:
        x2 = F.layer_norm(x2, (256,), d["lnp_w"], d["lnp_b"], 1e-5)
    return x2 @ d["out_w"] + d["out_b"]


@pytest.mark.parametrize("ln_post", [True, False])
@pytest.mark.parametrize("hidden", [256, 1024])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_fused_tail_in_isolation(tail_weights, n, hidden, ln_post):
    import torch
    from r3g import ffi
    L = ffi.lib()
    w, dw = tail_weights[hidden]
    g = torch.Generator().manual_seed(1000 * n + hidden + int(ln_post))
    pad = 72                                                      # rows behind n: past the 64-row and the 128-row tile
    cat = torch.randn(n + pad, 256, generator=g).to(torch.bfloat16)
    x0 = torch.randn(n + pad, 256, generator=g).to(torch.bfloat16)
    ref = _tail_reference(w, cat[:n], x0[:n], ln_post)
    SENTINEL = -12345.5

    def run(cat_h, x0_h):
        dc, dx = cat_h.cuda().contiguous(), x0_h.cuda().contiguous()
        out = torch.full((n + pad,), SENTINEL, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        ffi.check(L.r3g_op_geo_tail(p(dc), p(dx), n, hidden, p(dw["w_proj"]), p(dw["b_proj"]), p(dw["ln3_w"]), p(dw["ln3_b"]),
                                    p(dw["w_fc"]), p(dw["b_fc"]), p(dw["w_fp"]), p(dw["b_fp"]),
                                    p(dw["lnp_w"]) if ln_post else None, p(dw["lnp_b"]) if ln_post else None, p(dw["out_w"]),
                                    float(dw["out_b"]), p(out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return out.cpu()
    out = run(cat, x0)
    assert torch.isfinite(out[:n]).all()
    assert (out[n:] == SENTINEL).all(), "the kernel wrote behind row n"
    d = float((out[:n].double() - ref).abs().max() / ref.abs().max())
    report("turbo vae: fused tail n=%d hidden=%d ln_post=%d" % (n, hidden, ln_post), d, TOL["grid_logits"])
    assert d <= TOL["grid_logits"]
    # rows past n must not influence a valid row
    cat2, x02 = cat.clone(), x0.clone()
    cat2[n:] = float("nan")
    x02[n:] = float("nan")
    out2 = run(cat2, x02)
    assert torch.equal(out2[:n].view(torch.int32), out[:n].view(torch.int32))
    assert (out2[n:] == SENTINEL).all()


def test_fused_tail_refuses_other_shapes():
    import torch
    from r3g import ffi
    L = ffi.lib()
    t = torch.zeros(256, 256, device="cuda", dtype=torch.bfloat16)
    v = torch.zeros(2048, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    for n, hidden in ((0, 256), (4, 128), (4, 2048)):
        rc = L.r3g_op_geo_tail(p(t), p(t), n, hidden, p(t), p(v), p(v), p(v), p(t), p(v), p(t), p(v), None, None, p(v), 0.0, p(v), None)
        assert rc != 0


# ---- fused against generic, in place --------------------------------------------------------------------------------------------------
NARROW = {"width": 512, "heads": 8, "num_decoder_layers": 1, "num_latents": 256, R.RATIO_KEY: 2, "geo_decoder_mlp_expand_ratio": 1,
          "geo_decoder_ln_post": False}


@pytest.fixture(scope="module")
def narrow(base):
    """VAE width 512 / 8 heads / 1 layer, r = 2: a decoder of width 256 with 4 heads, e = 1; passes of 2048 points"""
    c = Case(base, NARROW, 31, grid_chunk=2048)
    yield c
    _opt("geo_narrow_fused", DEFAULT_FUSED)
    _opt("geo_q_cache", 1)
    _opt("geo_fp8", 0)
    c.gpu.set_kv_selection(0, 8192, 64)


DEFAULT_FUSED = 0        # the library's default of option "geo_narrow_fused" (include/r3g.h; profiles/turbo_vae.md)


def test_fused_and_generic_tail_in_place(narrow):
    """a 4 097-point range of a 24^3 grid: two full passes (canonical: their x0 comes from the query-side cache) and a 1-point tail (the
    scratch stream)"""
    import torch
    from r3g import ffi
    c = narrow
    lat = c.latents(5)
    z_ref = R.decode(c.vae, lat)
    c.gpu.vae_decode(lat)
    got = {}
    for fused, passes in ((1, 3), (0, 0)):
        _opt("geo_narrow_fused", fused)
        n0 = ffi.counter("geo_narrow_passes")
        d, got[fused] = c.slice_error(z_ref, 24, 0, 4097)
        assert ffi.counter("geo_narrow_passes") - n0 == passes
        report("turbo vae: width_g 256 grid logits, geo_narrow_fused=%d" % fused, d, TOL["grid_logits"])
        assert d <= TOL["grid_logits"]
        d2, again = c.slice_error(z_ref, 24, 0, 4097)           # the two full passes now come from the cache
        assert torch.equal(again.view(torch.int32), got[fused].view(torch.int32))
    d = float((got[1] - got[0]).abs().max() / got[0].abs().max())
    report("turbo vae: fused against generic tail", d, TOL["same_function"])
    assert d <= TOL["same_function"]


def test_turbo_dimensions_once(base):
    """width 1024 / 16 heads / 3072 latents, r = 4, e = 1, no ln_post (one transformer layer): a slice of the 257^3 grid"""
    c = Case(base, {"width": 1024, "heads": 16, "num_decoder_layers": 1, "num_latents": 3072, R.RATIO_KEY: 4,
                    "geo_decoder_mlp_expand_ratio": 1, "geo_decoder_ln_post": False}, 41)
    lat = c.latents(3)
    z_ref = R.decode(c.vae, lat)
    z = c.gpu.vae_decode(lat, return_z=True)
    err = rel_l2(z, z_ref[0])
    report("turbo vae: latents at turbo dims (1 layer)", err, TOL["vae_latents"])
    assert err <= TOL["vae_latents"]
    try:
        for fused in (1, 0):
            _opt("geo_narrow_fused", fused)
            d, _ = c.slice_error(z_ref, 256, 257 * 257 * 100 + 12345, 3000)
            report("turbo vae: grid logits at turbo dims (257^3 slice), geo_narrow_fused=%d" % fused, d, TOL["grid_logits"])
            assert d <= TOL["grid_logits"]
    finally:
        _opt("geo_narrow_fused", DEFAULT_FUSED)


# ---- the existing invariants at heads_g -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
def test_query_side_cache_with_the_narrow_decoder(narrow, fused):
    import torch
    c, Rr = narrow, 24
    _opt("geo_narrow_fused", fused)
    la, lb = c.latents(8), c.latents(9)
    _opt("geo_q_cache", 0)
    c.gpu.vae_decode(la)
    ref_a = c.gpu.grid_query(BOUND, Rr).clone()
    c.gpu.vae_decode(lb)
    ref_b = c.gpu.grid_query(BOUND, Rr).clone()
    _opt("geo_q_cache", 1)
    c.gpu.vae_decode(la)
    assert torch.equal(c.gpu.grid_query(BOUND, Rr).view(torch.int32), ref_a.view(torch.int32))        # first object: builds
    c.gpu.vae_decode(lb)
    assert torch.equal(c.gpu.grid_query(BOUND, Rr).view(torch.int32), ref_b.view(torch.int32))        # second object: served from it
    assert not torch.equal(ref_a, ref_b)


@pytest.mark.parametrize("fused", [0, 1])
def test_listed_points_and_full_topk_equal_the_dense_grid(narrow, fused):
    """the hierarchical decoder's listed points, and top-k selection with k = num_latents, go through the same pass body"""
    import torch
    c, Rr = narrow, 24
    total = (Rr + 1) ** 3
    _opt("geo_narrow_fused", fused)
    c.gpu.vae_decode(c.latents(10))
    dense = c.gpu.grid_query(BOUND, Rr).reshape(-1).clone()
    lst = torch.sort(torch.randperm(total, generator=torch.Generator().manual_seed(4))[:2048 + 777]).values.to(torch.int32).cuda()
    listed = c.gpu.grid_query_points(BOUND, Rr, lst)
    assert torch.equal(listed.view(torch.int32), dense[lst.long()].view(torch.int32))
    grid, stats = c.gpu.grid_query_hier(BOUND, Rr, 0.0, 1e30, 6)       # a band that refines everything: every point is a listed one
    assert stats["levels"] == [6, 12, 24]
    assert torch.equal(grid.reshape(-1).view(torch.int32), dense.view(torch.int32))
    try:
        assert c.gpu.set_kv_selection(c.N, 1024, 64) == c.N
        full = c.gpu.grid_query(BOUND, Rr).reshape(-1).clone()
        table = c.gpu.kv_selection_last()
        assert table.shape[1] == 4 and table.shape[2] == c.N                                          # heads_g
        q, k = c.gpu.kv_selection_operands()
        assert q.shape[0] == 4 and k.shape[0] == 4
    finally:
        c.gpu.set_kv_selection(0, 8192, 64)
    assert torch.equal(full.view(torch.int32), dense.view(torch.int32))


def test_geo_fp8_is_refused_with_a_narrow_decoder(narrow):
    import torch
    from r3g import ffi
    c = narrow
    c.gpu.vae_decode(c.latents(11))
    before = c.gpu.grid_query(BOUND, 24).clone()
    _opt("geo_fp8", 1)
    try:
        with pytest.raises(ffi.R3GError) as e:
            c.gpu.grid_query(BOUND, 24)
        assert e.value.code == -1 and "geo_fp8" in str(e.value) and "narrow" in str(e.value)
    finally:
        _opt("geo_fp8", 0)
    assert torch.equal(c.gpu.grid_query(BOUND, 24).view(torch.int32), before.view(torch.int32))


def test_library_refuses_a_decoder_it_cannot_run(base):
    """the tensors decide: a query_proj whose rows are no multiple of 64, or a narrow decoder without latents_proj, is an error that
    names the tensor -- not a decoder of some other shape"""
    import torch
    from r3g import ffi
    c = Case(base, {R.RATIO_KEY: 2, "geo_decoder_mlp_expand_ratio": 1, "geo_decoder_ln_post": False}, 51)
    L = ffi.lib()
    lat = c.latents(1)
    c.gpu.vae_decode(lat)
    name = b"vae.geo_decoder.query_proj.weight"
    w = c.gpu._w[name.decode()][0]
    ffi.check(L.r3g_model_set_tensor(c.gpu.ctx, name, w.data_ptr(), 1, 48, w.shape[1]))
    with pytest.raises(ffi.R3GError) as e:
        c.gpu.vae_decode(lat)
    assert e.value.code == -1 and "query_proj.weight" in str(e.value)
    ffi.check(L.r3g_model_set_tensor(c.gpu.ctx, name, w.data_ptr(), 1, w.shape[0], w.shape[1]))
    c.gpu.vae_decode(lat)
    # the host refuses the disagreement before the library sees it
    from r3g import model as M
    with pytest.raises(KeyError):
        M.ShapeModel(c.cfg, {k: v for k, v in c.sd.items() if "latents_proj" not in k}, 0)


# ---- the swap through the pipeline ----------------------------------------------------------------------------------------------------
def test_replace_vae_through_the_pipeline():
    """tiny DiT / conditioner with a VAE wide enough for r = 4 (width 1024 / 16 heads / 1 layer / 256 latents -> a decoder of width 256):
    the swapped pipeline equals one CONSTRUCTED with the merged config and state dict, and swapping the original tensors back restores
    the first grid -- bit for bit"""
    import numpy as np
    import torch
    from PIL import Image
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline as Pipe
    from oracle import hy3d_torch as H
    from r3g import ffi
    from r3g import weights as W
    cfg = H.tiny_config()
    cfg["vae"].update(width=1024, heads=16, num_decoder_layers=1)
    sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=5))
    rng = np.random.default_rng(0)
    arr = np.zeros((80, 80, 4), np.uint8)
    arr[20:60, 15:65, :3] = rng.integers(0, 255, (40, 50, 3))
    arr[20:60, 15:65, 3] = 255
    pil = Image.fromarray(arr, "RGBA")

    def run(p):
        mesh = p(image=pil, num_inference_steps=4, octree_resolution=24, generator=torch.manual_seed(1234567))[0]
        return mesh, p.last_grid.clone()
    pipe = Pipe(cfg, sd, "cuda:0", grid_chunk=2048)
    _, g0 = run(pipe)
    assert pipe.timings["vae"] == "checkpoint"
    dit_ptr = pipe.model._w["model.latent_in.weight"][0].data_ptr()
    builds = ffi.counter("geo_q_cache_builds")
    pipe.replace_vae("synthetic:turbo-vae:7")
    assert pipe.cfg["vae"][R.RATIO_KEY] == 4 and pipe.model.cfg["vae"][R.RATIO_KEY] == 4
    assert pipe.model._w["model.latent_in.weight"][0].data_ptr() == dit_ptr           # the DiT was not uploaded again
    assert tuple(pipe.model._w["vae.geo_decoder.query_proj.weight"][0].shape) == (256, 64)
    mesh, g1 = run(pipe)
    assert pipe.timings["vae"] == "synthetic:turbo-vae:7"
    assert ffi.counter("geo_q_cache_builds") == builds + 1                              # the query-side cache was rebuilt
    assert mesh is not None and len(mesh.faces) > 0
    assert not torch.equal(g1, g0)
    vcfg = W.turbo_vae_config(cfg["vae"])
    merged_cfg = dict(cfg, vae=vcfg)
    merged_sd = {k: v for k, v in sd.items() if not k.startswith("vae.")}
    merged_sd.update(W.synthetic_vae_state_dict(vcfg, 7, device="cuda:0"))
    _, g1c = run(Pipe(merged_cfg, merged_sd, "cuda:0", grid_chunk=2048))
    assert torch.equal(g1c.view(torch.int32), g1.view(torch.int32))
    # a VAE that does not fit the DiT is refused and changes nothing
    with pytest.raises(ValueError):
        pipe.replace_vae_tensors(dict(vcfg, num_latents=512), {})
    pipe.replace_vae_tensors(cfg["vae"], {k: v for k, v in sd.items() if k.startswith("vae.")}, "original")
    _, g2 = run(pipe)
    assert torch.equal(g2.view(torch.int32), g0.view(torch.int32))
    assert pipe.timings["vae"] == "original"
