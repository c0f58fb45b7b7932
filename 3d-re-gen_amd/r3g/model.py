"""Host side of the shape model: configuration, checkpoint -> device weights, and thin methods over
the C ABI (include/r3g.h).  Mirrors what `Hunyuan3DDiTFlowMatchingPipeline.from_pretrained` builds
from config.yaml + model.safetensors (reference src/2d_to_3d_models/run.py:122-124, 204-206).

The state dict uses upstream key names with the 'model.' / 'vae.' / 'conditioner.' prefixes.
"""
import ctypes

import torch

from . import ffi as _l


def swiglu_hidden(hidden_size, mlp_ratio):
    """transformers Dinov2SwiGLUFFN: hidden_features = (int(hidden*mlp_ratio*2/3) + 7) // 8 * 8"""
    return (int(int(hidden_size * mlp_ratio) * 2 / 3) + 7) // 8 * 8


def make_config(cfg, grid_chunk=0):
    d, v, c = cfg["dit"], cfg["vae"], cfg["cond"]
    if not c.get("use_swiglu_ffn", True):
        raise ValueError("only the SwiGLU Dinov2 variant (dinov2-giant) is implemented")
    m = _l.ModelConfig()
    m.dit_in_channels, m.dit_context_dim, m.dit_hidden = d["in_channels"], d["context_in_dim"], d["hidden_size"]
    m.dit_heads, m.dit_depth_double, m.dit_depth_single = d["num_heads"], d["depth"], d["depth_single_blocks"]
    m.dit_mlp_hidden = int(d["hidden_size"] * d["mlp_ratio"])
    m.dit_qkv_bias, m.dit_time_factor = int(d["qkv_bias"]), float(d["time_factor"])
    m.vae_num_latents, m.vae_embed_dim, m.vae_width, m.vae_heads = v["num_latents"], v["embed_dim"], v["width"], v["heads"]
    m.vae_layers, m.vae_num_freqs, m.vae_include_pi = v["num_decoder_layers"], v["num_freqs"], int(v["include_pi"])
    m.vae_qkv_bias, m.vae_qk_norm = int(v["qkv_bias"]), int(v["qk_norm"])
    m.vae_mlp_ratio, m.vae_ln_post = int(v.get("geo_decoder_mlp_expand_ratio", 4)), int(v.get("geo_decoder_ln_post", True))
    m.vae_scale_factor = float(v["scale_factor"])
    m.cond_image_size, m.cond_patch, m.cond_hidden = c["image_size"], c["patch_size"], c["hidden_size"]
    m.cond_layers, m.cond_heads = c["num_hidden_layers"], c["num_attention_heads"]
    m.cond_ffn_hidden = swiglu_hidden(c["hidden_size"], c["mlp_ratio"])
    m.cond_ln_eps = float(c.get("layer_norm_eps", 1e-6))
    m.grid_chunk = int(grid_chunk)
    return m


def kv_topk(topk, num_latents):
    """keys the geo decoder keeps per (group, head) for option "geo_kv_topk" = topk (the library's rule, csrc/kvsel_kernels.h):
    0 = exact attention; -1 = upstream's rule [UPSTREAM-RECALLED], 1024 of 3072 latents, 256 of 512, otherwise a third; k > 0 is
    clamped to num_latents"""
    topk, num_latents = int(topk), int(num_latents)
    if topk < -1:
        raise ValueError("kv_topk: topk is 0 (exact), a key count or -1 (upstream's rule), not %d" % topk)
    if topk == 0:
        return 0
    if topk == -1:
        topk = 1024 if num_latents == 3072 else 256 if num_latents == 512 else num_latents // 3
    return max(1, min(topk, num_latents))


def _pad_k(w):
    n, k = w.shape
    kp = (k + 63) // 64 * 64
    if kp == k:
        return w
    out = torch.zeros((n, kp), dtype=w.dtype, device=w.device)
    out[:, :k] = w
    return out


def prepare_weights(sd, device):
    """upstream state dict -> {name: (tensor on device, dtype code)}; matrices bf16 [N][Kpad64], vectors f32.
    Fusions done here (pure re-layout, no arithmetic): Dinov2 query/key/value -> one qkv matrix; patch conv
    kernel [C,3,p,p] -> [C, 3*p*p]; cls/pos embeddings flattened."""
    out, scalars = {}, {}
    qkv_parts = {}
    for k, t in sd.items():
        if not torch.is_floating_point(t) or k.endswith("mask_token"):
            continue
        t = t.detach()
        if ".attention.attention." in k and k.split(".")[-2] in ("query", "key", "value"):
            base, which, kind = k.rsplit(".", 2)
            qkv_parts.setdefault((base, kind), {})[which] = t
            continue
        if k.endswith("patch_embeddings.projection.weight"):
            t = t.reshape(t.shape[0], -1)
        if k.endswith("cls_token"):
            t = t.reshape(-1)
        if k.endswith("position_embeddings"):
            t = t.reshape(t.shape[-2], t.shape[-1])
        if k.endswith("geo_decoder.output_proj.bias"):
            scalars[k] = float(t.reshape(-1)[0])
            continue
        if k.endswith("geo_decoder.output_proj.weight"):
            out[k] = (t.reshape(1, -1).to(device=device, dtype=torch.float32).contiguous(), 0)
            continue
        if t.ndim == 2 and not k.endswith("position_embeddings"):
            out[k] = (_pad_k(t.to(device=device, dtype=torch.float32)).to(torch.bfloat16).contiguous(), 1)
        else:
            out[k] = (t.to(device=device, dtype=torch.float32).reshape(1, -1).contiguous(), 0)
    for (base, kind), parts in qkv_parts.items():
        t = torch.cat([parts["query"], parts["key"], parts["value"]], dim=0)
        name = base + ".qkv." + kind
        if kind == "weight":
            out[name] = (_pad_k(t.to(device=device, dtype=torch.float32)).to(torch.bfloat16).contiguous(), 1)
        else:
            out[name] = (t.to(device=device, dtype=torch.float32).reshape(1, -1).contiguous(), 0)
    return out, scalars


def check_guidance_keys(cfg, state_dict):
    """config and checkpoint must agree on guidance distillation: `guidance_embed: true` needs all four model.guidance_in.*
    tensors (the first missing one is named), and a checkpoint that holds them needs the flag -- the library decides by the
    tensors it is given (include/r3g.h r3g_flow_sample_sigmas), so a silent disagreement would change the sampler"""
    from .weights import GUIDANCE_KEYS
    have = [k for k in GUIDANCE_KEYS if k in state_dict]
    if cfg["dit"].get("guidance_embed", False):
        missing = [k for k in GUIDANCE_KEYS if k not in state_dict]
        if missing:
            raise KeyError("guidance-distilled model (guidance_embed: true): the checkpoint lacks '%s'" % missing[0])
    elif have:
        raise ValueError("the checkpoint holds '%s' but the config does not say guidance_embed: true" % have[0])


def check_geo_decoder_keys(cfg, state_dict):
    """config and checkpoint must agree on the geo decoder's width: `geo_decoder_downsample_ratio` other than
    1 needs vae.geo_decoder.latents_proj.{weight,bias} (the first missing one is named), and a checkpoint that holds either needs
    the ratio -- the library decides by the tensors it is given (include/r3g.h r3g_vae_decode: the rows of query_proj.weight), so a
    silent disagreement would change the decoder"""
    from .weights import LATENTS_PROJ_KEYS, geo_decoder_ratio
    have = [k for k in LATENTS_PROJ_KEYS if k in state_dict]
    if geo_decoder_ratio(cfg["vae"]) != 1:
        missing = [k for k in LATENTS_PROJ_KEYS if k not in state_dict]
        if missing:
            raise KeyError("narrow geo decoder (geo_decoder_downsample_ratio: %d): the checkpoint lacks '%s'"
                           % (geo_decoder_ratio(cfg["vae"]), missing[0]))
    elif have:
        raise ValueError("the checkpoint holds '%s' but the config does not say geo_decoder_downsample_ratio" % have[0])


class ShapeModel:
    """Weights + activation arena of one shape model on one GPU."""

    def __init__(self, cfg, state_dict, device=0, grid_chunk=0, private_ctx=False):
        if not torch.cuda.is_available():
            raise RuntimeError("r3g.ShapeModel needs an MI355X: libr3g has no CPU path")
        check_guidance_keys(cfg, state_dict)
        check_geo_decoder_keys(cfg, state_dict)
        self.guidance_embed = bool(cfg["dit"].get("guidance_embed", False))
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self.private_ctx = bool(private_ctx)
        self.ctx = _l.new_context(device) if private_ctx else _l.context(device)
        self.L = _l.lib()
        self._c = make_config(cfg, grid_chunk)
        with torch.cuda.device(self.device):
            self._w, self._scalars = prepare_weights(state_dict, self.device)
            self._install()
        p = cfg["cond"]["image_size"] // cfg["cond"]["patch_size"]
        self.cond_tokens = p * p + 1
        self.num_latents = cfg["vae"]["num_latents"]
        self.in_channels = cfg["dit"]["in_channels"]

    # The C context holds ONE model (arena + weight table) per device.  Several ShapeModel objects may coexist in a
    # process (e.g. mini + full, or test fixtures): the one being called re-installs itself if it is not current.
    _current = {}

    def _install(self):
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            _l.check(self.L.r3g_model_create(self.ctx, ctypes.byref(self._c)))
            for name, (t, code) in self._w.items():
                _l.check(self.L.r3g_model_set_tensor(self.ctx, name.encode(), t.data_ptr(), code, t.shape[0], t.shape[1]))
            for name, v in self._scalars.items():
                _l.check(self.L.r3g_model_set_scalar(self.ctx, name.encode(), v))
            torch.cuda.synchronize()
        if not self.private_ctx:
            ShapeModel._current[self.device.index] = self
        self._have_z = False

    def replace_vae(self, vcfg, vae_state_dict):
        """swap the WHOLE VAE (post_kl, transformer, geo decoder, scale_factor) for another one: `vcfg` its config (the `vae` part
        of a pipeline config), `vae_state_dict` its tensors under 'vae.'-prefixed names.  num_latents and embed_dim must equal the
        DiT's.  Only the VAE's tensors are uploaded; the DiT's and the conditioner's stay where they are and are registered again
        with the new model, whose arena and query-side cache are built afresh."""
        from .weights import geo_decoder_ratio
        old = self.cfg["vae"]
        for k in ("num_latents", "embed_dim"):
            if int(vcfg[k]) != int(old[k]):
                raise ValueError("replace_vae: the new VAE has %s=%s, the DiT was trained on %s" % (k, vcfg[k], old[k]))
        geo_decoder_ratio(vcfg)
        extra = [k for k in vae_state_dict if not k.startswith("vae.")]
        if extra:
            raise ValueError("replace_vae: '%s' is not a VAE tensor" % extra[0])
        cfg = dict(self.cfg)
        cfg["vae"] = dict(vcfg)
        check_geo_decoder_keys(cfg, vae_state_dict)
        c = make_config(cfg, self._c.grid_chunk)
        with torch.cuda.device(self.device):
            w, scalars = prepare_weights(vae_state_dict, self.device)
            if not self.private_ctx and ShapeModel._current.get(self.device.index) is self:
                self.trim()                       # the old cache goes before the new arena comes
            torch.cuda.synchronize()
            self._w = {k: v for k, v in self._w.items() if not k.startswith("vae.")}
            self._scalars = {k: v for k, v in self._scalars.items() if not k.startswith("vae.")}
            self._w.update(w)
            self._scalars.update(scalars)
            self.cfg, self._c = cfg, c
            self._install()

    def trim(self):
        """give the query-side cache of the geo decoder back to the device (r3g_model_trim); it is rebuilt on the next grid query"""
        if self.private_ctx or ShapeModel._current.get(self.device.index) is self:
            with torch.cuda.device(self.device):
                _l.check(self.L.r3g_model_trim(self.ctx))

    def _activate(self):
        if not self.private_ctx and ShapeModel._current.get(self.device.index) is not self:
            self._install()

    def _s(self):
        self._activate()
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def cond_encode(self, image):
        """image f32 [3,S,S] (resized / cropped / ImageNet-normalised) -> bf16 [tokens, hidden]"""
        image = image.to(self.device, torch.float32).contiguous()
        out = torch.empty((self.cond_tokens, self.cfg["cond"]["hidden_size"]), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_cond_encode(self.ctx, image.data_ptr(), out.data_ptr(), self._s()))
        return out

    def dit_forward(self, x, t, cond, n_double=-1, n_single=-1):
        """x f32 [B,N,C], t f32 [B], cond bf16 [B,Lc,D] -> f32 [B,N,C]"""
        x = x.to(self.device, torch.float32).contiguous()
        t = t.to(self.device, torch.float32).contiguous()
        cond = cond.to(self.device, torch.bfloat16).contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_dit_forward(self.ctx, x.data_ptr(), t.data_ptr(), cond.data_ptr(), out.data_ptr(),
                                            x.shape[0], n_double, n_single, self._s()))
        return out

    def dit_stream(self, batch):
        """joint residual stream left by the last dit_forward(): f32 [B, cond_tokens + num_latents, hidden], cond first"""
        out = torch.empty((batch, self.cond_tokens + self.num_latents, self.cfg["dit"]["hidden_size"]),
                          dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_dit_stream(self.ctx, out.data_ptr(), int(batch), self._s()))
        return out

    def flow_sample(self, latents, cond2, steps, guidance_scale, shift=1.0, uncond_uniform=None):
        """latents f32 [N,C] (modified in place and returned), cond2 bf16 [2,Lc,D] = [cond, uncond].
        uncond_uniform: all unconditional tokens identical (None = check on the device)."""
        latents = latents.to(self.device, torch.float32).contiguous()
        cond2 = cond2.to(self.device, torch.bfloat16).contiguous()
        if uncond_uniform is None:
            uncond_uniform = bool((cond2[1] == cond2[1, :1]).all().item())
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_flow_sample(self.ctx, latents.data_ptr(), cond2.data_ptr(), int(steps),
                                            float(guidance_scale), float(shift), int(bool(uncond_uniform)), self._s()))
        return latents

    def flow_sample_batch(self, latents, cond2, steps, guidance_scale, shift=1.0, uncond_uniform=None):
        """n independent objects through the denoising loop together: latents f32 [n,N,C] (modified in place and
        returned), cond2 bf16 [n,2,Lc,D].  Per-object results equal flow_sample() of that object bit for bit."""
        latents = latents.to(self.device, torch.float32).contiguous()
        cond2 = cond2.to(self.device, torch.bfloat16).contiguous()
        if latents.ndim != 3 or cond2.ndim != 4 or cond2.shape[0] != latents.shape[0] or cond2.shape[1] != 2:
            raise ValueError("flow_sample_batch: latents [n,N,C] and cond2 [n,2,Lc,D] expected")
        if uncond_uniform is None:
            uncond_uniform = bool((cond2[:, 1] == cond2[:, 1, :1]).all().item())
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_flow_sample_batch(self.ctx, latents.data_ptr(), cond2.data_ptr(), int(latents.shape[0]),
                                                  int(steps), float(guidance_scale), float(shift),
                                                  int(bool(uncond_uniform)), self._s()))
        return latents

    def flow_sample_sigmas(self, latents, cond2, sigmas, guidance_scale, uncond_uniform=None):
        """the denoising loop over an explicit sigma table (r3g_flow_sample_sigmas): latents f32 [n,N,C] (modified in place and
        returned), cond2 bf16 [n,2,Lc,D], sigmas float32 [steps + 1] on the host.  A guidance-distilled model (guidance_embed)
        runs without the CFG batch -- guidance_scale feeds guidance_in, the unconditional half of cond2 is never read, up to 8
        objects share a launch --; any other model runs classifier-free guidance as flow_sample_batch does."""
        import numpy as np
        latents = latents.to(self.device, torch.float32).contiguous()
        cond2 = cond2.to(self.device, torch.bfloat16).contiguous()
        if latents.ndim != 3 or cond2.ndim != 4 or cond2.shape[0] != latents.shape[0] or cond2.shape[1] != 2:
            raise ValueError("flow_sample_sigmas: latents [n,N,C] and cond2 [n,2,Lc,D] expected")
        sig = np.ascontiguousarray(np.asarray(sigmas, dtype=np.float32).reshape(-1))
        if sig.size < 2 or not np.isfinite(sig).all():
            raise ValueError("flow_sample_sigmas: at least two finite sigmas expected")
        if uncond_uniform is None:
            uncond_uniform = self.guidance_embed or bool((cond2[:, 1] == cond2[:, 1, :1]).all().item())
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_flow_sample_sigmas(self.ctx, latents.data_ptr(), cond2.data_ptr(), int(latents.shape[0]),
                                                   sig.ctypes.data_as(ctypes.c_void_p), int(sig.size), float(guidance_scale),
                                                   int(bool(uncond_uniform)), self._s()))
        return latents

    def vae_decode(self, latents, return_z=False):
        latents = latents.to(self.device, torch.float32).contiguous()
        z = torch.empty((self.num_latents, self.cfg["vae"]["width"]), dtype=torch.float32, device=self.device) \
            if return_z else None
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_vae_decode(self.ctx, latents.data_ptr(), z.data_ptr() if return_z else None, self._s()))
        self._have_z = True
        return z

    def grid_query(self, bound, octree_resolution, out=None, start=0, count=None):
        n = octree_resolution + 1
        if out is None:
            out = torch.empty((n, n, n), dtype=torch.float32, device=self.device)
        if count is None:
            count = n ** 3 - start
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_grid_query(self.ctx, float(bound), int(octree_resolution), out.data_ptr(), int(start),
                                           int(count), self._s()))
        return out

    def grid_query_points(self, bound, octree_resolution, idx, out=None):
        """the geo decoder at listed points of the (R+1)^3 lattice (int32 linear indices, any order) -> f32 [len(idx)];
        a point's logit equals grid_query's for the same index bit for bit"""
        idx = idx.to(self.device, torch.int32).contiguous()
        if out is None:
            out = torch.empty((idx.numel(),), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_grid_query_points(self.ctx, float(bound), int(octree_resolution), idx.data_ptr() if idx.numel() else None,
                                                  int(idx.numel()), out.data_ptr() if idx.numel() else None, self._s()))
        return out

    def set_kv_selection(self, topk=0, group=None, stride=None):
        """adaptive top-k selection of the geo decoder's cross-attention keys (options "geo_kv_topk" /
        "geo_kv_group" / "geo_kv_stride" of the library, which are process-wide): topk 0 = exact attention (the default), k > 0 =
        keep k keys per group of `group` consecutive points and head (clamped to num_latents), -1 = upstream's rule (1024 of 3072,
        256 of 512, otherwise a third).  group / stride None: left as they are (8192 / 64 unless set before).  A value outside its
        range raises R3GError and changes nothing.  Returns the number of keys a grid query of this model will keep (0: exact)."""
        if group is not None:
            _l.check(self.L.r3g_set_option(b"geo_kv_group", int(group)))
        if stride is not None:
            _l.check(self.L.r3g_set_option(b"geo_kv_stride", int(stride)))
        _l.check(self.L.r3g_set_option(b"geo_kv_topk", int(topk)))
        return kv_topk(int(topk), self.num_latents)

    def kv_selection_last(self):
        """the index table of the last pass evaluated in top-k mode: int32 [groups, heads, k] on the device (ascending key indices
        per group and head; a pass's tail group last).  R3GError (R3G_ERR_STATE) when no pass has run in top-k mode."""
        self._activate()
        g, h, k = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_kv_selection_last(self.ctx, None, 0, ctypes.byref(g), ctypes.byref(h), ctypes.byref(k), self._s()))
            out = torch.empty((g.value, h.value, k.value), dtype=torch.int32, device=self.device)
            _l.check(self.L.r3g_kv_selection_last(self.ctx, out.data_ptr(), out.numel(), None, None, None, self._s()))
        return out

    def kv_selection_operands(self):
        """what kv_selection_last()'s table was selected from (r3g_kv_selection_operands): the pass's Q rows bf16 [heads, lq, 64]
        as the attention kernel reads them and the object's K bf16 [heads, num_latents, 64].  Valid until the next grid query."""
        self._activate()
        n = [ctypes.c_int(0) for _ in range(4)]
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_kv_selection_operands(self.ctx, None, 0, None, 0, *[ctypes.byref(v) for v in n], self._s()))
            lq, lq_pad, lk, lk_pad = (v.value for v in n)
            from .weights import geo_decoder_ratio
            heads = self.cfg["vae"]["heads"] // geo_decoder_ratio(self.cfg["vae"])
            q = torch.empty((heads, lq_pad, 64), dtype=torch.bfloat16, device=self.device)
            k = torch.empty((heads, lk_pad, 64), dtype=torch.bfloat16, device=self.device)
            _l.check(self.L.r3g_kv_selection_operands(self.ctx, q.data_ptr(), q.numel(), k.data_ptr(), k.numel(), None, None, None,
                                                      None, self._s()))
        return q[:, :lq], k[:, :lk]

    def grid_query_hier(self, bound, octree_resolution, mc_level=0.0, band=0.95, min_resolution=63, out=None, stats=True):
        """hierarchical volume decoding (r3g_grid_query_hier): a full (R+1)^3 grid whose points near the surface hold the dense
        decoder's values, and {"levels", "evaluated_per_level", "evaluated", "dense_points", "unsafe_cells"} (None without stats)"""
        n = octree_resolution + 1
        if out is None:
            out = torch.empty((n, n, n), dtype=torch.float32, device=self.device)
        st = (ctypes.c_int64 * 36)()
        with torch.cuda.device(self.device):
            _l.check(self.L.r3g_grid_query_hier(self.ctx, float(bound), int(octree_resolution), float(mc_level), float(band),
                                                int(min_resolution), out.data_ptr(), st if stats else None, 36 if stats else 0,
                                                self._s()))
        if not stats:
            return out, None
        nl = int(st[0])
        return out, {"levels": [int(st[4 + 2 * i]) for i in range(nl)],
                     "evaluated_per_level": [int(st[5 + 2 * i]) for i in range(nl)],
                     "evaluated": int(st[1]), "dense_points": int(st[2]), "unsafe_cells": int(st[3])}
