"""TEST INFRASTRUCTURE: the turbo shape VAE restated in PyTorch (CPU, fp32) from the text of DESIGN.md section 4e -- a ShapeVAE whose
geo decoder runs at width // r and heads // r behind a `latents_proj` -- as subclasses of the oracle's ShapeVAE /
CrossAttentionDecoder (oracle/hy3d_torch.py has no downsample ratio).  [UPSTREAM-RECALLED], parity-unpinned: no upstream source is
available; what the GPU tests establish is that the HIP path computes THIS function.

The three `mut_*` switches are the wiring hazards of the new pieces (tests/test_turbo_vae_cpu.py shows each of them moves the logits
by >= MARGIN x the tolerance the GPU tests apply)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import hy3d_torch as H

RATIO_KEY = "geo_decoder_downsample_ratio"


class TurboCrossAttentionDecoder(H.CrossAttentionDecoder):
    def __init__(self, fourier_embedder, width, heads, mlp_expand_ratio, enable_ln_post, qkv_bias, qk_norm, downsample_ratio=1):
        r = int(downsample_ratio)
        assert width % r == 0 and heads % r == 0
        super().__init__(fourier_embedder, width // r, heads // r, mlp_expand_ratio, enable_ln_post, qkv_bias, qk_norm)
        self.downsample_ratio = r
        self.full_heads = heads
        if r != 1:
            self.latents_proj = nn.Linear(width, width // r)          # with bias; registered after every other parameter
        self.mut_skip_bias = self.mut_proj_after_ln2 = self.mut_full_heads = False

    def forward(self, queries, latents):
        blk = self.cross_attn_decoder
        attention = blk.attn.attention
        heads_g = attention.heads
        ln_2 = blk.ln_2
        try:
            if self.mut_full_heads:
                attention.heads = self.full_heads
            if self.downsample_ratio != 1:
                if self.mut_proj_after_ln2:
                    # hazard: the normalisation in front of the projection (at the VAE's width, where ln_2 has no parameters), its
                    # affine behind it
                    latents = F.layer_norm(latents, latents.shape[-1:], eps=1e-6)
                    latents = self.latents_proj(latents) * ln_2.weight + ln_2.bias
                    blk.ln_2 = nn.Identity()
                elif self.mut_skip_bias:
                    latents = F.linear(latents, self.latents_proj.weight)
                else:
                    latents = self.latents_proj(latents)              # BEFORE ln_2 (which is inside the block)
            return super().forward(queries, latents)
        finally:
            attention.heads = heads_g
            blk.ln_2 = ln_2


class TurboShapeVAE(H.ShapeVAE):
    def __init__(self, num_latents, embed_dim, width, heads, num_decoder_layers, num_freqs, include_pi, qkv_bias, qk_norm,
                 scale_factor, geo_decoder_mlp_expand_ratio=4, geo_decoder_ln_post=True, geo_decoder_downsample_ratio=1):
        super().__init__(num_latents, embed_dim, width, heads, num_decoder_layers, num_freqs, include_pi, qkv_bias, qk_norm,
                         scale_factor, geo_decoder_mlp_expand_ratio, geo_decoder_ln_post)
        self.geo_decoder = TurboCrossAttentionDecoder(self.fourier_embedder, width, heads, geo_decoder_mlp_expand_ratio,
                                                      geo_decoder_ln_post, qkv_bias, qk_norm, geo_decoder_downsample_ratio)


class TurboShapePipeline(H.ShapePipeline):
    """oracle.ShapePipeline whose VAE honours geo_decoder_downsample_ratio"""

    def __init__(self, cfg):
        base = dict(cfg)
        base["vae"] = {k: v for k, v in cfg["vae"].items() if k != RATIO_KEY}
        super().__init__(base)
        self.cfg = cfg
        self.vae = TurboShapeVAE(**cfg["vae"])
        self.eval()


def turbo_vae_cfg(vcfg, ratio=4, expand=1, ln_post=False):
    v = dict(vcfg)
    v.update({RATIO_KEY: ratio, "geo_decoder_mlp_expand_ratio": expand, "geo_decoder_ln_post": ln_post})
    return v


def synthetic_vae_state_dict(vcfg, seed=0):
    """unit-scale seeded weights of a TurboShapeVAE, 'vae.'-prefixed (the oracle's rule: Linear ~ N(0, 1 / fan_in), biases
    N(0, 0.1^2) -- latents_proj's N(0, 0.5^2), see below --, norm scales 1 +- 10 %)"""
    vae = TurboShapeVAE(**vcfg)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, p in vae.state_dict().items():
        if H._is_norm_scale(k):
            t = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
        elif p.ndim >= 2:
            t = torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5
        elif k.endswith("latents_proj.bias"):
            # latents_proj's output has unit spread per channel and goes straight into ln_2, which removes most of a small common
            # offset: at the oracle's 0.1 a missing bias would hide inside the bf16 tolerance.  At 0.5 it is a first-order term.
            t = 0.5 * torch.randn(p.shape, generator=g)
        else:
            t = 0.1 * torch.randn(p.shape, generator=g)
        sd["vae." + k] = t.float()
    return sd


def synthetic_state_dict(cfg, seed=0):
    """a whole checkpoint for `cfg`: the oracle's synthetic DiT / conditioner of the same seed, and this file's VAE"""
    base = dict(cfg)
    base["vae"] = {k: v for k, v in cfg["vae"].items() if k != RATIO_KEY}
    sd = {k: v for k, v in H.synthetic_state_dict(base, seed=seed).items() if not k.startswith("vae.")}
    sd.update(synthetic_vae_state_dict(cfg["vae"], seed + 1000))
    return sd


def load_vae(vcfg, sd):
    vae = TurboShapeVAE(**vcfg)
    vae.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("vae.")}, strict=True)
    return vae.eval()


def load_pipeline(cfg, sd):
    pipe = TurboShapePipeline(cfg)
    for prefix, mod in (("model.", pipe.model), ("vae.", pipe.vae), ("conditioner.", pipe.conditioner)):
        mod.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)
    return pipe


@torch.no_grad()
def decode(vae, latents):
    """latents [N, C] -> z [1, N, width]"""
    return vae(latents[None] / vae.scale_factor)


@torch.no_grad()
def logits(vae, z, bound, R, start, count):
    pts = torch.from_numpy(H.dense_grid_points(bound, R)[start:start + count])
    return vae.geo_decoder(queries=pts[None], latents=z)[0, :, 0]
