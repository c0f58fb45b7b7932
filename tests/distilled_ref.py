"""Test-side restatement of upstream's guidance-distilled shape model (the -fast / -turbo checkpoints) and of its two sigma
tables, written from the specification in DESIGN.md section 4b ([UPSTREAM-RECALLED]; parity unpinned) -- independently of the
product's r3g/flow.py and csrc/model.cpp.  oracle/hy3d_torch.py asserts `not guidance_embed`, so the restatement subclasses its
Hunyuan3DDiT (constructed with guidance_embed=False) and adds what a distilled checkpoint adds:

    guidance_in = MLPEmbedder(256 -> H -> H)
    vec = time_in(timestep_embedding(t, 256)) + guidance_in(timestep_embedding(g, 256))      g: the guidance scale itself

and the sampler without the CFG batch: x <- x + (sigma_next - sigma) v, conditional context only.

The `mutate` switches are the wiring hazards tests/test_distilled_cpu.py proves the tolerance against.
"""
import numpy as np
import torch

from oracle import hy3d_torch as H

GUIDANCE_KEYS = ("model.guidance_in.in_layer.weight", "model.guidance_in.in_layer.bias",
                 "model.guidance_in.out_layer.weight", "model.guidance_in.out_layer.bias")
MUTATIONS = ("guidance_in_dropped", "g_minus_one", "no_time_factor_on_g", "linspace_table")


def linspace_sigmas(n, shift=1.0):
    s = np.linspace(0, 1, n)
    s = shift * s / (1 + (shift - 1) * s)
    return np.concatenate([s, [1.0]]).astype(np.float32)


def consistency_sigmas(n, num_train_timesteps=1000, pcm_timesteps=100):
    full = np.linspace(0, 1, num_train_timesteps)
    euler = np.concatenate([[0], (np.arange(1, pcm_timesteps) * (num_train_timesteps // pcm_timesteps)).round() - 1]).astype(int)
    idx = np.floor(np.linspace(0, pcm_timesteps, n, endpoint=False)).astype(int)
    return np.concatenate([full[euler[idx]], [1.0]]).astype(np.float32)


class DistilledDiT(H.Hunyuan3DDiT):
    def __init__(self, **dit_cfg):
        kw = dict(dit_cfg)
        kw["guidance_embed"] = False
        super().__init__(**kw)
        self.guidance_in = H.MLPEmbedder(256, kw["hidden_size"])
        self.mutate = None

    def vec(self, t, guidance, dtype):
        v = self.time_in(H.timestep_embedding(t, 256, time_factor=self.time_factor).to(dtype))
        if self.mutate == "guidance_in_dropped":
            return v
        g = guidance - 1.0 if self.mutate == "g_minus_one" else guidance
        tf = 1.0 if self.mutate == "no_time_factor_on_g" else self.time_factor
        return v + self.guidance_in(H.timestep_embedding(g, 256, time_factor=tf).to(dtype))

    def forward(self, x, t, cond, guidance):
        latent = self.latent_in(x)
        vec = self.vec(t, guidance, latent.dtype)
        cond = self.cond_in(cond)
        for blk in self.double_blocks:
            latent, cond = blk(latent, cond, vec)
        latent = H._joint(cond, latent)
        for blk in self.single_blocks:
            latent = blk(latent, vec)
        latent = H._unjoint(latent, cond.shape[1])[1]
        return self.final_layer(latent, vec)


def distilled_cfg(cfg):
    import copy
    c = copy.deepcopy(cfg)
    c["dit"]["guidance_embed"] = True
    return c


def synthetic_state_dict(cfg, seed):
    """the oracle's unit-scale checkpoint of `cfg` (undistilled keys, same seed -> same tensors) + guidance_in.* drawn the same
    way from a generator of its own: Linear ~ N(0, 1/fan_in), bias ~ N(0, 0.1^2)"""
    base = copy_cfg_undistilled(cfg)
    sd = H.synthetic_state_dict(base, seed=seed)
    g = torch.Generator().manual_seed(10_000 + seed)
    Hd = cfg["dit"]["hidden_size"]
    for name, shape in zip(GUIDANCE_KEYS, ((Hd, 256), (Hd,), (Hd, Hd), (Hd,))):
        sd[name] = (torch.randn(shape, generator=g) / shape[1] ** 0.5) if len(shape) == 2 else 0.1 * torch.randn(shape, generator=g)
    return sd


def copy_cfg_undistilled(cfg):
    import copy
    c = copy.deepcopy(cfg)
    c["dit"]["guidance_embed"] = False
    return c


def load_dit(cfg, sd):
    m = DistilledDiT(**cfg["dit"])
    m.load_state_dict({k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}, strict=True)
    return m.eval()


@torch.no_grad()
def sample(model, cond, latents, sigmas, guidance_scale):
    """cond f32 [1, Lc, D] (the conditional context), latents f32 [1, N, C], sigmas [steps + 1] -> latents after all steps"""
    g = torch.full((latents.shape[0],), float(guidance_scale), dtype=latents.dtype)
    for i in range(len(sigmas) - 1):
        ds = float(sigmas[i + 1] - sigmas[i])
        if ds == 0.0:
            continue                                              # x += 0 * v
        t = torch.full((latents.shape[0],), float(sigmas[i]), dtype=latents.dtype)
        latents = latents + ds * model(latents, t, cond, g)
    return latents


def table(n, consistency, mutate=None):
    if mutate == "linspace_table":
        consistency = False
    return consistency_sigmas(n) if consistency else linspace_sigmas(n)
