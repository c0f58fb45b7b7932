"""Checkpoint layout of the Hunyuan3D-2 shape model (upstream state-dict names and shapes) and
checkpoint sources: safetensors on disk, or seeded synthetic weights generated directly on the GPU
(no network and no real weights are available where this was built; SURVEY.md 8d "synthetic weights").
"""
import os

import torch


def swiglu_hidden(hidden_size, mlp_ratio):
    return (int(int(hidden_size * mlp_ratio) * 2 / 3) + 7) // 8 * 8


def param_shapes(cfg):
    """name -> shape for every floating-point parameter the pipeline loads."""
    d, v, c = cfg["dit"], cfg["vae"], cfg["cond"]
    s = {}

    def lin(name, n, k, bias=True):
        s[name + ".weight"] = (n, k)
        if bias:
            s[name + ".bias"] = (n,)

    H, mh, hd = d["hidden_size"], int(d["hidden_size"] * d["mlp_ratio"]), d["hidden_size"] // d["num_heads"]
    lin("model.latent_in", H, d["in_channels"])
    lin("model.time_in.in_layer", H, 256)
    lin("model.time_in.out_layer", H, H)
    lin("model.cond_in", H, d["context_in_dim"])
    for i in range(d["depth"]):
        for st in ("img", "txt"):
            b = "model.double_blocks.%d.%s" % (i, st)
            lin(b + "_mod.lin", 6 * H, H)
            lin(b + "_attn.qkv", 3 * H, H, d["qkv_bias"])
            s[b + "_attn.norm.query_norm.scale"] = (hd,)
            s[b + "_attn.norm.key_norm.scale"] = (hd,)
            lin(b + "_attn.proj", H, H)
            lin(b + "_mlp.0", mh, H)
            lin(b + "_mlp.2", H, mh)
    for i in range(d["depth_single_blocks"]):
        b = "model.single_blocks.%d" % i
        lin(b + ".linear1", 3 * H + mh, H)
        lin(b + ".linear2", H, H + mh)
        s[b + ".norm.query_norm.scale"] = (hd,)
        s[b + ".norm.key_norm.scale"] = (hd,)
        lin(b + ".modulation.lin", 3 * H, H)
    lin("model.final_layer.linear", d["in_channels"], H)
    lin("model.final_layer.adaLN_modulation.1", 2 * H, H)

    _vae_shapes(v, lin, s)

    def ln(name, n):
        s[name + ".weight"] = (n,)
        s[name + ".bias"] = (n,)

    Hc, P = c["hidden_size"], c["image_size"] // c["patch_size"]
    F = swiglu_hidden(Hc, c["mlp_ratio"])
    m = "conditioner.main_image_encoder.model"
    s[m + ".embeddings.cls_token"] = (1, 1, Hc)
    s[m + ".embeddings.mask_token"] = (1, Hc)
    s[m + ".embeddings.position_embeddings"] = (1, P * P + 1, Hc)
    s[m + ".embeddings.patch_embeddings.projection.weight"] = (Hc, 3, c["patch_size"], c["patch_size"])
    s[m + ".embeddings.patch_embeddings.projection.bias"] = (Hc,)
    for i in range(c["num_hidden_layers"]):
        b = "%s.encoder.layer.%d" % (m, i)
        ln(b + ".norm1", Hc)
        for n in ("query", "key", "value"):
            lin(b + ".attention.attention." + n, Hc, Hc)
        lin(b + ".attention.output.dense", Hc, Hc)
        s[b + ".layer_scale1.lambda1"] = (Hc,)
        ln(b + ".norm2", Hc)
        lin(b + ".mlp.weights_in", 2 * F, Hc)
        lin(b + ".mlp.weights_out", Hc, F)
        s[b + ".layer_scale2.lambda1"] = (Hc,)
    ln(m + ".layernorm", Hc)
    if d.get("guidance_embed", False):
        # guidance-distilled checkpoints (upstream's -fast / -turbo subfolders): guidance_in = MLPEmbedder(256 -> H -> H).  AFTER
        # every other key: synthetic_state_dict draws from one generator in this order, so all other tensors of a distilled
        # synthetic checkpoint equal the undistilled one of the same seed
        lin("model.guidance_in.in_layer", H, 256)
        lin("model.guidance_in.out_layer", H, H)
    if geo_decoder_ratio(v) != 1:
        # the turbo VAE's narrow geo decoder: latents_proj = Linear(width -> width_g), AFTER every other key for
        # the same reason -- and only then, so that every checkpoint of ratio 1 keeps its keys, their order and its tensors
        lin(LATENTS_PROJ, geo_decoder_width(v), v["width"])
    return s


LATENTS_PROJ = "vae.geo_decoder.latents_proj"
LATENTS_PROJ_KEYS = (LATENTS_PROJ + ".weight", LATENTS_PROJ + ".bias")


def geo_decoder_ratio(v):
    """`geo_decoder_downsample_ratio` of a VAE config (upstream's turbo VAEs: 4; absent = 1)"""
    r = int(v.get("geo_decoder_downsample_ratio", 1))
    if r < 1 or v["width"] % r or v["heads"] % r or (v["width"] // r) // (v["heads"] // r) != v["width"] // v["heads"]:
        raise ValueError("geo_decoder_downsample_ratio=%r does not divide width %d / heads %d" % (r, v["width"], v["heads"]))
    return r


def geo_decoder_width(v):
    """width_g = width // ratio (heads_g = heads // ratio: the head dimension stays)"""
    return v["width"] // geo_decoder_ratio(v)


def _vae_shapes(v, lin, s):
    """the ShapeVAE's decoder-side parameters ('vae.' prefix) in checkpoint order, without latents_proj (param_shapes and
    vae_param_shapes append it last).  The geo decoder is built at width_g = width // geo_decoder_downsample_ratio."""
    W, whd = v["width"], v["width"] // v["heads"]
    Wg = geo_decoder_width(v)
    lin("vae.post_kl", W, v["embed_dim"])

    def qknorm(base):
        if v["qk_norm"]:
            for n in ("q_norm", "k_norm"):
                s["%s.%s.weight" % (base, n)] = (whd,)
                s["%s.%s.bias" % (base, n)] = (whd,)

    def ln(name, n):
        s[name + ".weight"] = (n,)
        s[name + ".bias"] = (n,)

    for i in range(v["num_decoder_layers"]):
        b = "vae.transformer.resblocks.%d" % i
        lin(b + ".attn.c_qkv", 3 * W, W, v["qkv_bias"])
        lin(b + ".attn.c_proj", W, W)
        qknorm(b + ".attn.attention")
        ln(b + ".ln_1", W)
        lin(b + ".mlp.c_fc", 4 * W, W)
        lin(b + ".mlp.c_proj", W, 4 * W)
        ln(b + ".ln_2", W)
    g = "vae.geo_decoder"
    e = v.get("geo_decoder_mlp_expand_ratio", 4)
    lin(g + ".query_proj", Wg, 3 * (2 * v["num_freqs"] + 1))
    lin(g + ".cross_attn_decoder.attn.c_q", Wg, Wg, v["qkv_bias"])
    lin(g + ".cross_attn_decoder.attn.c_kv", 2 * Wg, Wg, v["qkv_bias"])
    lin(g + ".cross_attn_decoder.attn.c_proj", Wg, Wg)
    if v.get("geo_decoder_ln_post", True):
        qknorm(g + ".cross_attn_decoder.attn.attention")
    for n in ("ln_1", "ln_2", "ln_3"):
        ln(g + ".cross_attn_decoder." + n, Wg)
    lin(g + ".cross_attn_decoder.mlp.c_fc", e * Wg, Wg)
    lin(g + ".cross_attn_decoder.mlp.c_proj", Wg, e * Wg)
    if v.get("geo_decoder_ln_post", True):
        ln(g + ".ln_post", Wg)
    lin(g + ".output_proj", 1, Wg)


def vae_param_shapes(vcfg):
    """name ('vae.' prefix) -> shape of a VAE-only checkpoint (upstream's hunyuan3d-vae-v2-0-turbo / -mini-turbo subfolders): the
    decoder side of the ShapeVAE, latents_proj last when the geo decoder is narrow"""
    s = {}

    def lin(name, n, k, bias=True):
        s[name + ".weight"] = (n, k)
        if bias:
            s[name + ".bias"] = (n,)

    _vae_shapes(vcfg, lin, s)
    if geo_decoder_ratio(vcfg) != 1:
        lin(LATENTS_PROJ, geo_decoder_width(vcfg), vcfg["width"])
    return s


def turbo_vae_config(vcfg):
    """the VAE config of 'synthetic:turbo-vae': `vcfg`'s own dims with upstream's turbo values [UPSTREAM-RECALLED] -- downsample
    ratio 4, MLP expand ratio 1, no ln_post (hence no q/k norm in the decoder)"""
    v = dict(vcfg)
    v.update(geo_decoder_downsample_ratio=4, geo_decoder_mlp_expand_ratio=1, geo_decoder_ln_post=False)
    geo_decoder_ratio(v)
    return v


GUIDANCE_KEYS = tuple("model.guidance_in.%s.%s" % (l, k) for l in ("in_layer", "out_layer") for k in ("weight", "bias"))


def _is_scale(name):
    return (name.endswith(".scale") or name.endswith("lambda1") or
            (name.endswith(".weight") and any(t in name for t in (
                "norm1.", "norm2.", "q_norm.", "k_norm.", "ln_1.", "ln_2.", "ln_3.", "ln_post.", "layernorm."))))


def synthetic_vae_state_dict(vcfg, seed=0, device="cuda"):
    """seeded synthetic VAE-only checkpoint ('vae.'-prefixed names) at unit scale, drawn from its OWN generator in
    vae_param_shapes order: it does not depend on what model it is swapped into"""
    g = torch.Generator(device=device).manual_seed(seed)
    return {name: _draw(name, shape, g, device, None) for name, shape in vae_param_shapes(vcfg).items()}


def synthetic_state_dict(cfg, seed=0, device="cuda", std=None):
    """Seeded synthetic checkpoint generated on `device` (timing / plumbing).  Default: every layer at
    unit scale -- Linear ~ N(0, 1/fan_in), adaLN modulation layers ~ N(0, 9/fan_in) with bias N(0, 0.3^2), norm scales
    1 +- 10 %, biases N(0, 0.1^2), Dinov2 cls / position embeddings N(0, 0.5^2) -- so that every branch contributes O(1)
    to its residual stream and the occupancy field changes sign (a surface exists at every model size).
    std = 0.02 (a float) reproduces the first-round checkpoint: Linear ~ N(0, std^2), near-identity blocks."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in param_shapes(cfg).items():
        sd[name] = _draw(name, shape, g, device, std)
    return sd


def _draw(name, shape, g, device, std):
    is_mod = ".lin." in name or "adaLN" in name
    emb = name.endswith(("cls_token", "mask_token", "position_embeddings"))
    if _is_scale(name):
        return 1.0 + (0.1 if std is None else 0.05) * torch.randn(shape, generator=g, device=device)
    if emb:
        return (0.5 if std is None else std) * torch.randn(shape, generator=g, device=device)
    if len(shape) >= 2:
        if std is None:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            scale = (3.0 if is_mod else 1.0) / fan_in ** 0.5
        else:
            scale = 0.2 if "output_proj" in name else std
        return scale * torch.randn(shape, generator=g, device=device)
    return ((0.3 if is_mod else 0.1) if std is None else 0.01) * torch.randn(shape, generator=g, device=device)


def load_safetensors_dir(path, variant=None, use_safetensors=True):
    """<path>/model[.variant].safetensors (upstream single-file layout with model./vae./conditioner. prefixes), or -- upstream's
    `use_safetensors=False` / older snapshots -- <path>/model[.variant].ckpt: a torch pickle of {"model": sd, "vae": sd,
    "conditioner": sd} (loaded with weights_only=True), flattened to the same prefixed names.  [UPSTREAM-RECALLED: the two file
    names and the three top-level keys are how hy3dgen/shapegen/pipelines.py `from_single_file` reads them.]"""
    stems = (["model.%s" % variant] if variant else []) + ["model", "model.fp16"]
    if use_safetensors:
        from safetensors.torch import load_file
        for n in stems:
            f = os.path.join(path, n + ".safetensors")
            if os.path.exists(f):
                return load_file(f)
    for n in stems:
        f = os.path.join(path, n + ".ckpt")
        if os.path.exists(f):
            return flatten_ckpt(torch.load(f, map_location="cpu", weights_only=True))
    raise FileNotFoundError("no model*.safetensors / model*.ckpt under " + path)


def flatten_ckpt(ckpt):
    """{"model": {...}, "vae": {...}, "conditioner": {...}} (optionally under "state_dict") -> {"model.x": t, ...}; a dict that
    is already flat passes through"""
    if isinstance(ckpt, dict) and isinstance(ckpt.get("state_dict"), dict):
        ckpt = ckpt["state_dict"]
    if not isinstance(ckpt, dict) or not ckpt:
        raise ValueError("checkpoint is not a state dict")
    if all(torch.is_tensor(v) for v in ckpt.values()):
        return dict(ckpt)
    flat = {}
    for part, sd in ckpt.items():
        if not isinstance(sd, dict):
            continue          # e.g. a stored step counter
        for k, v in sd.items():
            if torch.is_tensor(v):
                flat["%s.%s" % (part, k)] = v
    if not flat:
        raise ValueError("checkpoint holds no tensors under its top-level keys %s" % sorted(ckpt))
    return flat


def _model_file(path, variant, use_safetensors):
    stems = (["model.%s" % variant] if variant else []) + ["model", "model.fp16"]
    exts = ([".safetensors"] if use_safetensors else []) + [".ckpt"]
    for ext in exts:
        for n in stems:
            f = os.path.join(path, n + ext)
            if os.path.exists(f):
                return f
    raise FileNotFoundError("no model*.safetensors / model*.ckpt under " + path)


def vae_config_from_yaml(doc):
    """the `params` of a VAE-only snapshot's config.yaml, written either as {params: ...} (upstream's own layout, beside `target`)
    or as {vae: {params: ...}}"""
    if not isinstance(doc, dict):
        raise ValueError("VAE config.yaml is not a mapping")
    node = doc["vae"] if isinstance(doc.get("vae"), dict) else doc
    params = node.get("params")
    if not isinstance(params, dict):
        raise ValueError("VAE config.yaml has neither `params` nor `vae.params`")
    return dict(params)


def load_vae_dir(path, variant=None, use_safetensors=True):
    """a VAE-only snapshot folder (upstream's hunyuan3d-vae-v2-0-turbo layout): <path>/config.yaml + model[.variant].safetensors or
    .ckpt whose keys carry NO prefix (post_kl.weight, transformer.resblocks.0..., geo_decoder....) -> (params of config.yaml, state
    dict with the 'vae.' prefix added).  The encoder side (encoder.*, pre_kl.*) is not used here and is dropped."""
    import yaml
    with open(os.path.join(path, "config.yaml")) as f:
        params = vae_config_from_yaml(yaml.safe_load(f))
    f = _model_file(path, variant, use_safetensors)
    if f.endswith(".safetensors"):
        from safetensors.torch import load_file
        raw = load_file(f)
    else:
        raw = torch.load(f, map_location="cpu", weights_only=True)
        if isinstance(raw, dict) and isinstance(raw.get("state_dict"), dict):
            raw = raw["state_dict"]
        if isinstance(raw, dict) and isinstance(raw.get("vae"), dict):
            raw = raw["vae"]
    if not isinstance(raw, dict) or not raw:
        raise ValueError("VAE checkpoint %s is not a state dict" % f)
    sd = {}
    for k, t in raw.items():
        if not torch.is_tensor(t):
            continue
        if k.startswith("vae."):
            k = k[4:]
        if k.startswith(("encoder.", "pre_kl.")):
            continue
        sd["vae." + k] = t
    return params, sd
