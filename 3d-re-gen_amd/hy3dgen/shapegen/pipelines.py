"""Hunyuan3DDiTFlowMatchingPipeline on MI355X -- same constructor / call surface as upstream
hy3dgen/shapegen/pipelines.py as used by the reference (src/2d_to_3d_models/run.py:122-124, 77-84):

    pipe = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained(path, subfolder=..., variant=...)
    mesh = pipe(image=pil_rgba, num_inference_steps=50, octree_resolution=256, num_chunks=16000,
                generator=torch.manual_seed(seed), output_type="trimesh")[0]

All arithmetic runs in libr3g.so (HIP kernels); this file is host plumbing.  `num_chunks` is accepted and
ignored: the grid query is chunked internally and its result does not depend on the chunk size.
"""
import os

import numpy as np
import torch
import yaml

from r3g import flow as _flow
from r3g import dmc as _dmc
from r3g import mc as _mc
from r3g import model as _model
from r3g import weights as _weights
from r3g.mesh import Mesh

from .preprocessors import ImageProcessorV2, conditioner_transform

FULL = dict(
    dit=dict(in_channels=64, context_in_dim=1536, hidden_size=1024, mlp_ratio=4.0, num_heads=16, depth=16,
             depth_single_blocks=32, qkv_bias=True, time_factor=1000, guidance_embed=False),
    vae=dict(num_latents=3072, embed_dim=64, width=1024, heads=16, num_decoder_layers=16, num_freqs=8,
             include_pi=False, qkv_bias=False, qk_norm=True, scale_factor=0.9990943042622529,
             geo_decoder_mlp_expand_ratio=4, geo_decoder_ln_post=True),
    cond=dict(image_size=518, patch_size=14, hidden_size=1536, num_hidden_layers=40, num_attention_heads=24,
              mlp_ratio=4, use_swiglu_ffn=True, layer_norm_eps=1e-6),
    sched=dict(num_train_timesteps=1000, shift=1.0, kind="FlowMatchEulerDiscreteScheduler", pcm_timesteps=100),
    proc=dict(size=512, border_ratio=0.15),
    guidance_scale=5.0, box_v=1.01, mc_level=0.0)

BUILTIN = ("full", "mini", "full-fast", "full-turbo", "mini-turbo")


def builtin_config(name):
    """'full' = hunyuan3d-dit-v2-0, 'mini' = hunyuan3d-dit-v2-mini (dims recalled); the
    guidance-distilled subfolders 'full-fast' = hunyuan3d-dit-v2-0-fast, 'full-turbo' = hunyuan3d-dit-v2-0-turbo, 'mini-turbo' =
    hunyuan3d-dit-v2-mini-turbo: the same dims with guidance_embed, the turbo ones on the consistency scheduler."""
    import copy
    if name not in BUILTIN:
        raise KeyError(name)
    c = copy.deepcopy(FULL)
    base, _, variant = name.partition("-")
    if base == "mini":
        c["dit"].update(depth=8, depth_single_blocks=16)
        c["vae"].update(num_latents=512)
    if variant:
        c["dit"].update(guidance_embed=True)
    if variant == "turbo":
        c["sched"].update(kind="ConsistencyFlowMatchEulerDiscreteScheduler", pcm_timesteps=100)
    return c


def config_from_yaml(doc):
    """upstream config.yaml ({model, vae, conditioner, scheduler, image_processor}.params) -> cfg dict"""
    import copy
    c = copy.deepcopy(FULL)
    mp = doc.get("model", {}).get("params", {})
    for k in c["dit"]:
        if k in mp:
            c["dit"][k] = mp[k]
    vp = doc.get("vae", {}).get("params", {})
    for k in c["vae"]:
        if k in vp:
            c["vae"][k] = vp[k]
    if "geo_decoder_downsample_ratio" in vp:       # upstream's turbo VAEs; absent = 1, and the key stays absent
        c["vae"]["geo_decoder_downsample_ratio"] = int(vp["geo_decoder_downsample_ratio"])
    enc = doc.get("conditioner", {}).get("params", {}).get("main_image_encoder", {}).get("kwargs", {})
    for k in c["cond"]:
        if k in enc.get("config", {}):
            c["cond"][k] = enc["config"][k]
    if "image_size" in enc:
        c["cond"]["image_size"] = enc["image_size"]
    sched = doc.get("scheduler", {})
    sp = sched.get("params", {})
    c["sched"].update({k: sp[k] for k in ("num_train_timesteps", "shift", "pcm_timesteps") if k in sp})
    if "target" in sched:
        # the scheduler's class by the last dotted component of its target (hy3dgen.shapegen.schedulers.<Class>)
        kind = str(sched["target"]).rsplit(".", 1)[-1]
        if kind not in _flow.SCHEDULERS:
            raise ValueError("config.yaml names the scheduler %r; implemented: %s" % (kind, ", ".join(_flow.SCHEDULERS)))
        c["sched"]["kind"] = kind
    ip = doc.get("image_processor", {}).get("params", {})
    c["proc"].update({k: ip[k] for k in ("size", "border_ratio") if k in ip})
    return c


VOLUME_DECODERS = ("vanilla", "hierarchical")


def volume_decoder_from_env():
    """R3G_VOLUME_DECODER = vanilla (default) | hierarchical: the volume decoder a pipeline starts with"""
    v = os.environ.get("R3G_VOLUME_DECODER", "vanilla")
    if v not in VOLUME_DECODERS:
        raise ValueError("R3G_VOLUME_DECODER=%r: expected one of %s" % (v, ", ".join(VOLUME_DECODERS)))
    return v


KV_SELECTIONS = ("exact", "topk")


def kv_selection_from_env():
    """R3G_KV_SELECTION = exact (default) | topk: the cross-attention of the geo decoder a pipeline starts with"""
    v = os.environ.get("R3G_KV_SELECTION", "exact")
    if v not in KV_SELECTIONS:
        raise ValueError("R3G_KV_SELECTION=%r: expected one of %s" % (v, ", ".join(KV_SELECTIONS)))
    return v


class Hunyuan3DDiTPipeline:
    accepts_image_list = True     # `image` may be a list: its objects share the launches of the denoising loop

    def __init__(self, cfg, state_dict, device="cuda", grid_chunk=0, private_ctx=False):
        dev = torch.device(device)
        self.cfg = cfg
        self.device = torch.device("cuda", dev.index or 0)
        self.private_ctx = bool(private_ctx)     # own r3g_ctx: a second pipeline that runs beside another one on this GPU
        self.model = self._make_model(cfg, state_dict, grid_chunk)
        self.image_processor = ImageProcessorV2(**cfg["proc"])
        self.last_grid = None
        self.timings = {}
        self.volume_decoder = volume_decoder_from_env()
        self.hier_band = 0.95               # |logit - mc_level| below which a coarse point is refined
        self.hier_min_resolution = 63
        self.last_hier_stats = None
        self.mc_algo = "mc"                # surface extractor of a call that passes mc_algo=None: "mc" | "dmc"
        # cross-attention of the geo decoder: "exact" | "topk" (adaptive top-k KV selection, DESIGN.md section 4d: an approximation,
        # opt-in); kv_topk None = upstream's rule (1024 of 3072 keys), kv_group / kv_stride None = the library's 8192 / 64
        self.kv_selection = kv_selection_from_env()
        self.kv_topk = None
        self.kv_group = None
        self.kv_stride = None

    # The four places where this class touches the device.  (The API-contract test that runs the reference's stage
    # script on a machine without a GPU overrides the first three, all that the reference path reaches; the product has no CPU path.)
    def _make_model(self, cfg, state_dict, grid_chunk):
        return _model.ShapeModel(cfg, state_dict, self.device.index, grid_chunk=grid_chunk,
                                 private_ctx=getattr(self, "private_ctx", False))

    def _device_ctx(self):
        return torch.cuda.device(self.device)

    def _extract_mesh(self, grid, mc_level, box_v, octree_resolution):
        return _mc.extract_mesh(grid, mc_level, box_v, octree_resolution,
                                ctx=self.model.ctx if getattr(self, "private_ctx", False) else None)

    def _extract_mesh_dmc(self, grid, mc_level, octree_resolution):
        return _dmc.extract_mesh(grid, mc_level, octree_resolution,
                                 ctx=self.model.ctx if getattr(self, "private_ctx", False) else None)

    # ---- construction (same entry points as upstream) -------------------------------------------
    @classmethod
    def from_pretrained(cls, model_path, device="cuda", dtype=None, use_safetensors=True, variant="fp16",
                        subfolder="hunyuan3d-dit-v2-0", **kwargs):
        """model_path: a local directory holding <subfolder>/config.yaml + model[.variant].safetensors (or, with
        use_safetensors=False or when no safetensors file is there, model[.variant].ckpt) -- the HF snapshot layout --, or
        'synthetic:<full|mini|full-fast|full-turbo|mini-turbo>[:seed]' for seeded synthetic weights.  A snapshot whose
        config.yaml says `guidance_embed: true` (upstream's subfolders hunyuan3d-dit-v2-0-fast, hunyuan3d-dit-v2-0-turbo,
        hunyuan3d-dit-v2-mini-turbo) loads as a guidance-distilled model: no CFG batch, the turbo ones on the consistency
        scheduler their config names.  A snapshot whose config.yaml says `geo_decoder_downsample_ratio: 4` loads with its narrow
        geo decoder; upstream's turbo VAE swap is `replace_vae(...)` (enable_flashvdm(replace_vae=True) keeps
        the snapshot's own VAE).  NOT covered: guidance-distilled texture models.  (Top-k KV selection: the attribute
        `kv_selection`.)"""
        if isinstance(model_path, str) and model_path.startswith("synthetic:"):
            parts = model_path.split(":")
            cfg = builtin_config(parts[1])
            seed = int(parts[2]) if len(parts) > 2 else 0
            return cls(cfg, _weights.synthetic_state_dict(cfg, seed, device=device), device, **kwargs)
        path = os.path.join(os.path.expanduser(model_path), subfolder)
        if not os.path.isdir(path):
            raise FileNotFoundError("model directory not found: %s (no network access: pass a local snapshot "
                                    "directory or 'synthetic:full')" % path)
        with open(os.path.join(path, "config.yaml")) as f:
            cfg = config_from_yaml(yaml.safe_load(f))
        return cls(cfg, _weights.load_safetensors_dir(path, variant, use_safetensors=use_safetensors), device, **kwargs)

    @classmethod
    def from_single_file(cls, ckpt_path, config_path, device="cuda", dtype=None, use_safetensors=None, **kwargs):
        """upstream's from_single_file: `ckpt_path` is a .safetensors file (flat, prefixed names) or a .ckpt torch pickle of
        {"model", "vae", "conditioner"} state dicts; `use_safetensors` None = by the file's extension"""
        with open(config_path) as f:
            cfg = config_from_yaml(yaml.safe_load(f))
        if use_safetensors is None:
            use_safetensors = str(ckpt_path).endswith(".safetensors")
        if use_safetensors:
            from safetensors.torch import load_file
            sd = load_file(ckpt_path)
        else:
            sd = _weights.flatten_ckpt(torch.load(ckpt_path, map_location="cpu", weights_only=True))
        return cls(cfg, sd, device, **kwargs)

    def to(self, device=None, dtype=None):
        return self

    # ---- stages --------------------------------------------------------------------------------------
    def prepare_image(self, image):
        if isinstance(image, str) and not os.path.exists(image):
            raise FileNotFoundError("Couldn't find image at path " + image)
        return self.image_processor(image)

    def encode_cond(self, image):
        """conditioner(image) and its unconditional (zeros) twin -> bf16 [2, tokens, dim] = [cond, uncond]"""
        x = conditioner_transform(image, self.cfg["cond"]["image_size"])[0]
        return self._encode_prepared(x)

    def _encode_prepared(self, x):
        cond = self.model.cond_encode(x)
        return torch.stack([cond, torch.zeros_like(cond)], dim=0)

    # ---- host side of an object, ahead of time -------------------------------------------------------
    # Everything an image needs before it meets the GPU (open / recentre / INTER_AREA resize / composite: ImageProcessorV2, then
    # the conditioner's resize to 518 and normalisation) is ~15-40 ms of host work per crop (measured on the GPU box).  A service
    # that runs crop after crop does it for the NEXT launch group on a host thread while the GPU is in the current group's 49
    # evaluations, instead of in front of every group with the GPU idle: `prefetch(images)` starts it, the `__call__` on the same
    # image objects picks the results up (any other call simply prepares its images itself).  Same functions, same results.
    # Round 5: (a) several groups may be pending at once, keyed by the identity of their image objects -- the callers issue
    # prefetch(next group) BEFORE they run the current one, and round 4's single slot was overwritten by exactly that call, so
    # that only a run's last group was ever picked up (every other crop was prepared twice: ADVICE r4); (b) the host path runs no
    # torch operator any more (preprocessors.py: numpy / scipy.sparse / PIL, all single-threaded), so the pool no longer touches
    # torch's process-wide intra-op thread count; (c) the timing sum is updated under a lock.
    _PREFETCH_MAX_GROUPS = 4

    def _host_prepare(self, image):
        import time
        t0 = time.perf_counter()
        x = conditioner_transform(self.prepare_image(image)["image"], self.cfg["cond"]["image_size"])[0]
        dt = time.perf_counter() - t0
        with self._timings_lock():
            self.timings["host_prepare_s"] = self.timings.get("host_prepare_s", 0.0) + dt
            self.timings["host_prepare_n"] = self.timings.get("host_prepare_n", 0) + 1
        return x

    def _timings_lock(self):
        lock = self.__dict__.get("_tlock")
        if lock is None:
            import threading
            lock = self.__dict__.setdefault("_tlock", threading.Lock())
        return lock

    def prefetch(self, images):
        """start the host-side preparation of `images` (a coming call's objects) on a background thread; a later call made with
        any of these image OBJECTS picks their results up.  Round 6: kept per image (identity), not per group -- a caller whose
        groups are cut differently from its prefetches (bench.py: a warm-up of 5 crops in groups of 4) still gets every crop
        prepared once, on the worker.  At most _PREFETCH_MAX_GROUPS x 8 images pending; the oldest nobody came for go first."""
        import collections
        import concurrent.futures
        if getattr(self, "_prefetch_pool", None) is None:
            self._prefetch_pool = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="r3g-host-prep")
            self._prefetched = collections.OrderedDict()
        images = list(images) if isinstance(images, (list, tuple)) else [images]
        for im in images:
            if id(im) in self._prefetched:
                continue
            while len(self._prefetched) >= self._PREFETCH_MAX_GROUPS * 8:
                _, (_, fut) = self._prefetched.popitem(last=False)
                fut.cancel()
            self._prefetched[id(im)] = (im, self._prefetch_pool.submit(self._host_prepare, im))     # (the image is kept alive: its id stays its own)

    def close_prefetch(self):
        """stop the host-preparation thread (pending images are dropped)"""
        pool = getattr(self, "_prefetch_pool", None)
        if pool is not None:
            pool.shutdown(wait=True)
            self._prefetch_pool = None
            self._prefetched = {}

    def _prepared(self, images):
        """the prepared conditioner inputs of `images`: from the prefetch where one was started for the same image object"""
        pending = getattr(self, "_prefetched", None)
        out = []
        for im in images:
            hit = pending.pop(id(im), None) if pending else None
            if hit is not None and hit[0] is im and not hit[1].cancelled():
                with self._timings_lock():
                    self.timings["prefetch_hits"] = self.timings.get("prefetch_hits", 0) + 1
                out.append(hit[1].result())
            else:
                out.append(self._host_prepare(im))
        return out

    def prepare_latents(self, generator):
        shape = (self.model.num_latents, self.model.in_channels)
        # diffusers.randn_tensor with a CPU generator: drawn on the CPU IN THE PIPELINE DTYPE (upstream: fp16), then moved --
        # the same seed gives the same initial latents as the reference, bit for bit; the sampler then runs on their fp32
        # image (R3G_NOISE_DTYPE=float32 restores the first round's fp32 draw)
        dt = torch.float32 if os.environ.get("R3G_NOISE_DTYPE", "float16") == "float32" else torch.float16
        if generator is not None and generator.device.type != "cpu":
            return torch.randn(shape, generator=generator, device=generator.device, dtype=dt).float().to(self.device)
        return torch.randn((1,) + shape, generator=generator, device="cpu", dtype=dt)[0].float().to(self.device)

    def _latents_for(self, generator, n):
        """initial latents of n objects, f32 [n, N, C].  One generator (or None): ONE draw of shape (n, N, C), as upstream's
        prepare_latents does for a list of images; a list of n generators: one (1, N, C) draw each (diffusers.randn_tensor) --
        object i then gets exactly what a single-image call with generator[i] would give it."""
        if isinstance(generator, (list, tuple)):
            if len(generator) != n:
                raise ValueError("%d generators for %d images" % (len(generator), n))
            return torch.stack([self.prepare_latents(g) for g in generator], dim=0)
        shape = (n, self.model.num_latents, self.model.in_channels)
        dt = torch.float32 if os.environ.get("R3G_NOISE_DTYPE", "float16") == "float32" else torch.float16
        if generator is not None and generator.device.type != "cpu":
            return torch.randn(shape, generator=generator, device=generator.device, dtype=dt).float().to(self.device)
        return torch.randn(shape, generator=generator, device="cpu", dtype=dt).float().to(self.device)

    def generate_latents(self, images, num_inference_steps, guidance_scale, generator, sigmas=None):
        """preprocess + conditioner per image, then ALL objects through the denoising loop together
        (r3g_flow_sample_batch: every DiT layer is one launch over the objects' rows; per-object results do not depend on
        the company an object keeps) -> f32 [n, N, C]"""
        cond2 = torch.stack([self._encode_prepared(x) for x in self._prepared(images)], dim=0)
        latents = self._latents_for(generator, len(images))
        shift = self.cfg["sched"].get("shift", 1.0)
        sched = self.cfg["sched"]
        if sigmas is not None or getattr(self.model, "guidance_embed", False) or \
                sched.get("kind", _flow.SCHEDULERS[0]) != _flow.SCHEDULERS[0]:
            # an explicit table, the consistency scheduler, or a guidance-distilled model (no CFG batch: one entry per object,
            # up to 8 objects per launch; guidance_scale only feeds guidance_in)
            table = _flow.scheduler_sigmas(sched, num_inference_steps, sigmas)
            return self.model.flow_sample_sigmas(latents, cond2, table, guidance_scale, uncond_uniform=True)
        if len(images) == 1:
            return self.model.flow_sample(latents[0], cond2[0], num_inference_steps, guidance_scale, shift,
                                          uncond_uniform=True)[None]          # zeros_like(cond)
        return self.model.flow_sample_batch(latents, cond2, num_inference_steps, guidance_scale, shift, uncond_uniform=True)

    # ---- volume decoder --------------------------------------------------------------------------------
    def enable_flashvdm(self, enabled=True, adaptive_kv_selection=True, topk_mode="mean", mc_algo="mc", replace_vae=True):
        """upstream's switch to its hierarchical volume decoder.  Here: `enabled` selects hierarchical volume decoding
        (r3g_grid_query_hier: a coarse grid densely, then only the points near the surface; defined in DESIGN.md, modelled on
        upstream's decoder but not pinned to it) and enable_flashvdm(False) restores the dense decoder.  `adaptive_kv_selection`,
        `topk_mode` and `replace_vae` are accepted and IGNORED (the VAE swap is the method `replace_vae(model_path, ...)`, not this flag: its
        default is True upstream, so honouring it would change the decoder of every enable_flashvdm() caller).  Top-k KV selection exists but is chosen
        with the pipeline attribute `kv_selection = "topk"` (R3G_KV_SELECTION, stage key `r3g_kv_selection`), not here: this
        signature is upstream's and its default is True, so honouring it would turn every enable_flashvdm() caller into an
        approximation -- after this call the cross-attention is what `kv_selection` says, "exact" unless set.  The surface extractor is NOT chosen here: mc_algo other than 'mc' is
        refused; dual marching cubes is selected per call (`pipeline(image, mc_algo="dmc")`) or by the pipeline attribute
        `mc_algo` ("mc" | "dmc"), which a call that passes mc_algo=None uses."""
        if mc_algo not in (None, "mc"):
            raise NotImplementedError("enable_flashvdm selects the volume decoder only: choose the surface extractor with "
                                      "pipeline(image, mc_algo='dmc') or pipeline.mc_algo = 'dmc'")
        self.volume_decoder = "hierarchical" if enabled else "vanilla"

    def replace_vae(self, model_path, subfolder="hunyuan3d-vae-v2-0-turbo", variant="fp16", use_safetensors=True):
        """upstream's turbo VAE swap (what its enable_flashvdm(replace_vae=True) does): replace the WHOLE VAE --
        post_kl, transformer, geo decoder, scale_factor -- by the one under <model_path>/<subfolder>/ (config.yaml + model[.variant]
        .safetensors | .ckpt, keys without prefix; upstream's subfolders hunyuan3d-vae-v2-0-turbo / hunyuan3d-vae-v2-mini-turbo), or
        by 'synthetic:turbo-vae[:seed]': this pipeline's own VAE dims with geo_decoder_downsample_ratio 4, MLP expand ratio 1 and no
        ln_post, seeded synthetic weights.  num_latents and embed_dim must equal the DiT's (ValueError).  The latents are then
        divided by the new VAE's scale_factor; the DiT and the conditioner are untouched and not uploaded again; the query-side
        cache is rebuilt on the next grid query.  timings["vae"] names what decodes."""
        if isinstance(model_path, str) and model_path.startswith("synthetic:"):
            parts = model_path.split(":")
            if parts[1] != "turbo-vae":
                raise KeyError("replace_vae: %r (the synthetic VAE is 'synthetic:turbo-vae[:seed]')" % model_path)
            vcfg = _weights.turbo_vae_config(self.cfg["vae"])
            sd = _weights.synthetic_vae_state_dict(vcfg, int(parts[2]) if len(parts) > 2 else 0, device=self.device)
            name = model_path
        else:
            path = os.path.join(os.path.expanduser(model_path), subfolder)
            if not os.path.isdir(path):
                raise FileNotFoundError("VAE directory not found: %s (no network access: pass a local snapshot directory or "
                                        "'synthetic:turbo-vae')" % path)
            params, sd = _weights.load_vae_dir(path, variant, use_safetensors=use_safetensors)
            vcfg = dict(self.cfg["vae"])
            for k in list(vcfg) + ["geo_decoder_downsample_ratio"]:
                if k in params:
                    vcfg[k] = params[k]
            if "geo_decoder_downsample_ratio" not in params:
                vcfg.pop("geo_decoder_downsample_ratio", None)
            name = path
        self.replace_vae_tensors(vcfg, sd, name)

    def replace_vae_tensors(self, vcfg, vae_state_dict, name="tensors"):
        """replace_vae with the VAE given as (config, 'vae.'-prefixed state dict)"""
        with self._device_ctx():
            self.model.replace_vae(vcfg, vae_state_dict)
        self.cfg = dict(self.cfg)
        self.cfg["vae"] = dict(vcfg)
        self.vae_name = name
        self.timings["vae"] = name

    def _apply_kv_selection(self):
        """hand `kv_selection` (and kv_topk / kv_group / kv_stride) to the model ahead of a grid query; timings["kv_selection"]
        says what the query runs with"""
        mode = getattr(self, "kv_selection", "exact")
        if mode not in KV_SELECTIONS:
            raise ValueError("kv_selection=%r: expected one of %s" % (mode, ", ".join(KV_SELECTIONS)))
        if mode == "topk":
            topk = getattr(self, "kv_topk", None)
            kept = self.model.set_kv_selection(-1 if topk is None else topk, getattr(self, "kv_group", None),
                                               getattr(self, "kv_stride", None))
            self.timings["kv_selection"] = "topk:%d" % kept
        else:
            # (the library's options are process-wide: an exact pipeline switches off what a top-k one beside it left on)
            reset = getattr(self.model, "set_kv_selection", None)
            if reset is not None:
                reset(0)
            self.timings["kv_selection"] = "exact"

    def _query_grid(self, box_v, octree_resolution, mc_level):
        """the occupancy grid of the object whose latents the VAE has just decoded: always a full (R+1)^3 tensor"""
        self._apply_kv_selection()
        n_dense = (octree_resolution + 1) ** 3
        if getattr(self, "volume_decoder", "vanilla") == "hierarchical":
            grid, stats = self.model.grid_query_hier(box_v, octree_resolution, mc_level, self.hier_band, self.hier_min_resolution)
            self.last_hier_stats = stats
            self.timings["grid_points_evaluated"] = stats["evaluated"]
        else:
            grid = self.model.grid_query(box_v, octree_resolution)
            self.last_hier_stats = None
            self.timings["grid_points_evaluated"] = n_dense
        return grid

    def generate_grid(self, image, num_inference_steps, guidance_scale, generator, box_v, octree_resolution, mc_level=None,
                      sigmas=None):
        import time
        t0 = time.perf_counter()
        latents = self.generate_latents([image], num_inference_steps, guidance_scale, generator, sigmas=sigmas)[0]
        self.model.vae_decode(latents)
        self.timings["vae"] = getattr(self, "vae_name", "checkpoint")
        grid = self._query_grid(box_v, octree_resolution, self.cfg["mc_level"] if mc_level is None else mc_level)
        self.timings["grid_s"] = time.perf_counter() - t0
        return grid, latents

    def _resolve_mc_algo(self, mc_algo):
        algo = getattr(self, "mc_algo", "mc") if mc_algo is None else mc_algo
        if algo not in ("mc", "dmc"):
            raise NotImplementedError("mc_algo=%r: the surface extractors are 'mc' (Lewiner marching cubes) and 'dmc' "
                                      "(dual marching cubes)" % (algo,))
        return algo

    def _mesh_from_grid(self, grid, mc_level, box_v, octree_resolution, output_type, mc_algo="mc"):
        try:
            if mc_algo == "dmc":
                v, f = self._extract_mesh_dmc(grid, mc_level, octree_resolution)
            else:
                v, f = self._extract_mesh(grid, mc_level, box_v, octree_resolution)
        except (ValueError, RuntimeError) as e:   # upstream: traceback + None for this object
            print("[hy3dgen] surface extraction failed: %s" % e)
            return None
        if output_type == "trimesh":
            return Mesh.from_device(v, f)   # stays in HBM for the cleaners; host arrays on first read
        return (v, f)

    @torch.no_grad()
    def __call__(self, image=None, num_inference_steps=50, timesteps=None, sigmas=None, eta=0.0, guidance_scale=None,
                 generator=None, box_v=None, octree_resolution=384, mc_level=None, mc_algo=None, num_chunks=8000,
                 output_type="trimesh", enable_pbar=True, **kwargs):
        """image: one PIL image / path (the reference's call, src/2d_to_3d_models/run.py:77-84) or a list of them (upstream's
        batch dimension): the objects of a list share every launch of the denoising loop and are decoded one after the
        other; the result has one entry per image.  `sigmas`: an explicit strictly ascending table inside [0, 1] replaces the
        scheduler's (it gets the trailing 1 as upstream's set_timesteps does; anything else is a ValueError).  A
        guidance-distilled model runs without the CFG batch and groups up to 8 objects of a list per launch.  `mc_algo`:
        "mc" (Lewiner marching cubes, the reference path), "dmc" (dual marching cubes, DESIGN.md section 4c: vertices in
        upstream's dmc frame, box_v not applied) or None for the pipeline attribute `mc_algo`; anything else is a
        NotImplementedError."""
        if image is None:
            raise ValueError("image is required")
        if sigmas is not None:
            _flow.scheduler_sigmas(self.cfg["sched"], num_inference_steps, sigmas)      # refuse a bad table before any GPU work
        mc_algo = self._resolve_mc_algo(mc_algo)
        g = self.cfg["guidance_scale"] if guidance_scale is None else guidance_scale
        box_v = self.cfg["box_v"] if box_v is None else box_v
        mc_level = self.cfg["mc_level"] if mc_level is None else mc_level
        with self._device_ctx():
            if isinstance(image, (list, tuple)):
                import time
                t0 = time.perf_counter()
                latents = self.generate_latents(list(image), num_inference_steps, g, generator, sigmas=sigmas)
                out = []
                self.timings["vae"] = getattr(self, "vae_name", "checkpoint")
                for i in range(len(image)):
                    self.model.vae_decode(latents[i])
                    grid = self._query_grid(box_v, octree_resolution, mc_level)
                    self.last_grid = grid
                    out.append(self._mesh_from_grid(grid, mc_level, box_v, octree_resolution, output_type, mc_algo))
                self.timings["grid_s"] = time.perf_counter() - t0
                return out
            grid, latents = self.generate_grid(image, num_inference_steps, g, generator, box_v, octree_resolution, mc_level,
                                               sigmas=sigmas)
            self.last_grid = grid
            return [self._mesh_from_grid(grid, mc_level, box_v, octree_resolution, output_type, mc_algo)]


class Hunyuan3DDiTFlowMatchingPipeline(Hunyuan3DDiTPipeline):
    pass
