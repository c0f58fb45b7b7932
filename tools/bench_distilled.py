#!/usr/bin/env python3
"""Measures the guidance-distilled shape models on one MI355X; prints one JSON line.

    python tools/bench_distilled.py [--part a|b|ab] [--reps 5] [--evals 4] [--objects 8] [--resolution 256] [--no-default]

(a) Milliseconds per DiT evaluation per object at full dims (hunyuan3d-dit-v2-0: 16 + 32 blocks, 3072 + 1370 tokens), one process:
    the CFG engine at 4 objects per launch against the CFG-free engine at 4 and at 8, after a warm-up of every variant,
    alternating, `--reps` times each, device events around `--evals` whole evaluations (r3g_flow_sample_sigmas on a table without a
    zero step, the fp16 stream's guard included as in production).  The two models live in separate contexts so that alternating
    does not re-install them.  By row count alone the CFG-free evaluation of 4 objects pushes 57 % of the CFG group's rows through
    every GEMM (4 x 3072 + 4 x 1370 against 8 x 3072 + 4 x 1371) and does 68 % of its attention work; the bound fixed in advance is
    only that the CFG-free figure lies BELOW the CFG figure of the same run ("cfg_free_below_cfg").
(b) Objects per second of `synthetic:full-turbo` through the pipeline (5 consistency steps, dense (R+1)^3 grid, marching cubes,
    `--objects` per launch; wall clock around one call after a warm-up call) with the per-family milliseconds per object of
    r3g_prof_* from one further call, and -- unless --no-default -- `synthetic:full` (50 steps, CFG, 4 per launch) run the same way
    beside it.  No threshold: the first number of its kind.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))
import torch  # noqa: E402

FAMILIES = ["gemm", "attention", "layernorm", "qkv_split", "gemv", "elementwise", "mc_classify", "mc_other", "mesh"]   # csrc/prof.h


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def part_a(a):
    from hy3dgen.shapegen.pipelines import builtin_config
    from r3g import ffi, flow, model as M, weights as W
    cfg_c, cfg_d = builtin_config("full"), builtin_config("full-turbo")
    sd = W.synthetic_state_dict(cfg_d, 0, device="cuda")          # the undistilled tensors are the same draw (key order)
    sd_c = {k: v for k, v in sd.items() if k not in W.GUIDANCE_KEYS}
    m_c = M.ShapeModel(cfg_c, sd_c, 0)
    m_d = M.ShapeModel(cfg_d, sd, 0, private_ctx=True)
    del sd, sd_c
    Nl, C = cfg_c["vae"]["num_latents"], cfg_c["dit"]["in_channels"]
    Lc = (cfg_c["cond"]["image_size"] // cfg_c["cond"]["patch_size"]) ** 2 + 1
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(8, Nl, C, generator=g).cuda()
    cond2 = torch.zeros(8, 2, Lc, cfg_c["dit"]["context_in_dim"], dtype=torch.bfloat16)
    cond2[:, 0] = torch.randn(8, Lc, cfg_c["dit"]["context_in_dim"], generator=g).to(torch.bfloat16)
    cond2 = cond2.cuda()
    K = max(1, a.evals)
    sig = flow.consistency_sigmas(K)                              # K steps, K evaluations (no zero step)

    def run(m, n):
        return lambda: m.flow_sample_sigmas(lat[:n].clone(), cond2[:n], sig, 5.0, uncond_uniform=True)
    variants = (("cfg_4", run(m_c, 4), 4), ("cfg_free_4", run(m_d, 4), 4), ("cfg_free_8", run(m_d, 8), 8))
    f0 = ffi.counter("dit_f16_fallbacks")
    for _ in range(2):
        for _, fn, _ in variants:
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _, _ in variants}
    for _ in range(max(3, a.reps)):
        for k, fn, n in variants:
            ms[k].append(timed(fn) / K / n)
    med = {k: statistics.median(v) for k, v in ms.items()}
    rows_cfg, rows_free = 8 * Nl + 4 * (Lc + 1), 4 * Nl + 4 * Lc
    T = Nl + Lc
    keys_cfg, keys_free = 4 * (T * T + (Nl + 1) * (Nl + 1)), 4 * T * T
    return {"evaluations_per_call": K, "ms_per_evaluation_per_object": {k: summary(v) for k, v in ms.items()},
            "ratio_cfg_free_4_over_cfg_4": med["cfg_free_4"] / med["cfg_4"],
            "ratio_cfg_free_8_over_cfg_4": med["cfg_free_8"] / med["cfg_4"],
            "predicted_by_rows": rows_free / rows_cfg, "predicted_by_attention_pairs": keys_free / keys_cfg,
            "cfg_free_below_cfg": bool(med["cfg_free_4"] < med["cfg_4"] and med["cfg_free_8"] < med["cfg_4"]),
            "cfg_4_spread": (max(ms["cfg_4"]) - min(ms["cfg_4"])) / med["cfg_4"],
            "dit_f16_fallbacks": ffi.counter("dit_f16_fallbacks") - f0}


def pipeline_rate(name, steps, per_launch, n_objects, R):
    from bench import synthetic_crop
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    from r3g import ffi
    L = ffi.lib()
    pipe = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained("synthetic:%s:0" % name)
    crops = [synthetic_crop(j) for j in range(n_objects)]

    def run():
        out = []
        for g0 in range(0, n_objects, per_launch):
            imgs = crops[g0:g0 + per_launch]
            out += pipe(image=imgs, num_inference_steps=steps, octree_resolution=R, num_chunks=16000,
                        generator=[torch.Generator().manual_seed(1234567) for _ in imgs], output_type="raw")
        return out
    run()                                                           # warm-up: arenas, the query-side cache, every launch shape
    torch.cuda.synchronize()
    e0, f0 = ffi.counter("dit_evals"), ffi.counter("dit_f16_fallbacks")
    t0 = time.perf_counter()
    meshes = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    evals = ffi.counter("dit_evals") - e0
    n = len(FAMILIES)
    cnt, ms, work = (ctypes.c_int64 * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
    ffi.check(L.r3g_prof_enable(1))
    run()
    torch.cuda.synchronize()
    ffi.check(L.r3g_prof_read(cnt, ms, work, n))
    ffi.check(L.r3g_prof_enable(0))
    fam = {FAMILIES[i]: {"launches": int(cnt[i]), "ms_per_object": float(ms[i]) / n_objects} for i in range(n)}
    rep = {"model": name, "inference_steps": steps, "objects_per_launch": per_launch, "objects": n_objects, "octree_resolution": R,
           "seconds": dt, "objects_per_s": n_objects / dt, "ms_per_object": 1e3 * dt / n_objects, "dit_evaluations": evals,
           "meshes": sum(m is not None for m in meshes), "dit_f16_fallbacks": ffi.counter("dit_f16_fallbacks") - f0,
           "families_ms_per_object": fam,
           "dominant_family": max(fam, key=lambda k: fam[k]["ms_per_object"])}
    pipe.model.trim()
    del pipe
    torch.cuda.empty_cache()
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--evals", type=int, default=4)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--no-default", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distilled.py needs an MI355X (the product has no CPU path)")
    rep = {"bench": "distilled"}
    if "b" in a.part:
        rep["turbo"] = pipeline_rate("full-turbo", 5, 8, a.objects, a.resolution)
        if not a.no_default:
            rep["default"] = pipeline_rate("full", 50, 4, a.objects, a.resolution)
    if "a" in a.part:
        rep["dit_evaluation"] = part_a(a)
    print(json.dumps(rep), flush=True)


if __name__ == "__main__":
    main()
