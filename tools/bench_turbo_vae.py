#!/usr/bin/env python3
"""Measures the turbo shape VAE on one MI355X; prints one JSON line.

    python tools/bench_turbo_vae.py [--part a|b|ab] [--reps 5] [--resolution 256] [--objects 8]

(a) One process, one object's latents, full VAE dims (width 1024, 16 heads, 16 layers, 3072 latents).  Three decoders alternate
    A/B/C/A/B/C, `--reps` times each after a warm-up of every one:
      A  the standard VAE (geo decoder at width 1024, MLP ratio 4, ln_post),
      B  the turbo VAE (r = 4, e = 1, no ln_post: width 256, 4 heads) with option geo_narrow_fused = 0 (the generic launches),
      C  the same turbo VAE with geo_narrow_fused = 1 (the fused tail, csrc/geo_narrow.hip).
    Per decoder: milliseconds per dense (R+1)^3 grid by device events around r3g_grid_query with the query-side cache warm,
    per-family milliseconds of one further query (r3g_prof_*), the query-side cache's size, and the milliseconds of r3g_vae_decode.  The two VAEs live in separate
    contexts so that alternating does not re-install them; only their VAE tensors are created (the DiT does not run here).
(b) Objects per second of `synthetic:full-turbo` through the pipeline (5 consistency steps, dense grid, marching cubes, `--objects`
    per launch), as tools/bench_distilled.py part (b) measures it, with its own VAE and with `replace_vae("synthetic:turbo-vae")`
    under geo_narrow_fused = 0 and 1.
No threshold: the first numbers of their kind.
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


def families(fn, per=1):
    from r3g import ffi
    L = ffi.lib()
    n = len(FAMILIES)
    cnt, ms, work = (ctypes.c_int64 * n)(), (ctypes.c_double * n)(), (ctypes.c_double * n)()
    ffi.check(L.r3g_prof_enable(1))
    fn()
    torch.cuda.synchronize()
    ffi.check(L.r3g_prof_read(cnt, ms, work, n))
    ffi.check(L.r3g_prof_enable(0))
    return {FAMILIES[i]: {"launches": int(cnt[i]), "ms": float(ms[i]) / per} for i in range(n) if cnt[i]}


def set_fused(v):
    from r3g import ffi
    ffi.check(ffi.lib().r3g_set_option(b"geo_narrow_fused", int(v)))


def part_a(a):
    from hy3dgen.shapegen.pipelines import builtin_config
    from r3g import ffi, model as M, weights as W
    cfg = builtin_config("full")
    tcfg = dict(cfg, vae=W.turbo_vae_config(cfg["vae"]))
    m_std = M.ShapeModel(cfg, W.synthetic_vae_state_dict(cfg["vae"], 0, device="cuda"), 0)
    m_tur = M.ShapeModel(tcfg, W.synthetic_vae_state_dict(tcfg["vae"], 7, device="cuda"), 0, private_ctx=True)
    R = a.resolution
    lat = torch.randn(cfg["vae"]["num_latents"], cfg["vae"]["embed_dim"], generator=torch.Generator().manual_seed(5)).cuda()
    out = torch.empty((R + 1,) * 3, dtype=torch.float32, device="cuda")
    variants = (("A_standard", m_std, None), ("B_turbo_generic", m_tur, 0), ("C_turbo_fused", m_tur, 1))

    def query(m, fused):
        if fused is not None:
            set_fused(fused)                        # (no new option epoch: the query-side cache stays valid)
        return lambda: m.grid_query(1.01, R, out=out)
    vae_ms = {}
    for name, m, fused in variants:                  # warm-up: arenas, caches, every launch shape
        m.vae_decode(lat)
        vae_ms[name] = timed(lambda: m.vae_decode(lat))
        query(m, fused)()
        query(m, fused)()
    torch.cuda.synchronize()
    ms = {k: [] for k, _, _ in variants}
    n0 = ffi.counter("geo_narrow_passes")
    for _ in range(max(3, a.reps)):
        for name, m, fused in variants:
            ms[name].append(timed(query(m, fused)))
    fused_passes = ffi.counter("geo_narrow_passes") - n0
    fam = {name: families(query(m, fused)) for name, m, fused in variants}
    points = (R + 1) ** 3
    passes = (points + 131072 - 1) // 131072

    def cache_gb(width):
        return passes * 131072 * width * 2 * 2 / 1e9
    med = {k: statistics.median(v) for k, v in ms.items()}
    from r3g import meshdist
    query(m_tur, 0)()              # the fused tail against the generic launches of the same decoder, as meshes
    generic_grid = out.clone()
    query(m_tur, 1)()
    mesh_distance = dict(meshdist.grid_mesh_distance(generic_grid, out, 0.0, 1.01, R), between="B_turbo_generic / C_turbo_fused")
    del generic_grid
    set_fused(0)
    for m in (m_std, m_tur):
        m.trim()
    return {"octree_resolution": R, "grid_points": points, "ms_per_grid": {k: summary(v) for k, v in ms.items()},
            "families_ms_per_grid": fam, "vae_decode_ms": vae_ms, "fused_passes_counted": fused_passes,
            "query_side_cache_gb": {"standard_width_1024": cache_gb(1024), "turbo_width_256": cache_gb(256)},
            "ratio_B_over_A": med["B_turbo_generic"] / med["A_standard"], "ratio_C_over_A": med["C_turbo_fused"] / med["A_standard"],
            "ratio_C_over_B": med["C_turbo_fused"] / med["B_turbo_generic"],
            "fused_faster_than_generic": bool(med["C_turbo_fused"] < med["B_turbo_generic"]), "mesh_distance": mesh_distance}


def part_b(a):
    from bench import synthetic_crop
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    pipe = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained("synthetic:full-turbo:0")
    crops = [synthetic_crop(j) for j in range(a.objects)]
    R = a.resolution

    def run():
        return pipe(image=crops, num_inference_steps=5, octree_resolution=R, num_chunks=16000,
                    generator=[torch.Generator().manual_seed(1234567) for _ in crops], output_type="raw")

    def rate(tag):
        run()                                        # warm-up: arenas, the query-side cache, every launch shape
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        meshes = run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        fam = families(run, a.objects)
        return {"vae": pipe.timings.get("vae"), "objects": a.objects, "seconds": dt, "objects_per_s": a.objects / dt,
                "ms_per_object": 1e3 * dt / a.objects, "meshes": sum(m is not None for m in meshes),
                "families_ms_per_object": fam}
    rep = {"model": "synthetic:full-turbo", "inference_steps": 5, "octree_resolution": R, "own_vae": rate("own")}
    pipe.replace_vae("synthetic:turbo-vae:7")
    for fused in (0, 1):
        set_fused(fused)
        rep["turbo_vae_fused_%d" % fused] = rate("turbo")
    set_fused(0)
    pipe.model.trim()
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--objects", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_turbo_vae.py needs an MI355X (the product has no CPU path)")
    rep = {"bench": "turbo_vae"}
    if "a" in a.part:
        rep["decoders"] = part_a(a)
    if "b" in a.part:
        rep["pipeline"] = part_b(a)
    print(json.dumps(rep), flush=True)


if __name__ == "__main__":
    main()
