#!/usr/bin/env python3
"""Times the hierarchical volume decoder (r3g_grid_query_hier) against the dense grid query on the full-size geo decoder.

    python tools/bench_hier.py [--resolution 256] [--reps 5] [--field object-like|noise-like] [--band 0.95]

One process, after a warm-up of every variant: dense with the query-side cache, dense with `geo_q_cache` off (the decoder's full
per-point cost, what the hierarchical decoder's listed points pay too) and hierarchical, alternating, `--reps` times each, timed with
device events.  Prints one JSON line: the evaluated share f, milliseconds per variant (median, min, max), microseconds per
evaluated point of the hierarchical and the uncached dense decoder with the dense decoder's repetition spread beside them, and the
planner passes' (select, index list, merge) time and bytes from r3g_prof_* with their share of the 6.3 TB/s HBM rate.
"object-like" zeroes the Fourier frequencies above 2^1 in query_proj (the recipe of tests/test_cfg4_gpu.py); "noise-like" leaves
the synthetic weights as they are.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))
import torch  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
PC_ELEMWISE, PC_COUNT = 5, 9       # csrc/prof.h


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def prof_elementwise(L):
    counts, ms, work = (ctypes.c_int64 * PC_COUNT)(), (ctypes.c_double * PC_COUNT)(), (ctypes.c_double * PC_COUNT)()
    assert L.r3g_prof_read(counts, ms, work, PC_COUNT) == 0
    return int(counts[PC_ELEMWISE]), float(ms[PC_ELEMWISE]), float(work[PC_ELEMWISE])


def planner_profile(m, L, R, level, band):
    """the planner passes of one decode on their own (the decoder's launches run with the profile off): scopes, ms, bytes"""
    from r3g import ffi, hier
    lv = hier.levels(R)
    n0 = lv[0] + 1
    ffi.check(L.r3g_set_option(b"geo_q_cache", 0))
    try:
        grid = m.grid_query(1.01, lv[0])
    finally:
        ffi.check(L.r3g_set_option(b"geo_q_cache", 1))
    assert tuple(grid.shape) == (n0, n0, n0)
    tot = [0, 0.0, 0.0]
    for li in range(1, len(lv)):
        L.r3g_prof_enable(1)
        count = hier.select(grid, level, band, li == len(lv) - 1, m.ctx)
        idx = hier.indices(count, grid.device, m.ctx)
        torch.cuda.synchronize()
        a = prof_elementwise(L)
        L.r3g_prof_enable(0)
        vals = m.grid_query_points(1.01, lv[li], idx)
        L.r3g_prof_enable(1)
        grid = hier.merge(grid, vals, m.ctx)
        torch.cuda.synchronize()
        b = prof_elementwise(L)
        L.r3g_prof_enable(0)
        tot = [tot[0] + a[0] + b[0], tot[1] + a[1] + b[1], tot[2] + a[2] + b[2] + 8.0 * count]    # + index store and value load
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--field", default="object-like", choices=("object-like", "noise-like"))
    ap.add_argument("--band", type=float, default=0.95)
    ap.add_argument("--band-rel", type=float, default=None, help="band = this x max |logit| of the coarsest level instead of --band")
    a = ap.parse_args()
    from hy3dgen.shapegen.pipelines import builtin_config
    from r3g import ffi, hier, model as M, weights as W
    L = ffi.lib()
    cfg = builtin_config("full")
    sd = W.synthetic_state_dict(cfg, 0, device="cuda")
    if a.field == "object-like":
        w = sd["vae.geo_decoder.query_proj.weight"].clone()
        for c in range(3):
            for k in range(2, 8):
                w[:, 3 + c * 8 + k] = 0
                w[:, 27 + c * 8 + k] = 0
        sd["vae.geo_decoder.query_proj.weight"] = w
    R, n = a.resolution, a.resolution + 1
    m = M.ShapeModel(cfg, sd, 0)
    lat = torch.randn(cfg["vae"]["num_latents"], cfg["vae"]["embed_dim"], generator=torch.Generator().manual_seed(21)).cuda()
    m.vae_decode(lat)
    out = torch.empty((n, n, n), dtype=torch.float32, device="cuda")
    band = a.band
    if a.band_rel is not None:
        ffi.check(L.r3g_set_option(b"geo_q_cache", 0))
        band = a.band_rel * float(m.grid_query(1.01, hier.levels(R)[0]).abs().max())
        ffi.check(L.r3g_set_option(b"geo_q_cache", 1))

    def dense_cached():
        m.grid_query(1.01, R, out)

    def dense_uncached():
        ffi.check(L.r3g_set_option(b"geo_q_cache", 0))
        try:
            m.grid_query(1.01, R, out)
        finally:
            ffi.check(L.r3g_set_option(b"geo_q_cache", 1))

    def hierarchical():
        m.grid_query_hier(1.01, R, 0.0, band, out=out, stats=False)

    variants = (("dense_cached", dense_cached), ("dense_uncached", dense_uncached), ("hierarchical", hierarchical))
    dense_cached()                 # builds the cache
    for _, fn in variants:         # warm-up: every shape of the timed window
        fn()
    torch.cuda.synchronize()
    _, stats = m.grid_query_hier(1.01, R, 0.0, band)
    ms = {k: [] for k, _ in variants}
    for _ in range(max(5, a.reps)):
        for k, fn in variants:
            ms[k].append(timed(fn))
    p_scopes, p_ms, p_bytes = planner_profile(m, L, R, 0.0, band)
    dense_cached()                 # the error in space: the dense and the hierarchical grid through marching cubes
    dense_grid = out.clone()
    hierarchical()
    from r3g import meshdist
    mesh_distance = meshdist.grid_mesh_distance(dense_grid, out, 0.0, 1.01, R)
    del dense_grid

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
    du, hi = statistics.median(ms["dense_uncached"]), statistics.median(ms["hierarchical"])
    us_dense = 1e3 * du / stats["dense_points"]
    us_hier = 1e3 * hi / stats["evaluated"]
    spread = (max(ms["dense_uncached"]) - min(ms["dense_uncached"])) / du
    print(json.dumps({
        "bench": "hier_decode", "field": a.field, "resolution": R, "band": band, "levels": stats["levels"],
        "evaluated_per_level": stats["evaluated_per_level"], "evaluated": stats["evaluated"], "dense_points": stats["dense_points"],
        "f": stats["evaluated"] / stats["dense_points"], "unsafe_cells": stats["unsafe_cells"], "mesh_distance": mesh_distance,
        "ms": {k: summary(v) for k, v in ms.items()},
        "us_per_point_dense_uncached": us_dense, "us_per_point_hierarchical": us_hier,
        "per_point_ratio_hier_over_dense_uncached": us_hier / us_dense, "dense_uncached_spread": spread,
        "planner": {"profile_scopes": p_scopes, "ms": p_ms, "bytes": p_bytes,
                    "share_of_hbm_rate": (p_bytes / HBM_BYTES_PER_S) / (p_ms * 1e-3) if p_ms > 0 else None,
                    "share_of_hierarchical_ms": p_ms / hi},
    }), flush=True)


if __name__ == "__main__":
    main()
