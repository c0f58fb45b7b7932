#!/usr/bin/env python3
"""Exact cross-attention against adaptive top-k KV selection in the geo decoder, alternating in one process.

    python tools/bench_kvsel.py [--model synthetic:full] [--R 256] [--iters 3] [--topk -1] [--group 8192] [--stride 64]
                                [--decoders dense,hier]
One object (seeded latents through the VAE decoder), then per volume decoder (the dense (R+1)^3 grid query and the hierarchical
decoder) the two modes call by call.  Prints one JSON line per (decoder, mode):
  ms_median / ms_min   whole grid query, HIP events on the stream (the query-side cache is warm: it is built by the warm-up calls)
  attention_ms         the attention family per object (r3g_prof_*: HIP events around each launch, taken in calls of their own)
  regroup_ms / select_ms / gather_ms   the three kvsel kernels per object (families qkv_split, gemv, and elementwise minus what
                       the exact mode spends there; the row-major V copy, once per object, is inside gather_ms)
  *_per_pass_us        the same per pass of the dense decoder
  max_abs_dlogit / mean_abs_dlogit     against the exact mode's grid of the same decoder, and the logits' scale
  sign_flip_share      share of grid points on the other side of mc_level than in the exact grid
  mesh_distance        (top-k lines) both grids through marching cubes: chamfer_l1, hausdorff, p99, share within one voxel
Nothing is asserted: the numbers go to profiles/kvsel.md.  Synthetic N(0, 0.02^2) weights give nearly uniform attention; the errors
measured on them say nothing about a real snapshot.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic:full")
    ap.add_argument("--R", type=int, default=256, help="octree resolution: the grid has (R + 1)^3 points")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--topk", type=int, default=-1, help="keys kept per (group, head); -1: upstream's rule")
    ap.add_argument("--group", type=int, default=8192)
    ap.add_argument("--stride", type=int, default=64)
    ap.add_argument("--decoders", default="dense,hier")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    from r3g import ffi, meshdist
    pipe = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained(a.model, device="cuda:0")
    m, L = pipe.model, ffi.lib()
    bound, level = pipe.cfg["box_v"], pipe.cfg["mc_level"]
    lat = torch.randn(m.num_latents, m.in_channels, generator=torch.Generator().manual_seed(a.seed))
    m.vae_decode(lat)
    n_pts = (a.R + 1) ** 3
    passes = (n_pts + 131071) // 131072

    def query(decoder):
        if decoder == "hier":
            return m.grid_query_hier(bound, a.R, level, pipe.hier_band, pipe.hier_min_resolution)
        return m.grid_query(bound, a.R), None

    def set_mode(mode):
        return m.set_kv_selection(a.topk if mode == "topk" else 0, a.group, a.stride)

    def families():
        cnt, ms, work = (ctypes.c_int64 * 9)(), (ctypes.c_double * 9)(), (ctypes.c_double * 9)()
        ffi.check(L.r3g_prof_read(cnt, ms, work, 9))
        return list(ms)

    try:
        for decoder in a.decoders.split(","):
            modes = ("exact", "topk")
            grids, stats, kept = {}, {}, {}
            for mode in modes:                                  # warm-up: code objects, workspaces, the query-side cache
                kept[mode] = set_mode(mode)
                g, st = query(decoder)
                grids[mode], stats[mode] = g.clone(), st
            torch.cuda.synchronize()
            ev = {k: [] for k in modes}
            for _ in range(a.iters):                            # whole calls, the modes alternating
                for mode in modes:
                    set_mode(mode)
                    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    b.record()
                    query(decoder)
                    e.record()
                    ev[mode].append((b, e))
            torch.cuda.synchronize()
            fam = {}
            for mode in modes:                                  # kernel families, in calls of their own
                set_mode(mode)
                ffi.check(L.r3g_prof_enable(1))
                m.vae_decode(lat)                               # (so that the once-per-object V copy is inside the window)
                base = families()
                query(decoder)
                torch.cuda.synchronize()
                fam[mode] = [x - y for x, y in zip(families(), base)]
                ffi.check(L.r3g_prof_enable(0))
            scale = float(grids["exact"].abs().max())
            for mode in modes:
                ms = sorted(b.elapsed_time(e) for b, e in ev[mode])
                d = (grids[mode] - grids["exact"]).abs()
                flips = ((grids[mode] > level) != (grids["exact"] > level)).float().mean()
                out = {"decoder": decoder, "mode": mode, "model": a.model, "R": a.R, "points": n_pts,
                       "keys_kept": kept[mode], "group": a.group, "stride": a.stride,
                       "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "iters": a.iters,
                       "attention_ms": fam[mode][1],
                       "regroup_ms": fam[mode][3] - fam["exact"][3], "select_ms": fam[mode][4] - fam["exact"][4],
                       "gather_ms": fam[mode][5] - fam["exact"][5],
                       "max_abs_dlogit": float(d.max()), "mean_abs_dlogit": float(d.mean()), "logit_scale": scale,
                       "sign_flip_share": float(flips), "options": os.environ.get("R3G_OPTIONS", "")}
                if mode != "exact":       # the same error in space: both grids through marching cubes
                    out["mesh_distance"] = meshdist.grid_mesh_distance(grids["exact"], grids[mode], level, bound, a.R)
                if decoder == "dense":
                    for k in ("attention", "regroup", "select", "gather"):
                        out[k + "_per_pass_us"] = 1e3 * out[k + "_ms"] / passes
                    out["passes"] = passes
                else:
                    out["evaluated"] = stats[mode]["evaluated"]
                    out["evaluated_per_level"] = stats[mode]["evaluated_per_level"]
                print(json.dumps(out), flush=True)
    finally:
        m.set_kv_selection(0, 8192, 64)


if __name__ == "__main__":
    main()
