#!/usr/bin/env python3
"""Times the mesh distance (include/r3g.h r3g_meshdist_build / r3g_meshdist_query) on the 257^3 sphere
of golden D (10000 - rho^2 at level 0.5, by the product's marching cubes) against a copy of itself shifted by --shift
voxels, both directions.  One JSON line:
  ms_build / ms_query   median and min over --reps, HIP events on the stream (build: one call with its read-backs; query: the
                        surface samples plus the vertices of one mesh against the grid of the other)
  tests_per_point       point-triangle tests per query point (counter "meshdist_tests")
  resolution, pairs     the grid the automatic rule settled on
  chamfer_l1, hausdorff of the pair, for orientation (a shift s along one axis: hausdorff <= s)

    python tools/bench_meshdist.py [--samples 200000] [--reps 5] [--shift 0.5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402


def timed(fn):
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    out = fn()
    e.record()
    e.synchronize()
    return b.elapsed_time(e), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shift", type=float, default=0.5)
    ap.add_argument("--resolution", type=int, default=0, help="0: automatic")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshdist.py needs an MI355X (the product has no CPU path)")
    from mc_volumes import golden_volume
    from r3g import ffi, mc, meshdist
    vol, level = golden_volume("D")
    v, f = mc.marching_cubes(torch.from_numpy(vol).cuda(), level)
    w = v + torch.tensor([a.shift, 0.0, 0.0], device=v.device)
    meshes = {"a": (v, f), "b": (w, f)}
    out = {"bench": "meshdist", "volume": "golden D 257^3", "verts": int(v.shape[0]), "faces": int(f.shape[0]), "shift": a.shift,
           "samples": a.samples, "reps": a.reps, "directions": {}}
    with ffi.device_lock(0):
        for src, dst in (("a", "b"), ("b", "a")):
            pts = torch.cat([meshdist.sample_surface(*meshes[src], a.samples)[0], meshes[src][0]])
            meshdist.build(*meshes[dst], a.resolution)                         # warm-up: workspaces, code objects
            meshdist.query(pts)
            torch.cuda.synchronize()
            ms_b, ms_q, tests = [], [], 0
            for _ in range(max(1, a.reps)):
                t, info = timed(lambda: meshdist.build(*meshes[dst], a.resolution))
                ms_b.append(t)
                n0 = ffi.counter("meshdist_tests")
                t, _ = timed(lambda: meshdist.query(pts))
                ms_q.append(t)
                tests = ffi.counter("meshdist_tests") - n0
            out["directions"][src + "->" + dst] = {
                "points": int(pts.shape[0]), "resolution": info["resolution"], "pairs": info["pairs"],
                "ms_build": {"median": statistics.median(ms_b), "min": min(ms_b)},
                "ms_query": {"median": statistics.median(ms_q), "min": min(ms_q)},
                "tests_per_point": tests / int(pts.shape[0]),
                "ns_per_point": 1e6 * statistics.median(ms_q) / int(pts.shape[0])}
    s = meshdist.compare(meshes["a"], meshes["b"], samples=a.samples, taus=(a.shift, 1.0))
    out.update({"chamfer_l1": s["chamfer_l1"], "hausdorff": s["hausdorff"], "within": s["ab"]["within"]})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
