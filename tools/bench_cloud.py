#!/usr/bin/env python3
"""Times the point-cloud neighbour search (include/r3g.h r3g_cloud_build / r3g_cloud_knn) on the vertices
of the 257^3 sphere of golden D (by the product's marching cubes) as targets and a jittered copy of them as queries.
One JSON line:
  auto                  at the automatic resolution: ms_build, and per k in 1, 8, 30 ms_query, ns_per_query, tests_per_query
                        (counter "cloud_tests"); median and min over --reps, HIP events on the stream
  per_cell              the same at the resolution the automatic rule would give for P = 1, 2, 4, 8, 16 points per cell (forced),
                        k = 1 and 30: what csrc/cloud_core.h's kPointsPerCell is chosen from.  P changes speed only, never results
  cdist                 the chunked torch.cdist + min of the reference's compute_fscore on the device, one direction (ms)
  ckdtree               scipy's cKDTree on the host, build and k = 1 query (ms, wall clock), when scipy is there

    python tools/bench_cloud.py [--reps 7] [--jitter 0.5] [--no-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms)}


def auto_resolution(n, per_cell):
    r = 1
    while r < 256 and (r + 1) ** 3 * per_cell <= n:
        r += 1
    return r


def measure(cloud, ffi, pts, qry, resolution, ks, reps):
    cloud.build(pts, resolution)                                   # warm-up: workspaces, code objects
    for k in ks:
        cloud.knn(qry, k)
    torch.cuda.synchronize()
    ms_b, out = [], {}
    for _ in range(reps):
        t, info = timed(lambda: cloud.build(pts, resolution))
        ms_b.append(t)
    out["resolution"], out["ms_build"] = info["resolution"], stat(ms_b)
    for k in ks:
        ms_q = []
        for _ in range(reps):
            n0 = ffi.counter("cloud_tests")
            t, _ = timed(lambda: cloud.knn(qry, k))
            ms_q.append(t)
            tests = ffi.counter("cloud_tests") - n0
        out["k%d" % k] = {"ms_query": stat(ms_q), "ns_per_query": 1e6 * statistics.median(ms_q) / int(qry.shape[0]),
                          "tests_per_query": tests / int(qry.shape[0])}
    return out


def cdist_min(q, p, chunk=2048):
    out = torch.empty(q.shape[0], device=q.device)
    for i in range(0, q.shape[0], chunk):
        out[i:i + chunk] = torch.cdist(q[i:i + chunk][None], p[None], p=2).min(dim=2).values[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--jitter", type=float, default=0.5, help="standard deviation of the queries' offset, voxels")
    ap.add_argument("--no-host", action="store_true", help="skip cKDTree")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud.py needs an MI355X (the product has no CPU path)")
    from mc_volumes import golden_volume
    from r3g import cloud, ffi, mc
    vol, level = golden_volume("D")
    pts, _ = mc.marching_cubes(torch.from_numpy(vol).cuda(), level)
    pts = pts.contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    qry = (pts + a.jitter * torch.randn(pts.shape, device="cuda", generator=g)).contiguous()
    n = int(pts.shape[0])
    reps = max(1, a.reps)
    out = {"bench": "cloud", "volume": "golden D 257^3", "points": n, "queries": int(qry.shape[0]), "jitter": a.jitter, "reps": reps}
    with ffi.device_lock(0):
        out["auto"] = measure(cloud, ffi, pts, qry, None, (1, 8, 30), reps)
        out["per_cell"] = {str(p): measure(cloud, ffi, pts, qry, auto_resolution(n, p), (1, 30), reps) for p in (1, 2, 4, 8, 16)}
        cloud.build(pts)
        d_grid = cloud.knn(qry, 1)[0][:, 0].sqrt()
    cdist_min(qry[:4096], pts)
    torch.cuda.synchronize()
    ms = []
    for _ in range(min(reps, 3)):
        t, d_cd = timed(lambda: cdist_min(qry, pts))
        ms.append(t)
    out["cdist"] = {"ms": stat(ms), "max_abs_difference_from_knn": float((d_cd - d_grid).abs().max())}
    if not a.no_host:
        try:
            from scipy.spatial import cKDTree
            p_h, q_h = pts.cpu().numpy(), qry.cpu().numpy()
            t0 = time.perf_counter()
            tree = cKDTree(p_h)
            t1 = time.perf_counter()
            tree.query(q_h, k=1)
            t2 = time.perf_counter()
            out["ckdtree"] = {"ms_build": 1e3 * (t1 - t0), "ms_query_k1": 1e3 * (t2 - t1), "threads": 1}
        except ImportError:
            out["ckdtree"] = None
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
