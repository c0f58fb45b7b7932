#!/usr/bin/env python3
"""Times DBSCAN on the GPU (include/r3g.h r3g_cloud_dbscan) on the vertices of the 257^3 sphere of golden D
(by the product's marching cubes) plus 5 % uniform noise in their box, min_samples 10, at eps = 1, 2 and 4 times the median
nearest-neighbour distance of the cloud.  One JSON line; per eps:
  ms                    per pass (grid build, count, link, border, number: HIP events inside the call, r3g_cloud_dbscan_times),
                        their sum, and the whole call with its read-back (events around it); median, min and max over --reps
  tests_per_point       evaluations of the neighbour predicate per usable point, all three walks (counter "dbscan_tests")
  report                what the call reports (clusters, core, border, noise, largest)
  sklearn               scikit-learn's DBSCAN on the same cloud on the host, when it imports: ms of fit alone, ms of the
                        reference's path (device -> host copy, fit, largest-cluster mask, mask -> device; wall clock around
                        both copies), and whether its labels equal ours

    python tools/bench_dbscan.py [--reps 7] [--no-host] [--multiples 1 2 4]
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
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn):
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    out = fn()
    e.record()
    e.synchronize()
    return b.elapsed_time(e), out


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-samples", type=int, default=10)
    ap.add_argument("--multiples", type=float, nargs="+", default=[1.0, 2.0, 4.0])
    ap.add_argument("--no-host", action="store_true", help="skip scikit-learn")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dbscan.py needs an MI355X (the product has no CPU path)")
    from mc_volumes import golden_volume
    from r3g import cloud, ffi, mc
    vol, level = golden_volume("D")
    verts, _ = mc.marching_cubes(torch.from_numpy(vol).cuda(), level)
    g = torch.Generator(device="cuda").manual_seed(0)
    lo, hi = verts.min(0).values, verts.max(0).values
    noise = lo + (hi - lo) * torch.rand((verts.shape[0] // 20, 3), device="cuda", generator=g)
    pts = torch.cat([verts, noise])[torch.randperm(verts.shape[0] + noise.shape[0], device="cuda", generator=g)].contiguous()
    n = int(pts.shape[0])
    reps = max(1, a.reps)
    with ffi.device_lock(0):
        cloud.build(pts)
        nn = float(cloud.knn(pts, 2)[0][:, 1].sqrt().median())
    out = {"bench": "dbscan", "volume": "golden D 257^3 + 5% noise", "points": n, "min_samples": a.min_samples, "median_nn": nn,
           "reps": reps, "eps": {}}
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    for mult in a.multiples:
        eps = mult * nn
        with ffi.device_lock(0):
            cloud.dbscan(pts, eps, a.min_samples)                      # warm-up: workspaces, code objects
            torch.cuda.synchronize()
            passes = {k: [] for k in cloud.DBSCAN_PASSES}
            whole = []
            for _ in range(reps):
                t0 = ffi.counter("dbscan_tests")
                t, (labels, report) = timed(lambda: cloud.dbscan(pts, eps, a.min_samples))
                tests = ffi.counter("dbscan_tests") - t0
                whole.append(t)
                for k, v in cloud.dbscan_times(0).items():
                    passes[k].append(v)
        row = {"eps": eps, "ms": {k: stat(v) for k, v in passes.items()}, "report": report,
               "tests_per_point": tests / max(1, report["n_usable"])}
        row["ms"]["passes_total"] = stat([sum(passes[k][i] for k in passes) for i in range(reps)])
        row["ms"]["call"] = stat(whole)
        if DBSCAN is not None and not a.no_host:
            fit, path = [], []
            for _ in range(min(reps, 3)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = pts.cpu().numpy()
                t1 = time.perf_counter()
                db = DBSCAN(eps=eps, min_samples=a.min_samples).fit(host)
                t2 = time.perf_counter()
                lab = db.labels_
                uniq, cnt = np.unique(lab[lab != -1], return_counts=True)
                kept = pts[torch.from_numpy(lab == uniq[cnt.argmax()]).to(pts.device)] if len(cnt) else pts
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                fit.append(1e3 * (t2 - t1))
                path.append(1e3 * (t3 - t0))
            row["sklearn"] = {"ms_fit": stat(fit), "ms_reference_path": stat(path), "labels_equal": bool(np.array_equal(lab, labels.cpu().numpy())),
                              "kept": int(kept.shape[0]), "threads": 1}
        out["eps"]["%gx" % mult] = row
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
