#!/usr/bin/env python3
"""Times the plane fit on the GPU (include/r3g.h r3g_plane_ransac) on a floor made from the vertices of the
257^3 sphere of golden D (the product's marching cubes): scaled into [-1, 1]^3, y replaced by noise of sigma 0.01, resampled to
the size asked for, 20 % of the rows replaced by uniform outliers.  Reads nothing but the tree.  One JSON line; per size:
  ransac_ms             H = 2000 hypotheses at threshold 0.05: per pass (table, count, winner + mask, moments: HIP events inside the
                        call, r3g_plane_times), and the whole call with its read-back (events around it); median, min, max over --reps
  tests_per_s           point-plane tests (usable points x valid hypotheses) over the median of the count pass
  torch_loop_ms         the reference's loop restated in torch on the same GPU: per iteration one torch.randperm(n)[:3] on the host,
                        a [n,3] @ [3] pass and one .item(); the same 2000 iterations, --loop-reps runs
  same_winner_count     the restated loop and the product, fed the same triples, find the same best count
and for the yaw search: best_initial_yaw (two grid builds, 36 nearest-neighbour queries) beside 18 brute-force Chamfers by
torch.cdist on the same 8192 + 8192 points.

    python tools/bench_plane.py [--reps 9] [--loop-reps 2] [--sizes 200000 1000000]
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, THRESHOLD = 2000, 0.05


def timed(fn):
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    out = fn()
    e.record()
    e.synchronize()
    return b.elapsed_time(e), out


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def floor_cloud(verts, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lo, hi = verts.min(0).values, verts.max(0).values
    unit = (verts - (lo + hi) / 2) / ((hi - lo).max() / 2)
    p = unit[torch.randint(0, unit.shape[0], (n,), device="cuda", generator=g)].clone()
    p[:, [0, 2]] += 1e-3 * torch.randn((n, 2), device="cuda", generator=g)
    p[:, 1] = 0.01 * torch.randn((n,), device="cuda", generator=g)
    out = torch.rand((n,), device="cuda", generator=g) < 0.2
    p[out] = 2 * torch.rand((int(out.sum()), 3), device="cuda", generator=g) - 1
    return p.contiguous()


def torch_loop(points, triples, threshold):
    """the reference's fit_plane_ransac_refined loop, restated; `triples` None: its own sampler (a host randperm per iteration)"""
    best, best_mask = 0, None
    for i in range(H):
        idx = torch.randperm(len(points))[:3] if triples is None else triples[i]
        pts = points[idx]
        normal = torch.linalg.cross(pts[1] - pts[0], pts[2] - pts[0])
        if torch.norm(normal) < 1e-6:
            continue
        normal = normal / torch.norm(normal)
        mask = torch.abs((points - pts[0]) @ normal) < threshold
        count = mask.sum().item()
        if count > best:
            best, best_mask = count, mask
    return best, best_mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[200000, 1000000])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plane.py needs an MI355X (the product has no CPU path)")
    from mc_volumes import golden_volume
    from r3g import mc, plane
    vol, level = golden_volume("D")
    verts, _ = mc.marching_cubes(torch.from_numpy(vol).cuda(), level)
    out = {"tool": "bench_plane", "hypotheses": H, "threshold": THRESHOLD, "reps": a.reps, "loop_reps": a.loop_reps,
           "sphere_vertices": int(verts.shape[0]), "sizes": {}}
    for n in a.sizes:
        p = floor_cloud(verts, n, n)
        triples = plane.draw_triples(n, H, torch.Generator().manual_seed(1))
        dt = triples.to(device="cuda", dtype=torch.int32)
        for _ in range(3):                                  # warm-up: code objects, the workspace
            r = plane.ransac(p, dt, THRESHOLD)
        whole, passes = [], {k: [] for k in plane.PASSES}
        for _ in range(a.reps):
            ms, r = timed(lambda: plane.ransac(p, dt, THRESHOLD))
            whole.append(ms)
            for k, v in plane.times(0).items():
                passes[k].append(v)
        rep = r["report"]
        count_ms = statistics.median(passes["count"])
        row = {"points": n, "report": rep, "ransac_ms": {"whole": stat(whole), **{k: stat(v) for k, v in passes.items()}},
               "tests_per_s": rep["n_usable"] * rep["n_valid"] / (count_ms * 1e-3)}
        same, _ = torch_loop(p, triples, THRESHOLD)         # also the loop's warm-up
        row["same_winner_count"] = bool(same == rep["best_count"])
        row["loop_best_count"], row["product_best_count"] = int(same), rep["best_count"]
        loop = []
        for _ in range(a.loop_reps):
            torch.manual_seed(7)
            ms, _ = timed(lambda: torch_loop(p, None, THRESHOLD))
            loop.append(ms)
        row["torch_loop_ms"] = stat(loop)
        row["speedup_whole_call"] = statistics.median(loop) / statistics.median(whole)
        out["sizes"][str(n)] = row
    # the yaw search
    g = torch.Generator(device="cuda").manual_seed(3)
    unit = (verts - verts.mean(0)) / verts.std()
    v = (unit[torch.randint(0, unit.shape[0], (8192,), device="cuda", generator=g)] * torch.tensor([1.0, 0.4, 0.6], device="cuda")).contiguous()
    rs = plane.yaw_matrices(18, "cuda")
    t = (v[torch.randperm(8192, device="cuda", generator=g)] @ rs[7].T + 0.01 * torch.randn((8192, 3), device="cuda", generator=g)).contiguous()

    def brute():
        vc, tc = v - plane._centre(v, "bbox"), t - plane._centre(t, "bbox")
        losses = []
        for r in rs:
            d2 = torch.cdist(vc @ r.T, tc) ** 2
            losses.append(d2.min(dim=1).values.mean() + d2.min(dim=0).values.mean())
        losses = torch.stack(losses)
        return losses, int(torch.argmin(losses))

    for _ in range(2):
        ours, theirs = plane.best_initial_yaw(v, t), brute()
    yaw_ms, brute_ms = [], []
    for _ in range(a.reps):
        yaw_ms.append(timed(lambda: plane.best_initial_yaw(v, t))[0])
        brute_ms.append(timed(brute)[0])
    out["yaw"] = {"points": [8192, 8192], "best_initial_yaw_ms": stat(yaw_ms), "cdist_chamfer_ms": stat(brute_ms), "index": ours[2],
                  "cdist_index": theirs[1], "max_rel_loss_difference": float(((ours[1] - theirs[0]).abs() / theirs[0]).max())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
