#!/usr/bin/env python3
"""Record the goldens of tests/test_cloud_gpu.py from the reference's own metrics module (host only, run once by hand):

    python tools/make_cloud_goldens.py REFERENCE_ROOT

REFERENCE_ROOT is a checkout of the reference project; its src/utils/metrics.py is loaded by path and RUN, nothing of its
text is copied.  It imports pytorch3d.ops.knn_points, which this image does not have: a stub module is put in sys.modules
whose knn_points is a brute force of our own (float64 distances, lowest index on a tie).

Writes tests/golden/cloud_pairs.npz (the clouds) and tests/golden/cloud_metrics.json (what the reference computes on them):
compute_fscore at tau 0.1 and at the median nearest-neighbour distance, compute_volume_iou in both modes, and icp.  The
clouds are regenerated with another seed until, in float64,
  * no nearest-neighbour distance lies within 1e-3 * tau of a tau (the reference's cdist takes the matmul route and is only
    that accurate), and
  * no scaled voxel coordinate (x - min) / voxel_size lies within 1e-4 of an integer, except the exact zeros of the points
    that attain the minimum (x - min is exactly 0 in any arithmetic),
so that the match counts and the voxel sets are exact and the scores depend on float32 rounding of one ratio only.
icp runs twice, on float32 and on float64 inputs; the largest element difference between the two results is recorded as
the reference's own rounding noise (the test allows four times that).

The icp pair.  The reference's compute_rigid_transform unpacks torch.svd(H) as U, S, Vt, but torch.svd returns V, so a step
applies V^T D U^T where Kabsch has V D U^T.  With correspondences right and the target R0 A + t, H = S R0^T for the source's
scatter S = Q L Q^T, U = Q and V = R0 Q, and the step is Q^T R0^T Q^T: the applied motion only when R0 = I and Q^2 = I.  So the
pair is one on which that solver is a registration at all: a cloud that is its own mirror image in all three coordinate planes
(its scatter is diagonal, Q = I) with three distinct axis variances, and a copy shifted by less than a quarter of its minimum
point spacing.  Asserted in float64: off-diagonal scatter below 1e-12 of the smallest diagonal entry, the diagonal entries
apart by a factor of 1.5, the shift below a quarter of the spacing, every nearest neighbour the point's own copy.  What the
solver does on a pair turned by 4 degrees is recorded beside it (icp_turned_pair: it ends far from the motion applied).
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VOXEL, GRID = 0.05, 64


def _knn_points(src, dst, K=1):
    assert K == 1
    d = torch.cdist(src.to(torch.float64), dst.to(torch.float64), compute_mode="donot_use_mm_for_euclid_dist")
    return types.SimpleNamespace(idx=d.argmin(dim=2, keepdim=True), dists=d.min(dim=2, keepdim=True).values ** 2)


def load_metrics(reference_root):
    p3d, ops = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.ops")
    ops.knn_points = _knn_points
    p3d.ops = ops
    sys.modules["pytorch3d"], sys.modules["pytorch3d.ops"] = p3d, ops
    spec = importlib.util.spec_from_file_location("reference_metrics", os.path.join(reference_root, "src", "utils", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def torus(n, r):
    """n points on a torus (radii 0.7 / 0.25), unevenly spread"""
    u, v = r.uniform(0, 2 * np.pi, n), r.uniform(0, 2 * np.pi, n) ** 1.1 % (2 * np.pi)
    return np.stack([(0.7 + 0.25 * np.cos(v)) * np.cos(u), (0.7 + 0.25 * np.cos(v)) * np.sin(u), 0.25 * np.sin(v)], 1)


def make_pair(seed):
    r = np.random.default_rng(seed)
    gt = torus(1500, r)
    pred = torus(2000, r) + r.normal(0, 0.02, (2000, 3))
    far = r.choice(2000, 300, replace=False)                   # a share of the prediction is off the surface
    pred[far] += r.normal(0, 0.15, (300, 3))
    pred = pred * 1.04 + np.array([0.03, -0.02, 0.01])
    return pred.astype(np.float32), gt.astype(np.float32)


def nn_dist(a, b):
    d = torch.cdist(torch.from_numpy(a).double(), torch.from_numpy(b).double(), compute_mode="donot_use_mm_for_euclid_dist")
    return d.min(1).values.numpy()


def conditions(pred, gt):
    """-> (ok, tau_med)"""
    d = np.concatenate([nn_dist(pred, gt), nn_dist(gt, pred)])
    tau_med = float(np.float32(np.median(d)))
    for tau in (0.1, tau_med, 0.01):
        if (np.abs(d - tau) < 1e-3 * tau).any():
            return False, tau_med
    lo = np.minimum(pred.min(0), gt.min(0)).astype(np.float64)
    for c in (pred, gt):
        s = (c.astype(np.float64) - lo) / VOXEL
        near = np.abs(s - np.round(s)) < 1e-4
        if (near & (s != 0.0)).any() or s.max() >= GRID:
            return False, tau_med
    return True, tau_med


ICP_SHIFT = np.array([0.011, -0.009, 0.006])


def make_symmetric_pair(seed, n=100, lo=0.08, ext=(1.0, 0.6, 0.3), gap=0.08):
    """dst: n points of the box [lo, ext], no two closer than `gap`, with their 8 mirror images, shuffled; src = dst - ICP_SHIFT"""
    r = np.random.default_rng(seed + 11)
    pts = []
    while len(pts) < n:
        c = r.uniform([lo] * 3, ext)
        if all(np.linalg.norm(c - p) >= gap for p in pts):
            pts.append(c)
    b = np.array(pts, np.float32)
    signs = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float32)
    dst = (b[None] * signs[:, None]).reshape(-1, 3)
    dst = np.ascontiguousarray(dst[r.permutation(len(dst))])
    src = (dst.astype(np.float64) - ICP_SHIFT).astype(np.float32)
    d = dst.astype(np.float64)
    s = (d - d.mean(0)).T @ (d - d.mean(0))
    diag = np.diag(s)
    assert np.abs(s - np.diag(diag)).max() < 1e-12 * diag.min() and diag[0] > 1.5 * diag[1] > 2.25 * diag[2]
    pair = np.linalg.norm(d[:, None] - d[None], axis=2) + np.eye(len(d))
    assert np.linalg.norm(ICP_SHIFT) < 0.25 * pair.min()
    assert (np.linalg.norm(src.astype(np.float64)[:, None] - d[None], axis=2).argmin(1) == np.arange(len(d))).all()
    return src, dst


def make_turned_pair(gt, seed):
    """dst = the gt cloud; src = 1200 of its points, lightly jittered, turned by 4 degrees and shifted -> (src, the motion
    src -> dst that was applied, as (R, t))"""
    r = np.random.default_rng(seed + 7)
    pick = r.choice(len(gt), 1200, replace=False)
    ax = np.array([0.3, -0.5, 0.81])
    ax /= np.linalg.norm(ax)
    ang = np.deg2rad(4.0)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    rot = np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)
    src = (gt[pick].astype(np.float64) + r.normal(0, 0.002, (1200, 3))) @ rot.T + np.array([0.02, -0.015, 0.01])
    return src.astype(np.float32), rot.T, -rot.T @ np.array([0.02, -0.015, 0.01])


def run_icp(m, src, dst):
    """the reference's icp on float32 and on float64 inputs -> (moved32, R32, t32, noise_Rt, noise_moved)"""
    ts, td = torch.from_numpy(src)[None], torch.from_numpy(dst)[None]
    mv32, r32, t32 = m.icp(ts, td)
    # the float64 run: the module builds its accumulators with torch.eye / torch.zeros, which follow the default dtype
    torch.set_default_dtype(torch.float64)
    mv64, r64, t64 = m.icp(ts.double(), td.double())
    torch.set_default_dtype(torch.float32)
    noise_rt = float(max((r32.double() - r64).abs().max(), (t32.double() - t64).abs().max()))
    return mv32[0].numpy(), r32[0].double().numpy(), t32[0, :, 0].double().numpy(), noise_rt, float((mv32.double() - mv64).abs().max())


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    m = load_metrics(sys.argv[1])
    torch.manual_seed(0)
    seed = 0
    while True:
        pred, gt = make_pair(seed)
        ok, tau_med = conditions(pred, gt)
        if ok:
            break
        seed += 1
    tp, tg = torch.from_numpy(pred)[None], torch.from_numpy(gt)[None]
    out = {"seed": seed, "voxel_size": VOXEL, "grid_size": GRID, "tau_med": tau_med,
           "fscore_tau_0.1": float(m.compute_fscore(tp, tg, tau=0.1)),
           "fscore_tau_med": float(m.compute_fscore(tp, tg, tau=tau_med)),
           "iou_pcd": float(m.compute_volume_iou(tp, tg, voxel_size=VOXEL, grid_size=GRID, mode="pcd")),
           "iou_bbox": float(m.compute_volume_iou(tp, tg, voxel_size=VOXEL, grid_size=GRID, mode="bbox"))}
    src, dst = make_symmetric_pair(seed)
    moved, r32, t32, noise_rt, noise_moved = run_icp(m, src, dst)
    out["icp"] = {"R": r32.tolist(), "t": t32.tolist(), "shift_applied": ICP_SHIFT.tolist(), "noise_Rt": noise_rt, "noise_moved": noise_moved}
    tsrc, r_true, t_true = make_turned_pair(gt, seed)
    _, rt, tt, noise_turned, _ = run_icp(m, tsrc, gt)
    out["icp_turned_pair"] = {"noise_Rt": noise_turned,
                              "distance_from_the_motion_applied": float(max(np.abs(rt - r_true).max(), np.abs(tt - t_true).max()))}
    np.savez(os.path.join(GOLDEN, "cloud_pairs.npz"), pred=pred, gt=gt, icp_src=src, icp_dst=dst, icp_moved=moved)
    with open(os.path.join(GOLDEN, "cloud_metrics.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
