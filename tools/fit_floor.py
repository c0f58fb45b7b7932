#!/usr/bin/env python3
"""Fit the floor plane of a point cloud on the GPU the way the reference's extract_and_fit_floor_plane chooses it:

    python tools/fit_floor.py IN.ply [--iterations 2000] [--threshold 0.05] [--seed 0]

r3g.plane.fit_floor: the PCA planarity test, the batched RANSAC fit and the total-least-squares fit, and upstream's rule among
them ("pca" below a planarity of 1e-3, "ransac" below an inlier ratio of 0.85, otherwise "svd").

Prints one JSON line: the method, the normal, the point on the plane, the inliers, both RMSEs, planarity and inlier ratio.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0, help="seed of the triple sampler")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fit_floor.py needs a GPU (the product has no CPU path)")
    from r3g import cloud, plane
    pts = torch.from_numpy(cloud.load_ply(a.src).vertices).to(torch.float32).cuda()
    fit = plane.fit_floor(pts, a.iterations, a.threshold, generator=torch.Generator().manual_seed(a.seed))
    print(json.dumps({"tool": "fit_floor", "points": int(pts.shape[0]), "method": fit["method"],
                      "normal": [float(v) for v in fit["normal"].cpu()], "point": [float(v) for v in fit["point"][0].cpu()],
                      "inliers": int(fit["mask"].sum()), "svd_rmse": fit["svd_rmse"], "ransac_rmse": fit["ransac_rmse"],
                      "planarity": fit["planarity"], "inlier_ratio": fit["inlier_ratio"]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
