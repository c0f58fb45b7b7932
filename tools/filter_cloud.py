#!/usr/bin/env python3
"""Clean an object's point cloud on the GPU the way the reference's extract_pc_object.py does after its mask crop:

    python tools/filter_cloud.py IN.ply OUT.ply [--quantile Q] [--eps 0.035 --min-samples 10] [--no-dbscan] [--normals]

  1. --quantile Q     filter_points_by_quantile: keep the points inside the [Q, 1 - Q] quantiles of all three axes (off by
                      default, as upstream's filter_vggt_quantile is; upstream's quantile_value defaults to 0.05)
  2. DBSCAN           filter_dbscan: keep the largest cluster (r3g.cloud.dbscan, scikit-learn's labels; upstream's
                      dbscan_eps 0.035 and dbscan_min_points 10 are the defaults here); --no-dbscan skips it
  3. NaN              a cloud that still holds a NaN is refused (exit status 2), as upstream skips it
  4. --normals        estimate_normals(orient=True), written as the vertices of <OUT stem>_normals.ply the way upstream saves
                      them.  The orientation runs over each point's 30 nearest neighbours: r3g.cloud.orient_normals takes
                      k <= 31 where upstream passes 100 to Open3D.

Prints one JSON line: points in, after each step, and DBSCAN's report.
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
    ap.add_argument("dst")
    ap.add_argument("--quantile", type=float, default=None, help="trim this quantile from both ends of every axis first")
    ap.add_argument("--eps", type=float, default=0.035)
    ap.add_argument("--min-samples", type=int, default=10)
    ap.add_argument("--no-dbscan", action="store_true")
    ap.add_argument("--normals", action="store_true",
                    help="also write <stem>_normals.ply (orientation over k = 30 neighbours; upstream passes 100, ours takes k <= 31)")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filter_cloud.py needs a GPU (the product has no CPU path)")
    from r3g import cloud
    src = cloud.load_ply(a.src)
    pts = torch.from_numpy(src.vertices).to(torch.float32).cuda()
    out = {"tool": "filter_cloud", "points_in": int(pts.shape[0])}
    if a.quantile is not None:
        pts = cloud.filter_points_by_quantile(pts, a.quantile)
        out["after_quantile"] = int(pts.shape[0])
    if not a.no_dbscan and pts.shape[0]:
        labels, report = cloud.dbscan(pts, a.eps, a.min_samples)
        if report["n_clusters"]:
            pts = pts[labels == report["largest"]]
        out["dbscan"], out["after_dbscan"] = report, int(pts.shape[0])
    if bool(torch.isnan(pts).any()):
        print(json.dumps(dict(out, refused="NaN values")), flush=True)
        return 2
    cloud.save_ply(a.dst, pts.cpu().numpy())
    if a.normals:
        normals = cloud.estimate_normals(pts, orient=True)
        stem = a.dst[:-4] if a.dst.lower().endswith(".ply") else a.dst
        cloud.save_ply(stem + "_normals.ply", normals.cpu().numpy())
        out["normals"] = stem + "_normals.ply"
    out["points_out"] = int(pts.shape[0])
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
