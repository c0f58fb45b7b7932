#!/usr/bin/env python3
"""Times the point-cloud meshing (include/r3g.h r3g_cloud_orient, r3g_recon_splat / _solve / _sample) on the
vertices of the 257^3 sphere of golden D (by the product's marching cubes) with their exact normals, each reversed by a coin
for the orientation.  One JSON line:
  orient                k = 30: ms per call; ms_knn, the cloud build and the 31-list the call makes inside, timed on their own;
                        ms_rounds, the difference (Boruvka rounds and the final passes); rounds; frustrated; all_outward
  depth6, depth7, depth8   ms per splat / solve (10 cycles) / sample (the level) / mc (count + emit) / density sample at the
                        vertices; vertices, faces, level; residual: the max-norm residual relative to max |b| after 1 .. 10
                        cycles (each a solve of its own from zero)
median and min over --reps, HIP events on the stream.

    python tools/bench_recon.py [--reps 5] [--depths 6,7,8]
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


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms)}


def repeat(fn, reps):
    fn()                                                            # warm-up: workspaces, code objects
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t, out = timed(fn)
        ms.append(t)
    return stat(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depths", default="6,7,8")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recon.py needs an MI355X (the product has no CPU path)")
    from mc_volumes import golden_volume
    from r3g import cloud, ffi, mc, recon
    vol, level = golden_volume("D")
    pts, _ = mc.marching_cubes(torch.from_numpy(vol).cuda(), level)
    pts = pts.contiguous()
    centre = 0.5 * (pts.amin(0) + pts.amax(0))
    nrm = pts - centre
    nrm = (nrm / nrm.norm(dim=1, keepdim=True)).contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    coin = torch.where(torch.rand(pts.shape[0], device="cuda", generator=g) < 0.5, -1.0, 1.0)
    flipped = (nrm * coin[:, None]).contiguous()
    reps = max(1, a.reps)
    out = {"bench": "recon", "volume": "golden D 257^3", "points": int(pts.shape[0]), "reps": reps}
    with ffi.device_lock(0):
        k = 30
        ms_all, (oriented, info) = repeat(lambda: cloud.orient_normals(pts, flipped, k), reps)

        def knn_only():
            cloud.build(pts)
            return cloud.knn(pts, k + 1)
        ms_knn, _ = repeat(knn_only, reps)
        out["orient"] = {"k": k, "ms": ms_all, "ms_knn": ms_knn, "ms_rounds": {s: ms_all[s] - ms_knn[s] for s in ms_all},
                         "rounds": int(info["rounds"]), "trees": int(info["trees"]), "frustrated": int(info["frustrated"]),
                         "all_outward": bool(((oriented * nrm).sum(1) > 0).all())}
        for depth in [int(d) for d in a.depths.split(",")]:
            c, side, h = recon.box(pts, nrm, depth)
            row = {"n": 2 ** depth + 1, "h": h}
            row["ms_splat"], _ = repeat(lambda: recon.splat(pts, nrm, depth, c, side), reps)
            row["ms_solve"], chi = repeat(lambda: recon.solve(depth, pts.device, 10), reps)
            row["ms_sample_level"], (_, total, count) = repeat(lambda: recon.sample(1, pts, nrm), reps)
            lv = recon.level_from_sum(total, count)
            xf = recon.lattice_xform(depth, c, side)
            row["ms_mc"], (v, f) = repeat(lambda: mc._run(chi, lv, False, xf, recon.REVERSE_FACES["mc"]), reps)
            row["ms_sample_density"], _ = repeat(lambda: recon.sample(0, v), reps)
            row.update(level=lv, vertices=int(v.shape[0]), faces=int(f.shape[0]))
            res = []
            for cycles in range(1, 11):
                x, b = recon.solve(depth, pts.device, cycles, want_b=True)
                res.append(recon.residual_ratio(x, b, h))
                del x, b
            row["residual"] = res
            out["depth%d" % depth] = row
            del chi, v, f
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
