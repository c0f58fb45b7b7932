#!/usr/bin/env python3
"""Times the mesh registration (include/r3g.h r3g_meshfit_step / r3g_meshfit) on the 257^3 sphere of
golden D (10000 - rho^2 at level 0.5, by the product's marching cubes: the mesh tools/bench_meshdist.py uses) as target and
--samples area-weighted surface samples of it, moved by a small pose, as source.  One JSON line:
  ms_step_plane / ms_step_point   one fused step (move, walk, closest point, float64 sums, reduction, read-back): median and
                                  min over --reps, HIP events on the stream
  ms_query                        (a) r3g_meshdist_query alone on the same points: the walk, which should dominate a step
  ms_torch_sums                   (b) the same point-mode sums from r3g_meshdist_query plus torch operations (gather the faces,
                                  closest point by barycentric projection, reductions, one read-back): what a step cost
                                  before it was fused
  tests_per_point                 point-triangle tests per point of one step (counter "meshdist_tests")
  fit                             a full point-to-plane fit from the pose: ms, updates, rms, where the centre lands

    python tools/bench_meshfit.py [--samples 200000] [--reps 5]
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


def timed(fn):
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    out = fn()
    e.record()
    e.synchronize()
    return b.elapsed_time(e), out


def torch_sums(meshdist, pts, w, verts, faces):
    """the point-mode sums the unfused way: query, then torch (closest point = projection onto the winning face's plane clamped
    to the face by its barycentrics; enough for a timing, not the product's tri_closest)"""
    d2, face = meshdist.query(pts)
    t = verts[faces.long()[face.long()]].double()
    p = pts.double()
    a, ab, ac = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    ap = p - a
    g11, g12, g22 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
    e1, e2 = (ab * ap).sum(1), (ac * ap).sum(1)
    det = (g11 * g22 - g12 * g12).clamp_min(1e-300)
    v = ((g22 * e1 - g12 * e2) / det).clamp(0, 1)
    u = ((g11 * e2 - g12 * e1) / det).clamp(0, 1)
    q = a + v[:, None] * ab + u[:, None] * ac
    wd = w.double()
    sums = torch.cat([wd.sum().reshape(1), (wd[:, None] * p).sum(0), (wd[:, None] * q).sum(0),
                      (wd[:, None, None] * p[:, :, None] * q[:, None, :]).sum(0).reshape(-1),
                      (wd * (p * p).sum(1)).sum().reshape(1), (wd * d2.double()).sum().reshape(1)])
    return sums.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshfit.py needs an MI355X (the product has no CPU path)")
    import importlib.util
    spec = importlib.util.spec_from_file_location("r3g_build", os.path.join(ROOT, "3d-re-gen_amd", "build.py"))
    r3g_build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(r3g_build)
    import meshfit_ref as ref
    from mc_volumes import golden_volume
    from r3g import ffi, mc, meshdist, meshfit
    vol, level = golden_volume("D")
    v, f = mc.marching_cubes(torch.from_numpy(vol).cuda(), level)
    pts, _, w = meshdist.sample_surface(v, f, a.samples)
    w = w.float()
    centre = v.double().mean(0).cpu().numpy()
    pose = ref.pose(3.0, shift=(0.7, -0.4, 0.3))                                  # about the sphere's centre: 3 degrees, < 1 voxel
    pose[:3, 3] += centre - pose[:3, :3] @ centre
    src = meshfit.transform_points(np.linalg.inv(pose), pts)
    out = {"bench": "meshfit", "volume": "golden D 257^3", "verts": int(v.shape[0]), "faces": int(f.shape[0]),
           "points": int(src.shape[0]), "reps": a.reps, "library_digest": r3g_build.built_digest()}
    reps = max(1, a.reps)
    with ffi.device_lock(0):
        info = meshdist.build(v, f)
        out.update({"resolution": info["resolution"], "pairs": info["pairs"]})
        for fn in (lambda: meshfit.step(src, weights=w, method="plane"), lambda: meshfit.step(src, weights=w, method="point"),
                   lambda: meshdist.query(src), lambda: torch_sums(meshdist, src, w, v, f)):          # warm-up
            fn()
        torch.cuda.synchronize()
        n0 = ffi.counter("meshdist_tests")
        meshfit.step(src, weights=w, method="plane")
        out["tests_per_point"] = (ffi.counter("meshdist_tests") - n0) / int(src.shape[0])
        for key, fn in (("ms_step_plane", lambda: meshfit.step(src, weights=w, method="plane")),
                        ("ms_step_point", lambda: meshfit.step(src, weights=w, method="point")),
                        ("ms_query", lambda: meshdist.query(src)),
                        ("ms_torch_sums", lambda: torch_sums(meshdist, src, w, v, f))):
            ms = [timed(fn)[0] for _ in range(reps)]
            out[key] = {"median": statistics.median(ms), "min": min(ms)}
        ms, (matrix, fit) = timed(lambda: meshfit.fit(src, w, method="plane"))
        # a sphere does not constrain the rotation: where its centre lands is what the fit can find
        err = (ref.pose_error(matrix, pose)[0], float(np.linalg.norm(ref.apply(matrix, centre) - ref.apply(pose, centre))))
        out["fit"] = {"ms": ms, "updates": fit["iterations"], "converged": fit["converged"], "rms": fit["rms"],
                      "ms_per_accumulation": ms / (fit["iterations"] + 1), "centre_error": err[1], "rotation_error_deg": err[0]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
