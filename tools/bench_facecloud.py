#!/usr/bin/env python3
"""Times the face-to-cloud distance on the GPU (include/r3g.h r3g_cloud_faces / _backward): a 40 000-face
sphere (the reference's FaceReducer cap) against clouds of 10^4 and 10^5 points sampled on the half of the same sphere that one
depth view would see, with noise.  Reads nothing but the tree.  One JSON line; per cloud size:
  ms                 per pass (classify, narrow, wide, gather: HIP events inside the calls, r3g_cloud_faces_times) and of the
                     whole forward as the caller sees it; median, min, max over --reps calls after one warm-up
  tests_per_face     point-triangle tests of the walk over the usable faces
  wide_share         the share of faces walked by a wave, and the largest ring walked
  brute_ms           a chunked brute force in torch on the same GPU: the nearest point of every face's CENTROID (point-point, which
                     is less work than point-triangle), median over --reps
and, for the larger cloud, the same mesh with one floor-sized quad (two triangles, four times the cloud's extent) added: the forward
with the wide path, and -- when --no-wide-library names a build of the library with -DR3G_FC_NO_WIDE -- the forward of that build,
run in a child process.  `--build-no-wide` makes that build next to the product's library first (hipcc; it needs the objects of
3d-re-gen_amd/build.py).

    python tools/bench_facecloud.py [--reps 9] [--faces 40000] [--points 10000 100000] [--build-no-wide] [--no-wide-library PATH]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3d-re-gen_amd")
sys.path.insert(0, PKG)
NO_WIDE = os.path.join(PKG, "libr3g_nowide.so")


def sphere(n_faces):
    """lat-long sphere of about n_faces triangles with a ripple -> verts float32 [V, 3], faces int32 [F, 3]"""
    import numpy as np
    rows = max(3, int(round(math.sqrt(n_faces / 4.0))))
    cols = max(3, n_faces // (2 * rows))
    th = np.linspace(0.02, math.pi - 0.02, rows + 1)[:, None]
    ph = np.linspace(0, 2 * math.pi, cols, endpoint=False)[None, :]
    r = 1.0 + 0.08 * np.sin(5 * th) * np.cos(7 * ph)
    v = np.stack([r * np.sin(th) * np.cos(ph), r * np.cos(th) * np.ones_like(ph), r * np.sin(th) * np.sin(ph)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    a, b = i * cols + j, i * cols + (j + 1) % cols
    f = np.concatenate([np.stack([a, b, a + cols], -1).reshape(-1, 3), np.stack([b, b + cols, a + cols], -1).reshape(-1, 3)])
    return v.astype(np.float32), f.astype(np.int32)


def view_cloud(v, f, n, seed=0):
    """n points on the faces of the half z > 0 (what one depth view sees), with 0.2 % noise"""
    import numpy as np
    rng = np.random.default_rng(seed)
    tri = v[f]
    tri = tri[tri[:, :, 2].mean(1) > 0]
    pick = rng.integers(0, len(tri), n)
    w = rng.dirichlet(np.ones(3), n)
    return ((tri[pick] * w[:, :, None]).sum(1) + rng.normal(0, 0.002, (n, 3))).astype(np.float32)


def with_floor(v, f):
    """the mesh with one quad of four times its extent under it"""
    import numpy as np
    y = float(v[:, 1].min()) - 0.01
    q = np.array([[-4, y, -4], [4, y, -4], [4, y, 4], [-4, y, 4]], np.float32)
    n = len(v)
    return np.concatenate([v, q]), np.concatenate([f, np.array([[n, n + 1, n + 2], [n, n + 2, n + 3]], np.int32)])


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def time_forward(verts, faces, reps, backward=True):
    import torch
    from r3g import cloud, softras
    csr = softras.corner_csr(faces, verts.shape[0])
    g = torch.ones(faces.shape[0], device="cuda")
    ms = {p: [] for p in cloud.FACES_PASSES}
    wall, info = [], None
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d2, idx, w, diff, info = cloud.face_nearest(verts, faces)      # (synchronises: the report)
        t1 = time.perf_counter()
        if backward:
            cloud.face_nearest_backward(g, idx, w, diff, csr, verts.shape[0])
        if it:
            wall.append(1e3 * (t1 - t0))
            for p, x in cloud.faces_times(0).items():
                ms[p].append(x)
    return {"ms": {p: stat(x) for p, x in ms.items()}, "forward_wall_ms": stat(wall), "tests_per_face": info["tests"] / max(info["usable"], 1),
            "wide_share": info["wide"] / max(info["usable"], 1), "wide": info["wide"], "max_ring": info["max_ring"], "faces": int(faces.shape[0])}


def brute(verts, faces, points, reps, chunk=2048):
    import torch
    cen = verts[faces.long()].mean(1)
    ms = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best = torch.empty(cen.shape[0], device="cuda")
        for s in range(0, cen.shape[0], chunk):
            best[s:s + chunk] = torch.cdist(cen[s:s + chunk], points).min(1).values
        torch.cuda.synchronize()
        if it:
            ms.append(1e3 * (time.perf_counter() - t0))
    return stat(ms)


def floor_case(n_faces, n_points, reps):
    import torch
    from r3g import cloud
    v, f = sphere(n_faces)
    cloud.build(torch.from_numpy(view_cloud(v, f, n_points)).cuda())
    fv, ff = with_floor(v, f)
    return time_forward(torch.from_numpy(fv).cuda(), torch.from_numpy(ff).cuda(), reps, backward=False)


def build_no_wide():
    """the product's objects with facecloud_kernels.hip compiled -DR3G_FC_NO_WIDE -> NO_WIDE"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("r3g_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build(verbose=False)
    obj = os.path.join(b.OBJ, "facecloud_kernels_nowide.o")
    subprocess.check_call(["hipcc"] + b.COMMON + b.PER_FILE["facecloud_kernels.hip"] + ["-DR3G_FC_NO_WIDE", "-c", os.path.join(b.CSRC, "facecloud_kernels.hip"),
                           "-o", obj])
    objs = [os.path.join(b.OBJ, os.path.splitext(s)[0] + ".o") for s in b.sources() if s != "facecloud_kernels.hip"] + [obj]
    subprocess.check_call(["hipcc", "--offload-arch=" + b.ARCH, "-shared", "-fPIC", "-o", NO_WIDE] + objs)
    return NO_WIDE


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--faces", type=int, default=40000)
    ap.add_argument("--points", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--build-no-wide", action="store_true", help="build %s and stop (needs no GPU)" % os.path.relpath(NO_WIDE, ROOT))
    ap.add_argument("--no-wide-library", default=None, help="a build with -DR3G_FC_NO_WIDE, for the floor case")
    ap.add_argument("--floor-only", type=int, default=0, help=argparse.SUPPRESS)      # the child's mode: the floor case at this many points
    a = ap.parse_args(argv)
    if a.build_no_wide:
        print(build_no_wide())
        return 0
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_facecloud.py needs a GPU (the product has no CPU path)")
    if a.floor_only:
        print(json.dumps(floor_case(a.faces, a.floor_only, a.reps)), flush=True)
        return 0
    from r3g import cloud
    v, f = sphere(a.faces)
    verts, faces = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    cases = []
    for n in a.points:
        pts = torch.from_numpy(view_cloud(v, f, n)).cuda()
        info = cloud.build(pts)
        case = dict(time_forward(verts, faces, a.reps), points=n, resolution=info["resolution"], brute_ms=brute(verts, faces, pts, a.reps))
        cases.append(case)
    n = max(a.points)
    floor = {"points": n, "wide_path": floor_case(a.faces, n, a.reps), "no_wide_path": None}
    if a.no_wide_library:
        env = dict(os.environ, R3G_LIBRARY=os.path.abspath(a.no_wide_library))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--floor-only", str(n), "--faces", str(a.faces), "--reps", str(a.reps)],
                             env=env, capture_output=True, text=True, check=True, timeout=600)
        floor["no_wide_path"] = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps({"tool": "bench_facecloud", "device": torch.cuda.get_device_name(0), "reps": a.reps, "cases": cases, "floor": floor}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
