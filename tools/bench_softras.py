#!/usr/bin/env python3
"""Times the soft silhouette on the GPU (include/r3g.h r3g_softras_forward / _backward) on a 40 000-face
mesh (the reference's FaceReducer cap): a lat-long sphere with a radial ripple, seen by a pinhole camera so that it fills most of
the image.  Reads nothing but the tree.  One JSON line; per case (image 512^2 and 1024^2, K = 20, the reference's sigma = 5e-7 in
NDC units and one 100 times larger, blur radius = ln(1 / 1e-4 - 1) sigma):
  ms                    per pass (bin with its read-back, forward, backward, gather: HIP events inside the calls,
                        r3g_softras_times); median, min, max over --reps calls after one warm-up
  pairs_per_tile        (face, 8 x 8 tile) pairs of the bin pass over the tiles: mean; and the share of tiles with any
  found                 (pixel, face) fragments the backward found in the stored lists

    python tools/bench_softras.py [--reps 9] [--sizes 512 1024] [--faces 40000]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def sphere(n_faces):
    """lat-long sphere of about n_faces triangles with a ripple -> verts float32 [V, 3], faces int32 [F, 3]"""
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


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--faces", type=int, default=40000)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_softras.py needs a GPU (the product has no CPU path)")
    from r3g import softras
    v, f = sphere(a.faces)
    verts, faces = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    csr = softras.corner_csr(faces, verts.shape[0])
    cases = []
    for size in a.sizes:
        R, t = torch.eye(3, device="cuda"), torch.tensor([0.0, 0.0, 3.0], device="cuda")
        pos = softras.pinhole(verts, R, t, 1.2 * size, 1.2 * size, size / 2, size / 2).contiguous()
        for mult in (1, 100):
            sigma = softras.sigma_to_pixels(5e-7 * mult, size, size)
            blur = softras.default_blur_radius(sigma)
            ga = torch.ones(size, size, device="cuda")
            ms = {p: [] for p in softras.PASSES}
            rep = brep = None
            for it in range(a.reps + 1):
                alpha, face, dist, zbuf, rep = softras.forward_raw(pos, faces, (size, size), 20, sigma, blur)
                _, gp, brep = softras.backward_raw(pos, faces, (size, size), 20, sigma, blur, face, dist, ga, csr)
                if it:
                    for p, x in softras.times().items():
                        ms[p].append(x)
            cases.append({"size": size, "faces": int(faces.shape[0]), "verts": int(verts.shape[0]), "K": 20, "sigma_ndc": 5e-7 * mult,
                          "sigma_px2": sigma, "blur_radius_px2": blur, "ms": {p: stat(x) for p, x in ms.items()},
                          "pairs": rep["pairs"], "tiles": rep["tiles"], "pairs_per_tile": rep["pairs"] / rep["tiles"],
                          "faces_used": rep["used"], "faces_skipped": rep["skipped"], "found": brep["found"],
                          "covered": float((alpha > 0.5).float().mean()), "grad_max": float(gp.abs().max())})
    print(json.dumps({"tool": "bench_softras", "device": torch.cuda.get_device_name(0), "reps": a.reps, "cases": cases}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
