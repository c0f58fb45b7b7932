#!/usr/bin/env python3
"""Micro-benchmark of the marching-cubes kernels on one grid (HIP events on the launch stream).

    python tools/bench_mc.py [--n 257] [--iters 20] [--algo mc|dmc|both]
Prints one JSON line per algorithm: per-phase times, algorithmic bytes (4*n^3 + 12 V + 12 F) and GB/s.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def field(n, seed=5):
    rng = np.random.default_rng(seed)
    lo = torch.from_numpy(rng.standard_normal((n // 8 + 1,) * 3).astype(np.float32))[None, None]
    return torch.nn.functional.interpolate(lo, size=(n, n, n), mode="trilinear", align_corners=True)[0, 0].contiguous()


def blob(n):
    """smooth closed surface (union of a few spheres), V ~ 2e5 at n = 257: the size of a typical object mesh"""
    ax = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    f = torch.full((n, n, n), -1.0)
    for cx, cy, cz, r in ((0, 0, 0, .55), (.35, .2, .1, .35), (-.3, -.25, .2, .3), (.1, -.4, -.3, .28)):
        f = torch.maximum(f, r - torch.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2))
    return f.contiguous()


def dot(n):
    """almost empty grid: one small sphere -> the classify pass is a pure stream"""
    ax = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (0.06 - torch.sqrt(X ** 2 + Y ** 2 + Z ** 2)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", default="blob", choices=["blob", "noise", "dot"])
    ap.add_argument("--n", type=int, default=257)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--algo", default="mc", choices=["mc", "dmc", "both"],
                    help="mc: Lewiner marching cubes; dmc: dual marching cubes; both: the two alternating call by call "
                         "in one run (one JSON line each)")
    a = ap.parse_args()
    import ctypes
    from r3g import dmc, ffi, mc
    extract = {"mc": mc.extract_mesh, "dmc": dmc.extract_mesh}
    algos = ["mc", "dmc"] if a.algo == "both" else [a.algo]
    g = {"blob": blob, "noise": field, "dot": dot}[a.field](a.n).cuda()
    for _ in range(3):
        for k in algos:
            v, f = extract[k](g)
    torch.cuda.synchronize()
    # whole calls (count + read-back + allocation + emit), HIP events on the stream, the algorithms alternating
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)] for k in algos}
    size = {}
    for i in range(a.iters):
        for k in algos:
            ev[k][i][0].record()
            v, f = extract[k](g)
            ev[k][i][1].record()
            size[k] = (v.shape[0], f.shape[0])
    torch.cuda.synchronize()
    L = ffi.lib()
    for k in algos:
        ms = sorted(b.elapsed_time(e) for b, e in ev[k])
        med = ms[len(ms) // 2]
        V, F = size[k]
        bytes_alg = 4 * a.n ** 3 + 12 * V + 12 * F
        # the kernels alone (HIP events around each launch on its stream: r3g_prof_*): classify = family 6, the rest = 7
        ffi.check(L.r3g_prof_enable(1))
        for _ in range(a.iters):
            extract[k](g)
        torch.cuda.synchronize()
        cnt, pms, work = (ctypes.c_int64 * 9)(), (ctypes.c_double * 9)(), (ctypes.c_double * 9)()
        ffi.check(L.r3g_prof_read(cnt, pms, work, 9))
        ffi.check(L.r3g_prof_enable(0))
        cls_us = 1e3 * pms[6] / max(1, cnt[6])
        other_us = 1e3 * pms[7] / max(1, a.iters)
        kern_ms = (cls_us + other_us) * 1e-3
        print(json.dumps({"algo": k, "field": a.field, "n": a.n, "V": V, "F": F, "ms_median": med, "ms_min": ms[0],
                          "alg_bytes": bytes_alg, "GBps_median": bytes_alg / med / 1e6, "frac_of_8TBps": bytes_alg / med / 1e6 / 8000,
                          "classify_us": cls_us, "scan_vertices_faces_us": other_us,
                          "classify_GBps": 4 * a.n ** 3 / cls_us / 1e3, "kernels_GBps": bytes_alg / kern_ms / 1e6,
                          "kernels_frac_of_8TBps": bytes_alg / kern_ms / 1e6 / 8000,
                          "options": os.environ.get("R3G_OPTIONS", "")}))


if __name__ == "__main__":
    main()
