"""Mesh registration on the GPU: iterative closest point of a point set or mesh onto a mesh (include/r3g.h "mesh
registration").

`align` finds the rigid (optionally similarity) transform that takes a source onto a target mesh; `compare_aligned` aligns
first and then scores with r3g.meshdist.compare, which is what an evaluation of a generated mesh against a ground truth in
another frame needs.  One iteration is one fused kernel launch (move, nearest triangle, closest point, float64 sums in a
fixed order) and one small read-back; the 6 x 6 / 7 x 7 solve runs on the host (csrc/meshfit_core.h).

method "plane" (default): point-to-plane, one Gauss-Newton step per iteration; converges in a handful of iterations where the
point method slides along the surface for hundreds.  method "point": Horn / Umeyama closed form on the closest points (the
reference's compute_rigid_transform inside its icp).  ICP is local: from a start more than a few tens of degrees off it ends
in a wrong minimum; `inits` (e.g. `cube_inits`) tries several starts coarsely and refines the best.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

from . import ffi, meshdist

METHODS = {"point": 0, "plane": 1}
SUMS = 37


def _points_arg(points):
    if not (torch.is_tensor(points) and points.is_cuda):
        raise ValueError("source points must live on the GPU (there is no CPU path)")
    p = points.detach().to(torch.float32).contiguous()
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("expected points [N,3]")
    return p


def _weights_arg(weights, p):
    if weights is None:
        return None
    w = weights.detach().to(p.device, torch.float32).contiguous().reshape(-1)
    if w.shape[0] != p.shape[0]:
        raise ValueError("expected one weight per point")
    return w


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _max_dist(max_dist):
    return float("inf") if max_dist is None else float(max_dist)


def step(points, xform=None, weights=None, method="plane", max_dist=None):
    """r3g_meshfit_step against the last r3g.meshdist.build on the points' device: one accumulation, no solve.
    xform = 13 floats (s, R row-major, t; None: identity).  -> (sums float64 numpy [18 | 37], used); the layout of the sums
    is in include/r3g.h."""
    if method not in METHODS:
        raise ValueError("method must be 'plane' or 'point'")
    p = _points_arg(points)
    w = _weights_arg(weights, p)
    x = np.ascontiguousarray([1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] if xform is None else xform, np.float64).reshape(-1)
    if x.shape != (13,):
        raise ValueError("xform: expected 13 values (s, R row-major, t)")
    dev = p.device.index or 0
    sums, used = np.zeros(SUMS), ctypes.c_int64(0)
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_meshfit_step(ffi.context(dev), _ptr(p), p.shape[0], _ptr(w), x.ctypes.data, METHODS[method],
                                             _max_dist(max_dist), sums.ctypes.data, ctypes.byref(used),
                                             ffi.stream_ptr()))
    return sums[:18 if method == "point" else 37], used.value


def fit(points, weights=None, init=None, method="plane", with_scale=False, max_iterations=30, tolerance=1e-7, max_dist=None):
    """r3g_meshfit against the last r3g.meshdist.build on the points' device -> (matrix float64 numpy [4,4], info dict:
    iterations, converged, rms, used, scale)"""
    if method not in METHODS:
        raise ValueError("method must be 'plane' or 'point'")
    p = _points_arg(points)
    w = _weights_arg(weights, p)
    m0 = None
    if init is not None:
        m0 = np.ascontiguousarray(init, np.float64)
        if m0.shape != (4, 4):
            raise ValueError("init: expected a 4 x 4 matrix")
    dev = p.device.index or 0
    m, info = np.zeros(16), np.zeros(5)
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_meshfit(ffi.context(dev), _ptr(p), p.shape[0], _ptr(w), None if m0 is None else m0.ctypes.data,
                                        METHODS[method], int(bool(with_scale)), int(max_iterations), float(tolerance),
                                        _max_dist(max_dist), m.ctypes.data, info.ctypes.data, ffi.stream_ptr()))
    return m.reshape(4, 4), {"iterations": int(info[0]), "converged": bool(info[1]), "rms": float(info[2]), "used": int(info[3]),
                             "scale": float(info[4])}


def cube_rotations():
    """the 24 proper signed axis permutations (the rotation group of the cube) -> float64 numpy [24,3,3], identity first"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            r = np.zeros((3, 3))
            for i in range(3):
                r[i, perm[i]] = signs[i]
            if np.linalg.det(r) > 0:
                out.append(r)
    return np.stack(out)


def _centroid(points, weights):
    p = points.detach().to(torch.float64)
    if weights is None:
        return p.mean(0).cpu().numpy()
    w = weights.detach().to(p.device, torch.float64).reshape(-1, 1)
    return ((p * w).sum(0) / w.sum()).cpu().numpy()


def mesh_centroid(verts, faces):
    """area-weighted centroid of a mesh's surface -> float64 numpy [3] (works on CPU and CUDA tensors)"""
    area = meshdist.face_areas(verts, faces)
    cen = verts.to(torch.float64)[faces.long()].mean(1)
    cen = torch.nan_to_num(cen, nan=0.0, posinf=0.0, neginf=0.0)
    tot = area.sum()
    if not float(tot) > 0.0:
        return cen.mean(0).cpu().numpy()
    return ((cen * area[:, None]).sum(0) / tot).cpu().numpy()


def cube_inits(source_points, target, weights=None):
    """24 starts for `align(inits=...)`: every rotation of the cube about the centroids, each mapping the (weighted) centroid
    of the source points onto the area-weighted centroid of the target mesh (verts, faces) -> list of float64 numpy [4,4]"""
    cs = _centroid(source_points, weights)
    ct = mesh_centroid(*target)
    out = []
    for r in cube_rotations():
        m = np.eye(4)
        m[:3, :3] = r
        m[:3, 3] = ct - r @ cs
        out.append(m)
    return out


def _source(source, samples, seed):
    """-> (points, weights or None)"""
    if isinstance(source, (tuple, list)):
        sv, sf = meshdist._mesh_args(*source)
        pts, _, w = meshdist.sample_surface(sv, sf, samples, seed)
        return pts, w
    return source, None


def align(source, target, method="plane", with_scale=False, init=None, inits=None, coarse_iterations=4, max_iterations=30,
          tolerance=1e-7, max_dist=None, samples=20000, seed=0, weights=None, resolution=None):
    """Register `source` onto the mesh `target` = (verts, faces) (CUDA tensors) -> (matrix float64 numpy [4,4] taking source
    coordinates to target coordinates, info dict).

    source: points [N,3] (optionally with `weights` [N]) or a mesh (verts, faces), which is sampled with
    meshdist.sample_surface(samples, seed) and carries its area weights.  init: the start (4 x 4 similarity; None: identity).
    inits: a list of starts; each runs coarse_iterations, the one with the lowest rms is refined with max_iterations.
    Stops when the weighted rms distance changes by less than `tolerance`.  max_dist: points farther than this from the
    target take no part (None: all).  info: iterations, converged, rms, used, scale, and with inits: chosen (index) and
    candidate_rms (inf for a start that failed)."""
    if method not in METHODS:
        raise ValueError("method must be 'plane' or 'point'")
    if init is not None and inits is not None:
        raise ValueError("give init or inits, not both")
    if int(max_iterations) < 0 or int(coarse_iterations) < 0:
        raise ValueError("iterations must be >= 0")
    pts, w = _source(source, samples, seed)
    if weights is not None:
        w = weights
    pts = _points_arg(pts)
    dev = pts.device.index or 0
    kw = dict(method=method, with_scale=with_scale, tolerance=tolerance, max_dist=max_dist)
    with ffi.device_lock(dev):
        meshdist.build(target[0], target[1], resolution)
        extra = {}
        if inits is not None:
            if len(inits) == 0:
                raise ValueError("inits is empty")
            rms, mats = [], []
            for m0 in inits:
                try:
                    m, i = fit(pts, w, m0, max_iterations=coarse_iterations, **kw)
                    rms.append(i["rms"] if math.isfinite(i["rms"]) else float("inf"))
                    mats.append(m)
                except ffi.R3GError as e:
                    if "too few points" not in str(e):
                        raise
                    rms.append(float("inf"))
                    mats.append(None)
            best = int(np.argmin(rms))
            if mats[best] is None:
                raise ValueError("align: no start leaves 3 points within max_dist of the target")
            init = mats[best]
            extra = {"chosen": best, "candidate_rms": rms}
        matrix, info = fit(pts, w, init, max_iterations=max_iterations, **kw)
    info.update(extra)
    return matrix, info


def transform_points(matrix, points):
    """points [N,3] moved by a 4 x 4 matrix (float64 arithmetic, float32 result; any device)"""
    m = torch.as_tensor(np.asarray(matrix, np.float64), device=points.device)
    return (points.to(torch.float64) @ m[:3, :3].T + m[:3, 3]).to(torch.float32)


def compare_aligned(a, b, samples=200000, taus=None, include_vertices=True, resolution=None, seed=0, **kw):
    """Align mesh a = (verts, faces) onto mesh b, then r3g.meshdist.compare of the moved a against b: the distance of the
    shapes rather than of their poses.  kw goes to `align` (method, with_scale, init, inits, max_iterations, ...; its own
    `samples` is fit_samples here).  -> compare's dict plus matrix (4 x 4) and fit (align's info)."""
    fit_samples = kw.pop("fit_samples", 20000)
    av, af = meshdist._mesh_args(*a)
    matrix, info = align((av, af), b, samples=fit_samples, seed=seed, resolution=resolution, **kw)
    moved = transform_points(matrix, av)
    if np.linalg.det(matrix[:3, :3]) < 0:
        af = af[:, [0, 2, 1]].contiguous()
    out = meshdist.compare((moved, af), b, samples=samples, taus=taus, include_vertices=include_vertices, resolution=resolution,
                           seed=seed)
    out["matrix"] = matrix
    out["fit"] = info
    return out
