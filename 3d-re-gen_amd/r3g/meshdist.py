"""Mesh-to-mesh distance on the GPU: Chamfer, Hausdorff and F-score (include/r3g.h "mesh distance").

The primitive is `nearest`: for every query point the exact distance to the closest point of a triangle mesh and the face
that holds it, by the uniform-grid kernels of csrc/meshdist_kernels.hip.  `sample_surface` turns a mesh into weighted
surface samples, `summarise` turns two sets of distances into the usual scores, `compare` does all of it for two meshes.

Definitions (`summarise`), for direction a->b with distances d_i >= 0 and weights w_i >= 0, W = sum w_i:
    mean   = sum w_i d_i / W                  rms = sqrt(sum w_i d_i^2 / W)              max = max_i d_i (weight-0 points count)
    p99    = the smallest d_k with sum{w_i : d_i <= d_k} >= 0.99 W                   within[tau] = sum{w_i : d_i <= tau} / W
and symmetric
    chamfer_l1 = mean_ab + mean_ba            chamfer_l2 = rms_ab^2 + rms_ba^2           hausdorff = max(max_ab, max_ba)
    fscore[tau] = 2 P R / (P + R) with P = within_ab[tau], R = within_ba[tau]; 0 where both are 0.
With area weights (`sample_surface`) the means are surface integrals divided by the area.
"""
import ctypes
import math

import torch

from . import ffi

_G = 1.32471795724474602596          # the plastic number: R2 low-discrepancy sequence (a1, a2) = (1/g, 1/g^2)
_A1, _A2 = 1.0 / _G, 1.0 / (_G * _G)


def _mesh_args(verts, faces):
    if not (torch.is_tensor(verts) and torch.is_tensor(faces) and verts.is_cuda and faces.is_cuda):
        raise ValueError("mesh buffers must live on the GPU (there is no CPU path)")
    v = verts.detach().to(torch.float32).contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("expected verts [V,3] and faces [F,3]")
    if f.device != v.device:
        raise ValueError("verts and faces live on different devices")
    return v, f


def build(verts, faces, resolution=None):
    """r3g_meshdist_build on the shared context of the mesh's device -> dict(resolution, pairs, skipped).
    The grid stays in the context until the next build; hold ffi.device_lock(device) across build and query."""
    v, f = _mesh_args(verts, faces)
    dev = v.device.index or 0
    res, pairs, skipped = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    with ffi.device_lock(dev), torch.cuda.device(v.device):
        ffi.check(ffi.lib().r3g_meshdist_build(ffi.context(dev), ctypes.c_void_p(v.data_ptr()), v.shape[0],
                                               ctypes.c_void_p(f.data_ptr()), f.shape[0], int(resolution or 0), ctypes.byref(res),
                                               ctypes.byref(pairs), ctypes.byref(skipped), ffi.stream_ptr()))
    return {"resolution": res.value, "pairs": pairs.value, "skipped": skipped.value}


def query(points):
    """r3g_meshdist_query against the last build on the points' device -> (dist2 float32 [N], face int32 [N])"""
    if not (torch.is_tensor(points) and points.is_cuda):
        raise ValueError("query points must live on the GPU (there is no CPU path)")
    p = points.detach().to(torch.float32).contiguous()
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("expected points [N,3]")
    dev = p.device.index or 0
    d2 = torch.empty(p.shape[0], dtype=torch.float32, device=p.device)
    face = torch.empty(p.shape[0], dtype=torch.int32, device=p.device)
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_meshdist_query(ffi.context(dev), ctypes.c_void_p(p.data_ptr()), p.shape[0],
                                               ctypes.c_void_p(d2.data_ptr()), ctypes.c_void_p(face.data_ptr()), ffi.stream_ptr()))
    return d2, face


def nearest(points, verts, faces, resolution=None):
    """Distance from every point to the mesh and the face holding the closest point -> (dist float32 [N], face int32 [N]).
    dist = sqrt(min over faces of tri_dist2); face = the lowest index attaining the minimum; a point with a non-finite
    coordinate gets (NaN, -1).  CUDA tensors only.  resolution: cells per axis of the grid (None: automatic); the result
    does not depend on it."""
    if not (torch.is_tensor(points) and points.is_cuda):
        raise ValueError("query points must live on the GPU (there is no CPU path)")
    dev = points.device.index or 0
    with ffi.device_lock(dev):
        build(verts, faces, resolution)
        d2, face = query(points)
    return d2.sqrt(), face


def closest(points):
    """r3g_meshdist_closest against the last build on the points' device
    -> (dist2 float32 [N], face int32 [N], closest float32 [N,3]); dist2 and face are `query`'s"""
    if not (torch.is_tensor(points) and points.is_cuda):
        raise ValueError("query points must live on the GPU (there is no CPU path)")
    p = points.detach().to(torch.float32).contiguous()
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("expected points [N,3]")
    dev = p.device.index or 0
    d2 = torch.empty(p.shape[0], dtype=torch.float32, device=p.device)
    face = torch.empty(p.shape[0], dtype=torch.int32, device=p.device)
    q = torch.empty((p.shape[0], 3), dtype=torch.float32, device=p.device)
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_meshdist_closest(ffi.context(dev), ctypes.c_void_p(p.data_ptr()), p.shape[0],
                                                 ctypes.c_void_p(d2.data_ptr()), ctypes.c_void_p(face.data_ptr()),
                                                 ctypes.c_void_p(q.data_ptr()), ffi.stream_ptr()))
    return d2, face, q


def closest_point(points, verts, faces, resolution=None):
    """trimesh.proximity.closest_point: for every point the closest point of the mesh, its distance and the face that holds
    it -> (closest float32 [N,3], dist float32 [N], face int32 [N]).  dist and face are `nearest`'s; closest is tri_closest of
    csrc/meshdist_core.h on that face.  A point with a non-finite coordinate gets (NaN, NaN, -1).  CUDA tensors only."""
    if not (torch.is_tensor(points) and points.is_cuda):
        raise ValueError("query points must live on the GPU (there is no CPU path)")
    dev = points.device.index or 0
    with ffi.device_lock(dev):
        build(verts, faces, resolution)
        d2, face, q = closest(points)
    return q, d2.sqrt(), face


def face_areas(verts, faces):
    """float64 [F]; a face with a non-finite vertex has area 0"""
    t = verts.to(torch.float64)[faces.long()]
    n = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return torch.nan_to_num(0.5 * n.norm(dim=1), nan=0.0, posinf=0.0, neginf=0.0)


def sample_surface(verts, faces, n, seed=0):
    """Stratified surface samples -> (points float32 [S,3], face int64 [S], weight float64 [S]).
    Face f gets count_f = max(1, ceil(area_f * n / A)) samples (A = total area), so S <= n + F and no face goes unsampled.
    Sample k of face f sits at the k-th point of a fixed low-discrepancy sequence (R2, started at an offset that depends on
    seed and f) folded into the triangle, and carries weight area_f / count_f: weighted sums are surface integrals.
    Works on CPU and CUDA tensors (torch ops only: O(n) plumbing)."""
    nf = int(faces.shape[0])
    if nf == 0:
        raise ValueError("sample_surface: the mesh has no face")
    area = face_areas(verts, faces)
    total = area.sum()
    if float(total) > 0.0:
        count = torch.clamp(torch.ceil(area * (float(n) / total)), min=1.0).long()
    else:
        count = torch.ones(nf, dtype=torch.long, device=area.device)
    fidx = torch.repeat_interleave(torch.arange(nf, device=area.device), count)
    first = torch.cumsum(count, 0) - count
    k = torch.arange(int(fidx.shape[0]), device=area.device) - first[fidx]
    idx = (k + 1 + (fidx * 31 + int(seed) * 9973) % 65536).to(torch.float64)
    u = torch.frac(0.5 + _A1 * idx)
    v = torch.frac(0.5 + _A2 * idx)
    flip = (u + v) > 1.0
    u = torch.where(flip, 1.0 - u, u)
    v = torch.where(flip, 1.0 - v, v)
    t = verts.to(torch.float64)[faces.long()[fidx]]
    pts = t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])
    return pts.to(torch.float32), fidx, (area / count.to(torch.float64))[fidx]


def _direction(d, w, taus):
    d = d.to(torch.float64).reshape(-1)
    w = w.to(torch.float64).reshape(-1)
    tot = w.sum()
    order = torch.argsort(d)
    cw = torch.cumsum(w[order], 0)
    k = int(torch.searchsorted(cw, (0.99 * tot).reshape(1)).clamp(max=d.numel() - 1))
    return {"mean": float((w * d).sum() / tot), "rms": math.sqrt(float((w * d * d).sum() / tot)), "max": float(d.max()),
            "p99": float(d[order][k]), "within": {float(t): float(w[d <= float(t)].sum() / tot) for t in taus}}


def summarise(d_ab, w_ab, d_ba, w_ba, taus=()):
    """Scores of two one-sided distance sets (definitions in the module docstring).  Pure tensor arithmetic on any device.
    -> dict(ab, ba: dict(mean, rms, max, p99, within{tau}); chamfer_l1, chamfer_l2, hausdorff, fscore{tau})"""
    ab, ba = _direction(d_ab, w_ab, taus), _direction(d_ba, w_ba, taus)
    fscore = {}
    for t in ab["within"]:
        p, r = ab["within"][t], ba["within"][t]
        fscore[t] = 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0
    return {"ab": ab, "ba": ba, "chamfer_l1": ab["mean"] + ba["mean"], "chamfer_l2": ab["rms"] ** 2 + ba["rms"] ** 2,
            "hausdorff": max(ab["max"], ba["max"]), "fscore": fscore}


def _one_way(src, dst, samples, include_vertices, resolution, seed):
    """samples of src against the grid of dst -> (dist, weight, info, query_ms)"""
    sv, sf = _mesh_args(*src)
    pts, _, w = sample_surface(sv, sf, samples, seed)
    if include_vertices:
        used = torch.unique(sf.long().reshape(-1))
        pts = torch.cat([pts, sv[used]])
        w = torch.cat([w, torch.zeros(used.shape[0], dtype=w.dtype, device=w.device)])
    dev = sv.device.index or 0
    with ffi.device_lock(dev), torch.cuda.device(sv.device):
        info = build(*dst, resolution)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d2, _ = query(pts)
        e1.record()
        e1.synchronize()
    keep = torch.isfinite(d2)          # samples of faces with a non-finite vertex have no distance
    return d2[keep].sqrt(), w[keep], info, e0.elapsed_time(e1)


def compare(a, b, samples=200000, taus=None, include_vertices=True, resolution=None, seed=0):
    """Distance between two meshes a = (verts, faces), b = (verts, faces) (CUDA tensors): `samples` area-weighted surface
    samples per direction (plus, with include_vertices, every referenced vertex at weight 0: it takes no part in the means
    but full part in the maxima), one build and one query per direction.  taus: distances for within / fscore (None: one
    percent of a's largest bounding-box side).
    -> the dict of `summarise` plus samples (ab, ba), resolution (of b's grid, of a's grid), skipped (b, a), query_ms (the two
    queries, HIP events)"""
    if taus is None:
        av = _mesh_args(*a)[0]
        taus = (0.01 * float((av.max(0).values - av.min(0).values).max()),)
    d_ab, w_ab, info_b, ms_ab = _one_way(a, b, samples, include_vertices, resolution, seed)
    d_ba, w_ba, info_a, ms_ba = _one_way(b, a, samples, include_vertices, resolution, seed)
    out = summarise(d_ab, w_ab, d_ba, w_ba, taus)
    out.update({"samples": (int(d_ab.shape[0]), int(d_ba.shape[0])), "resolution": (info_b["resolution"], info_a["resolution"]),
                "skipped": (info_b["skipped"], info_a["skipped"]), "query_ms": ms_ab + ms_ba})
    return out


def voxel_size(box_v, octree_resolution):
    """Edge of one voxel of the extraction grid in mesh units, so that tau can be given in voxels: the pipeline maps index
    space to the box [-box_v, box_v]^3 by v / (R + 1) * 2 box_v - box_v (include/r3g.h, r3g_mc_emit's xform)."""
    return 2.0 * float(box_v) / (int(octree_resolution) + 1)


def grid_mesh_distance(grid_exact, grid_approx, mc_level, box_v, octree_resolution, samples=200000):
    """The mesh-level error of an approximate grid of logits: both grids through marching cubes (r3g.mc.extract_mesh, the
    pipeline's extraction), then `compare` with tau = one voxel.  -> dict(chamfer_l1, hausdorff, p99 (the larger of the two
    directions), within_one_voxel (the smaller of the two shares), voxel, faces (exact, approx), query_ms), all lengths in
    mesh units; dict(error=...) when a grid has no surface.  For the tools that time an opt-in approximation.  These figures
    are unsigned: on which side of the exact surface the approximation lies is r3g.meshinside.signed_distance's to say."""
    from . import mc
    try:
        a = mc.extract_mesh(grid_exact, mc_level, box_v, octree_resolution)
        b = mc.extract_mesh(grid_approx, mc_level, box_v, octree_resolution)
    except (ffi.LevelRangeError, ffi.NoSurfaceError) as e:
        return {"error": str(e)}
    vox = voxel_size(box_v, octree_resolution)
    s = compare((a[0], a[1]), (b[0], b[1]), samples=samples, taus=(vox,))
    return {"chamfer_l1": s["chamfer_l1"], "hausdorff": s["hausdorff"], "p99": max(s["ab"]["p99"], s["ba"]["p99"]),
            "within_one_voxel": min(s["ab"]["within"][vox], s["ba"]["within"][vox]), "voxel": vox,
            "faces": (int(a[1].shape[0]), int(b[1].shape[0])), "query_ms": s["query_ms"]}
