"""Plane fitting on the GPU: batched RANSAC, PCA refinement and the yaw search that start the reference's pose matching
(include/r3g.h "plane fit"; src/scene_reconstruction/source/pose_matching_planar.py upstream).

The primitives are `ransac_counts` / `fit_plane_ransac_refined` (r3g_plane_ransac: every hypothesis against every point in one
count launch, float64 predicate, integer counts) and `moments` (r3g_plane_moments: centroid, scatter and its eigenpairs, float64
sums in one fixed order).  The normal of a set is the eigenvector of the SMALLEST eigenvalue of its scatter, turned so that
n_y >= 0.  Upstream's fit_plane_svd takes a column of Vh where it means a row and so returns something else unless the
eigenvector matrix is symmetric up to signs; its docstring says what is computed here.  `best_initial_yaw`
runs on r3g.cloud's exact nearest neighbours; `yaw_obb` and `plane_frame` are small host-side definitions of this project.
CUDA tensors in and out; there is no CPU path."""
import ctypes
import math

import numpy as np
import torch

from . import cloud, ffi

RANSAC_REPORT = ("n_usable", "n_valid", "best", "best_count", "few")
MOMENTS_REPORT = ("n", "skipped", "few")
PASSES = ("table", "count", "winner", "moments")
MAX_HYPOTHESES = 65536


def _triples_arg(triples, device):
    t = torch.as_tensor(triples)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("expected triples [H,3]")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def ransac(points, triples, threshold, counts=True, mask=True):
    """r3g_plane_ransac -> dict(counts int32 [H] | None, mask uint8 [N] | None, report, plane float64 [16] numpy: the winner's
    p0 [0:3] and unit normal [3:6], the inliers' centroid [6:9], the refined normal [9:12], the eigenvalues ascending [12:15])"""
    p = cloud._cloud_arg(points)
    dev = p.device.index or 0
    t = _triples_arg(triples, p.device)
    n, h = p.shape[0], t.shape[0]
    cnt = torch.zeros((h,), dtype=torch.int32, device=p.device) if counts else None
    msk = torch.zeros((n,), dtype=torch.uint8, device=p.device) if mask else None
    rep, plane = (ctypes.c_int64 * 8)(), (ctypes.c_double * 16)()
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_plane_ransac(ffi.context(dev), _ptr(p), n, _ptr(t), h, float(threshold), _ptr(cnt), _ptr(msk), rep, plane,
                                             ffi.stream_ptr()))
    return {"counts": cnt, "mask": msk, "report": dict(zip(RANSAC_REPORT, (int(v) for v in rep))), "plane": np.array(list(plane), np.float64)}


def ransac_counts(points, triples, threshold):
    """count[h] = the points closer than `threshold` to the plane through the rows triples[h] (float64 test; 0 for a triple that
    spans no plane) -> (counts int32 [H], report dict: n_usable, n_valid, best (-1 without a valid triple), best_count, few)"""
    r = ransac(points, triples, threshold, counts=True, mask=False)
    return r["counts"], r["report"]


def times(device=0):
    """milliseconds of the passes of the last complete `ransac` on the device's context -> dict over PASSES"""
    ms = (ctypes.c_double * 4)()
    with ffi.device_lock(device):
        ffi.check(ffi.lib().r3g_plane_times(ffi.context(device), ms))
    return dict(zip(PASSES, (float(v) for v in ms)))


def moments(points, mask=None):
    """r3g_plane_moments of the rows with mask != 0 (all rows without a mask) -> dict(n, skipped, few, centroid [3], scatter [6]
    (xx, xy, xz, yy, yz, zz), eigenvalues [3] ascending, normal [3]; float64 numpy)"""
    p = cloud._cloud_arg(points)
    dev = p.device.index or 0
    m = None
    if mask is not None:
        m = mask.detach().to(device=p.device).ne(0).to(torch.uint8).contiguous()
        if tuple(m.shape) != (p.shape[0],):
            raise ValueError("expected mask [N]")
    out, rep = (ctypes.c_double * 16)(), (ctypes.c_int64 * 4)()
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_plane_moments(ffi.context(dev), _ptr(p), p.shape[0], _ptr(m), out, rep, ffi.stream_ptr()))
    o = np.array(list(out), np.float64)
    return {"n": int(rep[0]), "skipped": int(rep[1]), "few": int(rep[2]), "centroid": o[1:4], "scatter": o[4:10], "eigenvalues": o[10:13],
            "normal": o[13:16], "out": o}


def draw_triples(n, iterations, generator=None, sampler="fast"):
    """`iterations` index triples over n rows, int64 [iterations,3] on the CPU.  "fast": torch.randint from `generator`, a triple
    with a repeated index drawn again.  "reference": upstream's stream, one torch.randperm(n)[:3] per iteration from the global
    CPU generator."""
    if sampler == "reference":
        if n < 3:
            return torch.zeros((0, 3), dtype=torch.int64)
        return torch.stack([torch.randperm(n)[:3] for _ in range(int(iterations))]) if iterations else torch.zeros((0, 3), dtype=torch.int64)
    if sampler != "fast":
        raise ValueError("sampler must be 'fast' or 'reference'")
    if n < 3:
        return torch.zeros((0, 3), dtype=torch.int64)
    t = torch.randint(0, n, (int(iterations), 3), generator=generator)
    while True:
        bad = (t[:, 0] == t[:, 1]) | (t[:, 0] == t[:, 2]) | (t[:, 1] == t[:, 2])
        k = int(bad.sum())
        if not k:
            return t
        t[bad] = torch.randint(0, n, (k, 3), generator=generator)


def _chunks(triples):
    for lo in range(0, triples.shape[0], MAX_HYPOTHESES):
        yield lo, triples[lo:lo + MAX_HYPOTHESES]


def fit_plane_ransac_refined(points, iterations=2000, threshold=0.05, triples=None, generator=None, sampler="fast"):
    """Upstream's fit_plane_ransac_refined as one launch per 65536 hypotheses -> (normal float32 [3], point float32 [1,3],
    inlier_mask bool [N]): the hypothesis with the most points closer than `threshold` (the first one on a tie), then the
    eigenvector refinement on its inliers.  `triples` [H,3] overrides the sampler.  No triple spans a plane: ValueError."""
    p = cloud._cloud_arg(points)
    t = draw_triples(p.shape[0], iterations, generator, sampler) if triples is None else torch.as_tensor(triples)
    best = None
    for lo, part in _chunks(t) if t.shape[0] else ():
        r = ransac(p, part, threshold, counts=False)
        if r["report"]["best"] >= 0 and (best is None or r["report"]["best_count"] > best["report"]["best_count"]):
            best = r
    if best is None:
        raise ValueError("fit_plane_ransac_refined: no triple spans a plane")
    pl = best["plane"]
    normal = torch.tensor(pl[9:12], dtype=torch.float32, device=p.device)
    point = torch.tensor(pl[6:9], dtype=torch.float32, device=p.device).unsqueeze(0)
    return normal, point, best["mask"].bool()


def fit_plane_svd(points):
    """Upstream's fit_plane_svd as its docstring states it: the total-least-squares plane -> (normal float32 [3], the direction
    of smallest variance with n_y >= 0, centroid float32 [1,3])"""
    p = cloud._cloud_arg(points)
    m = moments(p)
    return (torch.tensor(m["normal"], dtype=torch.float32, device=p.device),
            torch.tensor(m["centroid"], dtype=torch.float32, device=p.device).unsqueeze(0))


def _rmse(p, normal, point):
    d = (p.to(torch.float64) - point.to(torch.float64)) @ normal.to(torch.float64)
    d = d[torch.isfinite(d)]
    return float(torch.sqrt((d * d).sum() / max(int(d.shape[0]), 1)))


def fit_floor(points, iterations=2000, threshold=0.05, triples=None, generator=None, sampler="fast"):
    """The selection rule of upstream's extract_and_fit_floor_plane: planarity = smallest / largest eigenvalue of the cloud's
    scatter; planarity < 1e-3 -> "pca"; otherwise an inlier ratio of the RANSAC fit below 0.85 -> "ransac"; otherwise "svd".
    ("pca" and "svd" are the same normal here; upstream's two differ)
    Where no triple spans a plane, a cloud below the planarity bound is still "pca" (ransac_rmse and inlier_ratio are then None);
    any other cloud raises ValueError.
    -> dict(method, normal [3], point [1,3], mask bool [N], svd_rmse, ransac_rmse, planarity, inlier_ratio)"""
    p = cloud._cloud_arg(points)
    if p.shape[0] == 0:
        raise ValueError("fit_floor: empty cloud")
    m = moments(p)
    svd_normal = torch.tensor(m["normal"], dtype=torch.float32, device=p.device)
    svd_point = torch.tensor(m["centroid"], dtype=torch.float32, device=p.device).unsqueeze(0)
    planarity = float(m["eigenvalues"][0] / m["eigenvalues"][2]) if m["eigenvalues"][2] > 0 else 0.0
    everything = torch.ones((p.shape[0],), dtype=torch.bool, device=p.device)
    out = {"svd_rmse": _rmse(p, svd_normal, svd_point), "ransac_rmse": None, "planarity": planarity, "inlier_ratio": None}
    try:
        r_normal, r_point, r_mask = fit_plane_ransac_refined(p, iterations, threshold, triples, generator, sampler)
    except ValueError:
        if planarity < 1e-3:      # the planarity test decides alone; the RANSAC figures stay None
            return dict(out, method="pca", normal=svd_normal, point=svd_point, mask=everything)
        raise
    ratio = float(r_mask.sum()) / p.shape[0]
    out.update(ransac_rmse=_rmse(p, r_normal, r_point), inlier_ratio=ratio)
    if planarity < 1e-3:
        return dict(out, method="pca", normal=svd_normal, point=svd_point, mask=everything)
    if ratio < 0.85:
        return dict(out, method="ransac", normal=r_normal, point=r_point, mask=r_mask)
    return dict(out, method="svd", normal=svd_normal, point=svd_point, mask=everything)


# ---- yaw search on r3g.cloud's nearest neighbours ---------------------------------------------------------------------------------
_CENTRES = {
    "bbox": lambda p: 0.5 * (p.amin(dim=0) + p.amax(dim=0)),      # the middle of the axis-aligned box
    "median": lambda p: p.median(dim=0).values,                   # per axis; the lower middle value of an even count
    "mean": lambda p: p.mean(dim=0),
}


def _centre(p, method):
    """the centre a cloud is rotated about, by name (a key of _CENTRES, any letter case)"""
    key = str(method).lower()
    if key not in _CENTRES:
        raise ValueError("centroid_method must be one of %s, not %r" % (", ".join(sorted(_CENTRES)), method))
    return _CENTRES[key](p)


def yaw_matrices(num_angles=18, device="cpu"):
    """R_y of upstream's candidates linspace(0, 2 * 3.14159, num_angles), both ends included -> float32 [num_angles,3,3]"""
    a = torch.linspace(0, 2 * 3.14159, int(num_angles), device=device)
    c, s, o, l = torch.cos(a), torch.sin(a), torch.zeros_like(a), torch.ones_like(a)
    return torch.stack([c, o, s, o, l, o, -s, o, c], dim=1).reshape(-1, 3, 3)


def best_initial_yaw(mesh_verts, target_points, num_angles=18, centroid_method="bbox"):
    """Upstream's find_best_initial_yaw (use_chamfer=True): both clouds centred, the vertices rotated about y by each candidate
    (verts @ R^T), loss = mean squared nearest-neighbour distance each way, summed; the first minimum wins.
    Two grid builds and 2 * num_angles exact nearest-neighbour queries: the target's grid serves the rotated vertices, the
    vertices' grid serves the inversely rotated targets, since d(R a, b) = d(a, R^T b).
    -> (R float32 [3,3], losses float32 [num_angles], index)"""
    v, t = cloud._cloud_arg(mesh_verts, "mesh_verts"), cloud._cloud_arg(target_points, "target_points")
    if v.shape[0] == 0 or t.shape[0] == 0:
        raise ValueError("best_initial_yaw: empty cloud")
    v, t = v - _centre(v, centroid_method), t - _centre(t, centroid_method)
    rs = yaw_matrices(num_angles, v.device)
    dev = v.device.index or 0
    fwd, bwd = [], []
    with ffi.device_lock(dev):
        cloud.build(t)
        for r in rs:
            fwd.append(cloud.knn((v @ r.T).contiguous(), 1)[0][:, 0].to(torch.float64).sum() / v.shape[0])
        cloud.build(v)
        for r in rs:
            bwd.append(cloud.knn((t @ r).contiguous(), 1)[0][:, 0].to(torch.float64).sum() / t.shape[0])
    losses = (torch.stack(fwd) + torch.stack(bwd)).to(torch.float32)
    index = int(torch.argmin(losses))
    return rs[index], losses, index


def yaw_obb(points):
    """Oriented bounding box with y kept up -> (centroid float64 [3], rotation float64 [3,3] about y, extents float64 [3]),
    numpy.  Columns 0 and 2 of the rotation are the principal axes of the cloud's scatter in xz (the major one first), taken
    from `moments`; extents are those of (p - centroid) @ rotation."""
    p = cloud._cloud_arg(points)
    m = moments(p)
    if m["n"] == 0:
        return np.zeros(3), np.eye(3), np.zeros(3)
    s = m["scatter"]
    theta = 0.5 * math.atan2(2.0 * s[2], s[0] - s[5])
    co, si = math.cos(theta), math.sin(theta)
    rot = np.array([[co, 0.0, -si], [0.0, 1.0, 0.0], [si, 0.0, co]])
    ok = torch.isfinite(p).all(dim=1)
    proj = (p[ok].to(torch.float64) - torch.from_numpy(m["centroid"]).to(p.device)) @ torch.from_numpy(rot).to(p.device)
    ext = (proj.max(dim=0).values - proj.min(dim=0).values).cpu().numpy()
    return m["centroid"].copy(), rot, ext


def plane_frame(normal, point):
    """The plane's frame -> (plane_to_world, world_to_plane), 4 x 4 float64 numpy acting on column vectors: plane-y is the unit
    normal, plane-z = normalise(y x ref), plane-x = normalise(y x z), ref = world X, or world Z when |n_x| > 0.9; the origin is
    `point`."""
    y = np.asarray(torch.as_tensor(normal).detach().cpu().numpy() if torch.is_tensor(normal) else normal, np.float64).reshape(3)
    o = np.asarray(torch.as_tensor(point).detach().cpu().numpy() if torch.is_tensor(point) else point, np.float64).reshape(3)
    y = y / np.linalg.norm(y)
    ref = np.array([0.0, 0.0, 1.0]) if abs(y[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    z = np.cross(y, ref)
    z = z / np.linalg.norm(z)
    x = np.cross(y, z)
    x = x / np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, o
    inv = np.eye(4)
    inv[:3, :3] = m[:3, :3].T
    inv[:3, 3] = -m[:3, :3].T @ o
    return m, inv
