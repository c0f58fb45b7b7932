"""Point clouds on the GPU: exact k nearest neighbours and what the reference's evaluation builds on them
(include/r3g.h "point clouds").

The primitive is `knn`: for every query point the k smallest (d2, index) pairs over the target cloud, d2 = ((px-qx)^2 +
(py-qy)^2) + (pz-qz)^2 in float32, by the uniform-grid kernels of csrc/cloud_kernels.hip.  Everything else here is thin
device-side tensor arithmetic on its output: the scores of the reference's src/evaluation/run_eval.py (`evaluate`), the
normals that stand in front of its Poisson step (`estimate_normals`) and its cloud ICP (`icp`).  Means and sums are taken
in float64 on the device.  `dbscan` (section 4m, csrc/dbscan_kernels.hip) is the second primitive: scikit-learn's DBSCAN
labels, on which the reference's cloud cleaning rests (`filter_dbscan`, beside `filter_points_by_quantile`).  CUDA tensors in and out; there is no CPU path.  `PointCloud`, `load_ply` and `save_ply` are the
host-side file layer (numpy) behind compat/trimesh.
"""
import ctypes

import numpy as np
import torch

from . import ffi


def _cloud_arg(points, what="points"):
    if not (torch.is_tensor(points) and points.is_cuda):
        raise ValueError("%s must live on the GPU (there is no CPU path)" % what)
    p = points.detach().to(torch.float32).contiguous()
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("expected %s [N,3]" % what)
    return p


def build(points, resolution=None):
    """r3g_cloud_build on the shared context of the points' device -> dict(resolution, skipped).
    The context keeps its own packed copy until the next build (`points` may be freed); hold ffi.device_lock(device)
    across build and knn."""
    p = _cloud_arg(points)
    dev = p.device.index or 0
    res, skipped = ctypes.c_int(0), ctypes.c_int64(0)
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_cloud_build(ffi.context(dev), ctypes.c_void_p(p.data_ptr()), p.shape[0], int(resolution or 0),
                                            ctypes.byref(res), ctypes.byref(skipped), ffi.stream_ptr()))
    return {"resolution": res.value, "skipped": skipped.value}


def knn(queries, k=1):
    """r3g_cloud_knn against the last build on the queries' device -> (dist2 float32 [N,k], index int32 [N,k]), each row
    ascending by (dist2, index); (+inf, -1) past the number of usable points, (NaN, -1) for a non-finite query."""
    q = _cloud_arg(queries, "queries")
    dev = q.device.index or 0
    k = int(k)
    d2 = torch.empty((q.shape[0], max(k, 0)), dtype=torch.float32, device=q.device)
    idx = torch.empty((q.shape[0], max(k, 0)), dtype=torch.int32, device=q.device)
    with ffi.device_lock(dev), torch.cuda.device(q.device):
        ffi.check(ffi.lib().r3g_cloud_knn(ffi.context(dev), ctypes.c_void_p(q.data_ptr()), q.shape[0], k,
                                          ctypes.c_void_p(d2.data_ptr()), ctypes.c_void_p(idx.data_ptr()), ffi.stream_ptr()))
    return d2, idx


def nearest(queries, points, resolution=None):
    """Distance from every query to its nearest point of `points` and that point's index -> (dist float32 [N], index int32
    [N]): dist = sqrt(min d2), index = the lowest one attaining it; a non-finite query gets (NaN, -1).  The result does not
    depend on `resolution` (cells per axis; None: automatic)."""
    q = _cloud_arg(queries, "queries")
    dev = q.device.index or 0
    with ffi.device_lock(dev):
        build(points, resolution)
        d2, idx = knn(q, 1)
    return d2[:, 0].sqrt(), idx[:, 0]


# ---- every triangle's nearest point ---------------------------------------------------------------------------
FACES_REPORT = ("usable", "tests", "wide", "max_ring")
FACES_PASSES = ("classify", "narrow", "wide", "gather")


def _mesh_arg(verts, faces):
    if not (torch.is_tensor(verts) and verts.is_cuda and torch.is_tensor(faces) and faces.is_cuda):
        raise ValueError("verts and faces must live on the GPU (there is no CPU path)")
    v = verts.detach().to(torch.float32).contiguous()
    f = faces.detach().to(torch.int32).contiguous()
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("expected verts [V,3] and faces [F,3]")
    return v, f


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t.numel() else None)


def face_nearest(verts, faces):
    """r3g_cloud_faces against the last `build` (or `orient_normals`, `dbscan`) on the mesh's device: for every face the nearest
    usable point of the cloud -> (dist2 float32 [F], index int32 [F], weights float32 [F,3], diff float32 [F,3], info dict: usable,
    tests, wide, max_ring).  dist2 is section 4f's float32 point-triangle function, index the lowest original index attaining the
    minimum; weights are the barycentrics of the face's closest point r to that point, diff = p_index - r.  A face with an index
    outside [0, V) or a non-finite vertex gets (NaN, -1, 0, 0).  The cloud is read and left as it is; hold ffi.device_lock(device)
    across build and face_nearest."""
    v, f = _mesh_arg(verts, faces)
    dev = v.device.index or 0
    n = f.shape[0]
    d2 = torch.empty((n,), dtype=torch.float32, device=v.device)
    idx = torch.empty((n,), dtype=torch.int32, device=v.device)
    w = torch.empty((n, 3), dtype=torch.float32, device=v.device)
    diff = torch.empty((n, 3), dtype=torch.float32, device=v.device)
    rep = (ctypes.c_int64 * 4)()
    with ffi.device_lock(dev), torch.cuda.device(v.device):
        ffi.check(ffi.lib().r3g_cloud_faces(ffi.context(dev), _ptr(v), v.shape[0], _ptr(f), n, _ptr(d2), _ptr(idx), _ptr(w), _ptr(diff), rep,
                                            ffi.stream_ptr()))
    return d2, idx, w, diff, dict(zip(FACES_REPORT, (int(x) for x in rep)))


def face_nearest_backward(grad_dist2, index, weights, diff, csr, n_verts):
    """r3g_cloud_faces_backward: grad_dist2 [F] and face_nearest's index, weights and diff -> grad_verts float32 [V,3], summed over
    the corner lists csr = r3g.softras.corner_csr(faces, V) without floating-point atomics"""
    g = grad_dist2.detach().to(torch.float32).contiguous()
    start, ids = csr
    if ids.numel() == 0 and g.shape[0]:      # no corner in range at all: the library refuses a NULL list while there are faces
        ids = torch.full((1,), -1, dtype=torch.int32, device=g.device)
    dev = g.device.index or 0
    out = torch.empty((n_verts, 3), dtype=torch.float32, device=g.device)
    with ffi.device_lock(dev), torch.cuda.device(g.device):
        ffi.check(ffi.lib().r3g_cloud_faces_backward(ffi.context(dev), int(n_verts), g.shape[0], _ptr(g), _ptr(index), _ptr(weights), _ptr(diff),
                                                     _ptr(start), _ptr(ids), _ptr(out), ffi.stream_ptr()))
    return out


def faces_times(device=0):
    """milliseconds of the passes of the last complete `face_nearest` (and backward) on the device's context -> dict over FACES_PASSES
    (gather: -1 while no backward has run)"""
    ms = (ctypes.c_double * 4)()
    with ffi.device_lock(device):
        ffi.check(ffi.lib().r3g_cloud_faces_times(ffi.context(device), ms))
    return dict(zip(FACES_PASSES, (float(v) for v in ms)))


class FaceCloudDistance(torch.autograd.Function):
    """verts [V,3] -> dist2 [F] of `face_nearest` against the cloud on the device's context, differentiable in the vertices:
    FaceCloudDistance.apply(verts, faces, csr) with csr = r3g.softras.corner_csr(faces, V).  The backward holds each face's nearest
    point (index) and the barycentric weights w of its closest point constant: d dist2 / d vertex_a = -2 w_a (p - r).  Because r
    minimises over the triangle and p_index over the cloud, the derivatives through w and through the choice of the point vanish,
    so this is the exact gradient wherever the distance is differentiable.  The CLOUD GETS NO GRADIENT: it lives on the context as
    a packed copy and is no input here.  Unusable faces (dist2 NaN) and non-finite incoming gradients contribute nothing.
    Do not hold ffi.device_lock(device) around backward(): autograd runs the backward on a thread of its own, which takes the lock
    itself (as r3g.softras's does)."""

    @staticmethod
    def forward(ctx, verts, faces, csr):
        d2, idx, w, diff, info = face_nearest(verts, faces)
        ctx.save_for_backward(idx, w, diff, csr[0], csr[1])
        ctx.n_verts, ctx.dtype = verts.shape[0], verts.dtype
        return d2.to(verts.dtype)

    @staticmethod
    def backward(ctx, grad_dist2):
        idx, w, diff, start, ids = ctx.saved_tensors
        g = face_nearest_backward(grad_dist2, idx, w, diff, (start, ids), ctx.n_verts)
        return g.to(ctx.dtype), None, None


# ---- the reference's evaluation (src/evaluation/run_eval.py, src/utils/metrics.py), each stated once ---------------------------
def _both_ways(a, b):
    """unsquared NN distances a->b and b->a"""
    return nearest(a, b)[0], nearest(b, a)[0]


def chamfer_distance(a, b):
    """[UPSTREAM-RECALLED] pytorch3d.loss.chamfer_distance(a, b, point_reduction="mean", norm=2) for one pair of clouds, as
    recalled: the mean over a of the SQUARED distance to the nearest point of b, plus the same from b to a (batch of one, so
    the batch reduction changes nothing).  -> (cd, cd_ab, cd_ba) as Python floats; the means are float64 sums of the float32
    squared distances."""
    a, b = _cloud_arg(a, "a"), _cloud_arg(b, "b")
    dev = a.device.index or 0
    with ffi.device_lock(dev):
        build(b)
        d_ab = knn(a, 1)[0][:, 0]
        build(a)
        d_ba = knn(b, 1)[0][:, 0]
    ab = float(d_ab.to(torch.float64).sum() / d_ab.shape[0])
    ba = float(d_ba.to(torch.float64).sum() / d_ba.shape[0])
    return ab + ba, ab, ba


def hausdorff(a, b):
    """max(max over a of dist(a_i, b), max over b of dist(b_j, a)), unsquared (point-cloud-utils' hausdorff_distance)"""
    d_ab, d_ba = _both_ways(a, b)
    return max(float(d_ab.max()), float(d_ba.max()))


def fscore(pred, gt, tau=0.1):
    """metrics.py::compute_fscore: P = share of pred points strictly closer than tau to gt, R = share of gt points strictly
    closer than tau to pred, 2 P R / (P + R + 1e-8), the shares and the ratio in float32 as upstream has them."""
    d_pg, d_gp = _both_ways(pred, gt)
    tau = float(tau)
    p = (d_pg < tau).to(torch.float64).sum().to(torch.float32) / d_pg.shape[0]
    r = (d_gp < tau).to(torch.float64).sum().to(torch.float32) / d_gp.shape[0]
    return float(2 * (p * r) / (p + r + 1e-8))


def precision_recall(pred, gt, threshold=0.01):
    """run_eval.py::compute_precision_recall, WITH ITS NAMING: `precision` is the share of **gt** points strictly within
    `threshold` of pred (it queries pred's tree with the gt points), `recall` the share of pred points within it of gt --
    the reverse of the usual convention, and of `fscore` above.  Kept so that the numbers compare with upstream's reports.
    -> (precision, recall) as Python floats"""
    d_pg, d_gp = _both_ways(pred, gt)
    t = float(threshold)
    precision = float((d_gp < t).to(torch.float64).sum() / d_gp.shape[0])
    recall = float((d_pg < t).to(torch.float64).sum() / d_pg.shape[0])
    return precision, recall


def _voxelize(points, voxel_size, grid_size, min_bound):
    idx = torch.floor((points - min_bound) / voxel_size).long().clamp(0, grid_size - 1)
    grid = torch.zeros((grid_size, grid_size, grid_size), dtype=torch.bool, device=points.device)
    grid[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    return grid


def volume_iou(pred, gt, voxel_size=0.05, grid_size=64, mode="pcd"):
    """metrics.py::compute_volume_iou in its own float32 arithmetic, torch ops only.  mode "pcd": both clouds voxelised from
    their common lower corner (floor((x - min) / voxel_size), clamped to the grid), occupied voxels intersected and united;
    mode "bbox": the IoU of the two axis-aligned bounding boxes.  Both / (union + 1e-8)."""
    pred, gt = _cloud_arg(pred, "pred"), _cloud_arg(gt, "gt")
    if mode == "pcd":
        min_bound = torch.min(pred.min(0).values, gt.min(0).values)
        pv = _voxelize(pred, voxel_size, grid_size, min_bound)
        gv = _voxelize(gt, voxel_size, grid_size, min_bound)
        inter = (pv & gv).sum().float()
        union = (pv | gv).sum().float()
        return float(inter / (union + 1e-8))
    if mode == "bbox":
        pmin, pmax, gmin, gmax = pred.min(0).values, pred.max(0).values, gt.min(0).values, gt.max(0).values
        inter = (torch.min(pmax, gmax) - torch.max(pmin, gmin)).clamp(min=0)
        inter_vol = inter[0] * inter[1] * inter[2]
        pd, gd = (pmax - pmin).clamp(min=0), (gmax - gmin).clamp(min=0)
        union_vol = pd[0] * pd[1] * pd[2] + gd[0] * gd[1] * gd[2] - inter_vol
        return float(inter_vol / (union_vol + 1e-8))
    raise ValueError("Invalid mode: %s" % mode)


def evaluate(pred, gt):
    """The point-cloud scores of run_eval.py under its keys: CD (`chamfer_distance`), FSCORE (`fscore`, tau 0.1), IOU_BBOX
    (`volume_iou`, mode "bbox"), HAUSDORFF, PRECISION and RECALL (`precision_recall`, threshold 0.01, upstream's naming).
    Two builds and two queries serve all of them."""
    pred, gt = _cloud_arg(pred, "pred"), _cloud_arg(gt, "gt")
    dev = pred.device.index or 0
    with ffi.device_lock(dev):
        build(gt)
        d2_pg = knn(pred, 1)[0][:, 0]
        build(pred)
        d2_gp = knn(gt, 1)[0][:, 0]
    d_pg, d_gp = d2_pg.sqrt(), d2_gp.sqrt()
    n_p, n_g = d_pg.shape[0], d_gp.shape[0]
    p = (d_pg < 0.1).to(torch.float64).sum().to(torch.float32) / n_p
    r = (d_gp < 0.1).to(torch.float64).sum().to(torch.float32) / n_g
    return {"CD": float(d2_pg.to(torch.float64).sum() / n_p) + float(d2_gp.to(torch.float64).sum() / n_g),
            "FSCORE": float(2 * (p * r) / (p + r + 1e-8)),
            "IOU_BBOX": volume_iou(pred, gt, mode="bbox"),
            "HAUSDORFF": max(float(d_pg.max()), float(d_gp.max())),
            "PRECISION": float((d_gp < 0.01).to(torch.float64).sum() / n_g),
            "RECALL": float((d_pg < 0.01).to(torch.float64).sum() / n_p)}


# ---- normals ---------------------------------------------------------------------------------------------------------------------
def neighbour_covariances(points, k=30):
    """float64 covariance of each point's k nearest neighbours in the cloud itself (the point included, as Open3D's KNN search
    has it) -> (cov float64 [N,3,3], count int64 [N], index int32 [N,k]).  Gathered and summed in the k-list's order, one
    operation at a time: mean = (sum_j x_j) / count, cov = (sum_j (x_j - mean)(x_j - mean)^T) / count.  Slots without a
    neighbour (index -1) take no part."""
    p = _cloud_arg(points)
    dev = p.device.index or 0
    with ffi.device_lock(dev):
        build(p)
        _, idx = knn(p, k)
    have = idx >= 0
    count = have.sum(1)
    w = have.to(torch.float64)
    nb = p.to(torch.float64)[idx.clamp(min=0).long()]         # [N,k,3]
    nb = torch.where(have[:, :, None], nb, torch.zeros_like(nb))
    s = torch.zeros((p.shape[0], 3), dtype=torch.float64, device=p.device)
    for j in range(idx.shape[1]):
        s = s + nb[:, j]
    cnt = count.clamp(min=1).to(torch.float64)
    mean = s / cnt[:, None]
    d = (nb - mean[:, None, :]) * w[:, :, None]
    cov = torch.zeros((p.shape[0], 3, 3), dtype=torch.float64, device=p.device)
    for j in range(idx.shape[1]):
        outer = d[:, j, :, None] * d[:, j, None, :]
        cov = cov + outer
    return cov / cnt[:, None, None], count, idx


ORIENT_MAX_K = 31


def orient_normals(points, normals, k=30, resolution=None):
    """Open3D's pcd.orient_normals_consistent_tangent_plane(k): the sign of every normal by propagation over the minimum
    spanning forest of the k-nearest-neighbour graph under the weight 1 - |n_i . n_j| (r3g_cloud_orient, DESIGN.md section
    4l) -> (oriented normals float32 [N,3], info dict: sign int8 [N], tree int32 [N], usable, trees, flipped, rounds,
    frustrated, k).  k is clamped to [1, 31] (upstream's usual 100 becomes 31: the neighbour lists hold at most 32 entries).
    In every tree the point with the largest z ends with n_z >= 0; separate trees (k-NN components) are not connected to each
    other.  A point that is not usable (non-finite, or a zero normal) keeps its normal and gets sign 0.  The call replaces
    the cloud of `build` on the device's shared context (built at `resolution` cells per axis, None: automatic; the result does
    not depend on it)."""
    p, nr = _cloud_arg(points), _cloud_arg(normals, "normals")
    if p.shape != nr.shape:
        raise ValueError("points and normals differ in shape")
    k = min(max(int(k), 1), ORIENT_MAX_K)
    dev = p.device.index or 0
    sign = torch.zeros(p.shape[0], dtype=torch.int8, device=p.device)
    tree = torch.full((p.shape[0],), -1, dtype=torch.int32, device=p.device)
    rep = (ctypes.c_int64 * 8)()
    if p.shape[0]:
        with ffi.device_lock(dev), torch.cuda.device(p.device):
            ffi.check(ffi.lib().r3g_cloud_orient(ffi.context(dev), ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(nr.data_ptr()), p.shape[0], k,
                                                 int(resolution or 0), ctypes.c_void_p(sign.data_ptr()), ctypes.c_void_p(tree.data_ptr()), rep, ffi.stream_ptr()))
    out = torch.where((sign < 0)[:, None], -nr, nr)
    info = {"sign": sign, "tree": tree, "usable": rep[0], "trees": rep[1], "flipped": rep[2], "rounds": rep[3], "frustrated": rep[4], "k": k}
    return out, info


def estimate_normals(points, k=30, orient=False, k_orient=30):
    """Open3D's pcd.estimate_normals(KDTreeSearchParamKNN(k)): the unit eigenvector of the smallest eigenvalue of the
    covariance of each point's k nearest neighbours (`neighbour_covariances`, torch.linalg.eigh in float64) -> float32 [N,3].
    The SIGN is left open -- n and -n are the same plane -- unless orient=True, which hands the result to `orient_normals`
    (k_orient neighbours) and returns its normals.  A point with fewer than 3 usable neighbours (itself included) gets NaN,
    and so does a non-finite point."""
    if orient:
        return orient_normals(points, estimate_normals(points, k), k_orient)[0]
    cov, count, _ = neighbour_covariances(points, k)
    ok = (count >= 3) & torch.isfinite(cov).all(-1).all(-1)
    eye = torch.eye(3, dtype=torch.float64, device=cov.device)
    _, vec = torch.linalg.eigh(torch.where(ok[:, None, None], cov, eye))
    n = vec[:, :, 0]
    n = n / n.norm(dim=1, keepdim=True)
    n = torch.where(ok[:, None], n, torch.full_like(n, float("nan")))
    return n.to(torch.float32)


# ---- cleaning: DBSCAN and the reference's two filters ----------------------------------------------------------------------------
DBSCAN_REPORT = ("n_usable", "n_core", "n_border", "n_noise", "n_clusters", "largest", "largest_size", "resolution")
DBSCAN_PASSES = ("build", "count", "link", "border", "number")


def dbscan(points, eps=0.05, min_samples=10, resolution=None, counts=False):
    """sklearn.cluster.DBSCAN(eps, min_samples).fit(points).labels_ on the GPU (r3g_cloud_dbscan)
    -> (labels int32 [N], report dict), or (labels, counts int32 [N], report) with counts=True.  q is a neighbour of p iff
    ((dx*dx) + dy*dy) + dz*dz <= eps*eps in float64 on the float32 coordinates; counts[i] = neighbours of i, itself included;
    clusters are numbered in ascending order of their smallest core index, a border point takes the smallest number among its
    core neighbours, noise and points with a non-finite coordinate get -1.  report: n_usable, n_core, n_border, n_noise,
    n_clusters, largest (most points, the lowest number on a tie, -1 without a cluster), largest_size, resolution.  The call
    replaces the cloud of `build` on the device's shared context by the usable points (built at `resolution` cells per axis,
    None: about eps a cell; the result does not depend on it)."""
    p = _cloud_arg(points)
    dev = p.device.index or 0
    n = p.shape[0]
    labels = torch.full((n,), -1, dtype=torch.int32, device=p.device)
    cnt = torch.zeros((n,), dtype=torch.int32, device=p.device) if counts else None
    rep = (ctypes.c_int64 * 8)()
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_cloud_dbscan(ffi.context(dev), ctypes.c_void_p(p.data_ptr() if n else None), n, float(eps), int(min_samples),
                                             int(resolution or 0), ctypes.c_void_p(labels.data_ptr() if n else None),
                                             ctypes.c_void_p(cnt.data_ptr()) if counts and n else None, rep, ffi.stream_ptr()))
    report = dict(zip(DBSCAN_REPORT, (int(v) for v in rep)))
    return (labels, cnt, report) if counts else (labels, report)


def dbscan_times(device=0):
    """milliseconds of the passes of the last complete `dbscan` on the device's context (HIP events on its stream)
    -> dict over DBSCAN_PASSES"""
    ms = (ctypes.c_double * 5)()
    with ffi.device_lock(device):
        ffi.check(ffi.lib().r3g_cloud_dbscan_times(ffi.context(device), ms))
    return dict(zip(DBSCAN_PASSES, (float(v) for v in ms)))


def filter_dbscan(points, eps=0.05, min_samples=10):
    """The reference's pc_utils.filter_dbscan without its trip to the host: the points of the largest DBSCAN cluster, in
    their order; the input itself when there is no cluster (or no point)."""
    if points.numel() == 0:
        return points
    labels, report = dbscan(points, eps, min_samples)
    if report["n_clusters"] == 0:
        return points
    return points[labels == report["largest"]]


def filter_points_by_quantile(points, q=0.02):
    """The reference's pc_utils.filter_points_by_quantile: the points inside the [q, 1 - q] quantiles (torch.quantile, linear
    interpolation) of all three axes, bounds included; the input itself when it is empty or nothing would remain."""
    if points.numel() == 0:
        return points
    lower = torch.quantile(points, q, dim=0)
    upper = torch.quantile(points, 1 - q, dim=0)
    kept = points[((points >= lower) & (points <= upper)).all(dim=1)]
    return points if kept.numel() == 0 else kept


# ---- cloud ICP -------------------------------------------------------------------------------------------------------------------
def rigid_transform(a, b):
    """metrics.py::compute_rigid_transform: the rotation R and translation t that minimise sum |R a_i + t - b_i|^2 (Kabsch,
    with the reflection fix: the last singular direction is negated when det < 0).  Sums in float64.  a, b [N,3]
    -> (R float64 [3,3], t float64 [3])"""
    a64, b64 = a.to(torch.float64), b.to(torch.float64)
    ca, cb = a64.sum(0) / a64.shape[0], b64.sum(0) / b64.shape[0]
    h = (a64 - ca).T @ (b64 - cb)
    u, _, vh = torch.linalg.svd(h)
    v = vh.T
    det = torch.linalg.det(v @ u.T)
    diag = torch.diag(torch.stack([torch.ones_like(det), torch.ones_like(det), det]))
    r = v @ diag @ u.T
    return r, cb - r @ ca


def icp(src, dst, max_iterations=20, tolerance=1e-5):
    """metrics.py::icp for one pair of clouds: per iteration the nearest point of dst to every moved source point (knn, k = 1,
    one build of dst for all iterations), `rigid_transform` on those pairs, the move, and upstream's stop test
    |previous mean distance - mean distance| < tolerance on the mean distance to the pairs just used.  The moved points are
    float32 (they are what the next search sees); R, t and every sum are float64.
    -> (moved float32 [N,3], R float64 [3,3], t float64 [3]) with moved ~ src @ R^T + t"""
    cur, dst = _cloud_arg(src, "src").clone(), _cloud_arg(dst, "dst")
    dev = cur.device.index or 0
    r_all = torch.eye(3, dtype=torch.float64, device=cur.device)
    t_all = torch.zeros(3, dtype=torch.float64, device=cur.device)
    prev = float("inf")
    with ffi.device_lock(dev):
        build(dst)
        for _ in range(int(max_iterations)):
            _, idx = knn(cur, 1)
            near = dst[idx[:, 0].clamp(min=0).long()]
            r, t = rigid_transform(cur, near)
            cur = (cur.to(torch.float64) @ r.T + t).to(torch.float32)
            r_all, t_all = r @ r_all, r @ t_all + t
            err = float((cur.to(torch.float64) - near.to(torch.float64)).norm(dim=1).sum() / cur.shape[0])
            if abs(prev - err) < tolerance:
                break
            prev = err
    return cur, r_all, t_all


# ---- files: the PLY layer behind compat/trimesh (host side, numpy) ---------------------------------------------------------------
class PointCloud:
    """trimesh.PointCloud as the reference's evaluation uses it: `.vertices` (float64 [N,3], numpy), optional `.colors`
    (uint8 [N,3]) and `.export(path)`, which writes a binary little-endian PLY."""

    def __init__(self, vertices, colors=None, normals=None):
        self.vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
        self.colors = None if colors is None else np.asarray(colors)[:, :3].astype(np.uint8).reshape(-1, 3)
        if self.colors is not None and len(self.colors) != len(self.vertices):
            raise ValueError("PointCloud: %d colours for %d vertices" % (len(self.colors), len(self.vertices)))
        self.normals = normals

    @property
    def normals(self):
        """float64 [N,3] or None; set by the caller or by `to_mesh`, which keeps the oriented normals it meshed with"""
        return self._normals

    @normals.setter
    def normals(self, value):
        self._normals = None if value is None else np.asarray(value, np.float64).reshape(-1, 3)
        if self._normals is not None and len(self._normals) != len(self.vertices):
            raise ValueError("PointCloud: %d normals for %d vertices" % (len(self._normals), len(self.vertices)))

    def to_mesh(self, device="cuda", **kw):
        """The cloud as a surface, on the GPU (r3g.recon).  Without `.normals`: the reference's `mesh_pointcloud(points, **kw)`,
        which estimates and orients its own.  With `.normals` (taken as oriented): `reconstruct(points, normals, **kw)`
        followed by `trim`; trim_quantile (default 0.025) is taken out of kw.  -> Mesh"""
        from . import recon
        p = torch.from_numpy(np.ascontiguousarray(self.vertices, np.float32)).to(device)
        if self.normals is None:
            return recon.mesh_pointcloud(p, **kw)
        quantile = kw.pop("trim_quantile", 0.025)
        nr = torch.from_numpy(np.ascontiguousarray(self.normals, np.float32)).to(device)
        mesh, densities, info = recon.reconstruct(p, nr, **kw)
        out = recon.trim(mesh, densities, quantile)
        out.metadata["recon"] = {k: info[k] for k in ("depth", "level", "residual", "usable")}
        return out

    def dbscan(self, eps=0.05, min_samples=10, device="cuda"):
        """`dbscan` of the vertices on the GPU -> (labels int32 [N] numpy, report dict)"""
        p = torch.from_numpy(np.ascontiguousarray(self.vertices, np.float32)).to(device)
        labels, report = dbscan(p, eps, min_samples)
        return labels.cpu().numpy(), report

    def largest_cluster(self, eps=0.05, min_samples=10, device="cuda"):
        """The reference's filter_dbscan as a PointCloud: the rows of the largest DBSCAN cluster (vertices, colours and normals),
        all rows when there is no cluster"""
        labels, report = self.dbscan(eps, min_samples, device)
        keep = np.ones(len(labels), bool) if report["n_clusters"] == 0 else labels == report["largest"]
        return PointCloud(self.vertices[keep], None if self.colors is None else self.colors[keep],
                          None if self.normals is None else self.normals[keep])

    def fit_plane(self, iterations=2000, threshold=0.05, device="cuda", **kw):
        """r3g.plane.fit_floor of the vertices on the GPU (the reference's floor-plane choice among PCA, RANSAC and total least
        squares) -> its dict with normal [3], point [1,3] and mask [N] as numpy arrays"""
        from . import plane
        p = torch.from_numpy(np.ascontiguousarray(self.vertices, np.float32)).to(device)
        fit = plane.fit_floor(p, iterations, threshold, **kw)
        return dict(fit, normal=fit["normal"].cpu().numpy(), point=fit["point"].cpu().numpy(), mask=fit["mask"].cpu().numpy())

    def export(self, path=None, file_type="ply"):
        if file_type != "ply" or (path is not None and not str(path).lower().endswith(".ply")):
            raise ValueError("PointCloud.export writes PLY only")
        data = save_ply(None, self.vertices, self.colors)
        if path is not None:
            with open(path, "wb") as fh:
                fh.write(data)
        return data


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def save_ply(path, vertices, colors=None, binary=True):
    """vertices [N,3] (written as float32) and optional uint8 colours [N,3] as a PLY with one `vertex` element, binary
    little-endian or ascii -> the bytes (also written to `path` unless it is None)"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    c = None if colors is None else np.asarray(colors).astype(np.uint8).reshape(-1, 3)
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % len(v),
            "property float x", "property float y", "property float z"]
    if c is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head = ("\n".join(head + ["end_header"]) + "\n").encode("ascii")
    if binary:
        rec = np.zeros(len(v), dtype=[("v", "<f4", 3)] + ([("c", "u1", 3)] if c is not None else []))
        rec["v"] = v
        if c is not None:
            rec["c"] = c
        body = rec.tobytes()
    else:
        rows = []
        for i in range(len(v)):
            row = " ".join(repr(float(x)) for x in v[i])
            rows.append(row + (" %d %d %d" % tuple(c[i]) if c is not None else ""))
        body = ("\n".join(rows) + ("\n" if rows else "")).encode("ascii")
    data = head + body
    if path is not None:
        with open(path, "wb") as fh:
            fh.write(data)
    return data


def load_ply(data):
    """A PLY file (path or bytes), ascii or binary little-endian -> PointCloud of its `vertex` element's x y z and, when all
    three are there, red green blue.  Other properties, and every other element (faces), are ignored."""
    if isinstance(data, str):
        with open(data, "rb") as fh:
            data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("not a PLY file")
    body = data.find(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w or w[0] == "comment":
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements:
            elements[-1][2].append(w[1:])
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("PLY format %r is not supported (ascii and binary_little_endian are)" % fmt)
    cols = None
    tokens = data[body:].split() if fmt == "ascii" else None
    pos = 0 if fmt == "ascii" else body
    for name, count, props in elements:
        scalar = all(p[0] != "list" for p in props)
        if name == "vertex":
            if not scalar:
                raise ValueError("PLY: list property in the vertex element")
            names = [p[1] for p in props]
            if fmt == "ascii":
                tab = np.array(tokens[pos:pos + count * len(names)], dtype=np.float64).reshape(count, len(names))
                cols = {n: tab[:, i] for i, n in enumerate(names)}
            else:
                dt = np.dtype([(p[1], "<" + _PLY_TYPES[p[0]]) for p in props])
                tab = np.frombuffer(data, dt, count, pos)
                cols = {n: tab[n] for n in names}
            break                                           # nothing after the vertices is needed
        if fmt == "ascii":                                  # skip an element that precedes the vertices
            for _ in range(count):
                for p in props:
                    pos += 1 + int(tokens[pos]) if p[0] == "list" else 1
        elif scalar:
            pos += count * sum(np.dtype(_PLY_TYPES[p[0]]).itemsize for p in props)
        else:
            for _ in range(count):
                for p in props:
                    if p[0] == "list":
                        n = int(np.frombuffer(data, "<" + _PLY_TYPES[p[1]], 1, pos)[0])
                        pos += np.dtype(_PLY_TYPES[p[1]]).itemsize + n * np.dtype(_PLY_TYPES[p[2]]).itemsize
                    else:
                        pos += np.dtype(_PLY_TYPES[p[0]]).itemsize
    if cols is None or not all(a in cols for a in "xyz"):
        raise ValueError("PLY: no vertex element with x y z")
    v = np.stack([np.asarray(cols[a], np.float64) for a in "xyz"], 1)
    c = None
    if all(a in cols for a in ("red", "green", "blue")):
        c = np.stack([np.asarray(cols[a]).astype(np.uint8) for a in ("red", "green", "blue")], 1)
    return PointCloud(v, c)
