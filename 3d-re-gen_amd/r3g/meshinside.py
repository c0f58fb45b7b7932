"""Point-in-mesh queries on the GPU: crossings, contains, signed distance, volumetric IoU and normal consistency
(include/r3g.h "point in mesh").

The primitive is `crossings`: for every query point the number of usable faces that the ray from the point in the +axis
direction crosses, by the column-grid kernels of csrc/meshinside_kernels.hip.  A point is inside when the count is odd.  The
count is a pure function of the mesh, the axis and the points (float64 arithmetic on the float32 inputs with one tie rule for
rays through shared edges and vertices), so a closed surface needs no jitter and no retries.  `contains` is the parity,
`signed_distance` puts that sign on r3g.meshdist.nearest, `volume_iou` counts lattice cells inside two meshes, and
`normal_consistency` compares the normals of nearest faces (it needs the distance query only).
"""
import ctypes

import torch

from . import ffi, meshdist
from .meshdist import _mesh_args

_CHUNK = 1 << 22          # lattice points per query of volume_iou


def _points(points):
    if not (torch.is_tensor(points) and points.is_cuda):
        raise ValueError("query points must live on the GPU (there is no CPU path)")
    p = points.detach().to(torch.float32).contiguous()
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("expected points [N,3]")
    return p


def _axes(axes):
    axes = tuple(int(a) for a in axes)
    if len(axes) not in (1, 3) or any(a not in (0, 1, 2) for a in axes):
        raise ValueError("axes: one axis or three, each in 0..2")
    return axes


def build(verts, faces, axis=2, resolution=None):
    """r3g_meshinside_build on the shared context of the mesh's device -> dict(resolution, pairs, skipped).
    The columns stay in the context until the next build; hold ffi.device_lock(device) across build and query."""
    v, f = _mesh_args(verts, faces)
    dev = v.device.index or 0
    res, pairs, skipped = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    with ffi.device_lock(dev), torch.cuda.device(v.device):
        ffi.check(ffi.lib().r3g_meshinside_build(ffi.context(dev), ctypes.c_void_p(v.data_ptr()), v.shape[0],
                                                 ctypes.c_void_p(f.data_ptr()), f.shape[0], int(axis), int(resolution or 0),
                                                 ctypes.byref(res), ctypes.byref(pairs), ctypes.byref(skipped), ffi.stream_ptr()))
    return {"resolution": res.value, "pairs": pairs.value, "skipped": skipped.value}


def query(points):
    """r3g_meshinside_query against the last build on the points' device -> count int32 [N]"""
    p = _points(points)
    dev = p.device.index or 0
    count = torch.empty(p.shape[0], dtype=torch.int32, device=p.device)
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_meshinside_query(ffi.context(dev), ctypes.c_void_p(p.data_ptr()), p.shape[0],
                                                 ctypes.c_void_p(count.data_ptr()), ffi.stream_ptr()))
    return count


def crossings(points, verts, faces, axis=2, resolution=None):
    """The number of usable faces the ray from each point in the +axis direction crosses -> int32 [N]; -1 for a point with a
    non-finite coordinate.  CUDA tensors only.  resolution: columns per projected axis (None: automatic); the result does not
    depend on it."""
    p = _points(points)
    with ffi.device_lock(p.device.index or 0):
        build(verts, faces, axis, resolution)
        return query(p)


def _parity(count):
    return (count > 0) & ((count & 1) == 1)


def contains(points, verts, faces, axes=(2,), resolution=None):
    """Is each point inside the mesh?  One axis: the parity of `crossings` -> bool [N].  Three axes: the majority of the three
    parities -> (bool [N], agreement), agreement = the share of points on which all three parities agree (1.0 on a closed
    surface, lower on an open one: a watertightness indicator; 1.0 for N = 0).  Non-finite points give False."""
    axes = _axes(axes)
    par = [_parity(crossings(points, verts, faces, a, resolution)) for a in axes]
    if len(par) == 1:
        return par[0]
    votes = par[0].to(torch.int32) + par[1].to(torch.int32) + par[2].to(torch.int32)
    agree = (votes == 0) | (votes == 3)
    return votes >= 2, float(agree.double().mean()) if agree.numel() else 1.0


def _inside(points, verts, faces, axes, resolution=None):
    r = contains(points, verts, faces, axes, resolution)
    return r if len(axes) == 1 else r[0]


def signed_distance(points, verts, faces, axes=(2,)):
    """Signed distance of every point to the mesh -> (sd float32 [N], face int32 [N]): r3g.meshdist.nearest's distance,
    NEGATED where `contains` is true -- the SDF convention, negative inside.  (trimesh.proximity.signed_distance uses the
    opposite sign, positive inside.)  face is nearest's face index; a non-finite point gets (NaN, -1)."""
    axes = _axes(axes)
    p = _points(points)
    with ffi.device_lock(p.device.index or 0):
        d, face = meshdist.nearest(p, verts, faces)
        inside = _inside(p, verts, faces, axes)
    return torch.where(inside, -d, d), face


def lattice_axis(lo, hi, n, device):
    """cell centres lo + (i + 1/2) / n * (hi - lo) along one axis: float64 on the device, rounded once to float32 -> [n]"""
    i = torch.arange(n, dtype=torch.float64, device=device)
    return (float(lo) + (i + 0.5) / n * (float(hi) - float(lo))).to(torch.float32)


def volume_iou(a, b, n=128, axes=(2,)):
    """Volumetric IoU of two meshes a = (verts, faces), b = (verts, faces) (CUDA tensors) on an n^3 lattice of cell centres
    lo + (i + 1/2) / n * (hi - lo) over the union bounding box of the finite vertices (float64, rounded once to float32,
    generated on the device).
    -> dict(iou = inter / union (0.0 when union == 0), inter, union, in_a, in_b: integer cell counts; volume_a, volume_b:
    counts times the cell volume; n; query_ms: the queries, HIP events)"""
    axes = _axes(axes)
    av, af = _mesh_args(*a)
    bv, bf = _mesh_args(*b)
    n = int(n)
    if n < 1 or n > 1024:
        raise ValueError("volume_iou: n outside [1, 1024]")
    both = torch.cat([av, bv])
    both = both[torch.isfinite(both).all(1)]
    if both.shape[0] == 0:
        raise ValueError("volume_iou: no finite vertex")
    lo, hi = both.min(0).values.double().tolist(), both.max(0).values.double().tolist()
    dev = av.device
    ax = [lattice_axis(lo[k], hi[k], n, dev) for k in range(3)]
    slabs = max(1, _CHUNK // (n * n))
    inside = [torch.empty(n * n * n, dtype=torch.bool, device=dev) for _ in range(2)]
    ms = 0.0
    with ffi.device_lock(dev.index or 0), torch.cuda.device(dev):
        for (v, f), out in zip(((av, af), (bv, bf)), inside):
            votes = torch.zeros(n * n * n, dtype=torch.int8, device=dev)
            for axis in axes:
                build(v, f, axis)
                for s in range(0, n, slabs):
                    xs = ax[0][s:s + slabs]
                    pts = torch.stack(torch.meshgrid(xs, ax[1], ax[2], indexing="ij"), -1).reshape(-1, 3)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    c = query(pts)
                    e1.record()
                    e1.synchronize()
                    ms += e0.elapsed_time(e1)
                    votes[s * n * n:s * n * n + c.shape[0]] += _parity(c).to(torch.int8)
            out.copy_(votes * 2 > len(axes))
    in_a, in_b = int(inside[0].sum()), int(inside[1].sum())
    inter, union = int((inside[0] & inside[1]).sum()), int((inside[0] | inside[1]).sum())
    cell = 1.0
    for k in range(3):
        cell *= (hi[k] - lo[k]) / n
    return {"iou": inter / union if union else 0.0, "inter": inter, "union": union, "in_a": in_a, "in_b": in_b,
            "volume_a": in_a * cell, "volume_b": in_b * cell, "n": n, "query_ms": ms}


def unit_normals(verts, faces):
    """float64 unit face normals [F,3] and a mask of the faces that have an area (torch ops, any device)"""
    t = verts.to(torch.float64)[faces.long()]
    nrm = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    length = nrm.norm(dim=1)
    ok = torch.isfinite(length) & (length > 0)
    return nrm / torch.where(ok, length, torch.ones_like(length))[:, None], ok


def normal_scores(sample_face, weight, nearest_face, src, dst):
    """One direction of the normal consistency (pure tensor arithmetic on any device): with n_s the unit normal of the
    sample's own face of src and n_f the unit normal of its nearest face of dst,
        abs = sum w |n_s . n_f| / W        signed = sum w (n_s . n_f) / W
    over the samples whose own face and nearest face both have an area (W = their weight).  -> dict(abs, signed)"""
    ns, oks = unit_normals(*src)
    nf, okf = unit_normals(*dst)
    sample_face, nearest_face = sample_face.long(), nearest_face.long()
    keep = (nearest_face >= 0) & oks[sample_face] & okf[nearest_face.clamp(min=0)]
    d = (ns[sample_face[keep]] * nf[nearest_face[keep]]).sum(1)
    w = weight.to(torch.float64)[keep]
    tot = w.sum()
    return {"abs": float((w * d.abs()).sum() / tot), "signed": float((w * d).sum() / tot)}


def normal_consistency(a, b, samples=200000, seed=0):
    """Normal consistency of two meshes a = (verts, faces), b = (verts, faces) (CUDA tensors): `samples` area-weighted
    surface samples per direction (r3g.meshdist.sample_surface), each compared with the face r3g.meshdist.query returns.
    -> dict(ab, ba: `normal_scores`; abs, signed: the means of the two directions).  abs ignores the winding, signed does not."""
    out = {}
    for key, src, dst in (("ab", a, b), ("ba", b, a)):
        sv, sf = _mesh_args(*src)
        dv, df = _mesh_args(*dst)
        pts, fidx, w = meshdist.sample_surface(sv, sf, samples, seed)
        with ffi.device_lock(sv.device.index or 0):
            meshdist.build(dv, df)
            _, face = meshdist.query(pts)
        out[key] = normal_scores(fidx, w, face, (sv, sf), (dv, df))
    out["abs"] = 0.5 * (out["ab"]["abs"] + out["ba"]["abs"])
    out["signed"] = 0.5 * (out["ab"]["signed"] + out["ba"]["signed"])
    return out
