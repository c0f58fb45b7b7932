"""Mesh topology on the GPU: edge adjacency, watertightness, winding and its repair (include/r3g.h "mesh topology", DESIGN.md
section 4i).

The primitive is `build`: the half-edge mate table, the bodies (faces joined through edges that exactly two faces share), the
winding parity of every face inside its body, and a report of counts and quantised volume / area, by the kernels of
csrc/meshtopo_kernels.hip.  All of it is a pure function of the faces (and, for volume and area, of the vertices): integer
atomics only, nothing depends on the order in which they land.  `fix_winding` and `fix_normals` rewrite the faces in place
(trimesh.repair's functions of the same names); `face_adjacency` and `broken_faces` are read off the mate table.

Filling holes is r3g.meshfill, on this module's mate table.  Out of scope: welding vertices, any
repair of non-manifold edges.
"""
import ctypes

import torch

from . import ffi
from .meshdist import _mesh_args

REPORT_FIELDS = ("usable", "skipped", "vref", "edges", "boundary", "clash", "nonmanifold", "bodies", "unorientable", "euler",
                 "nonfinite", "six_volume_q", "vol_scale", "two_area_q", "area_scale", "has_verts")


def _report(raw):
    """the int64 [16] report of include/r3g.h as a dict, with what follows from it: watertight, winding_consistent, and (when the
    vertices were given) volume and area as floats"""
    r = {k: int(x) for k, x in zip(REPORT_FIELDS, raw)}
    r["watertight"] = r["usable"] > 0 and r["boundary"] == 0 and r["nonmanifold"] == 0
    r["winding_consistent"] = r["clash"] == 0
    if r["has_verts"]:
        r["volume"] = r["six_volume_q"] / 2.0 ** r["vol_scale"] / 6.0
        r["area"] = r["two_area_q"] / 2.0 ** r["area_scale"] / 2.0
    return r


def _faces_only(faces, n_verts):
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise ValueError("mesh buffers must live on the GPU (there is no CPU path)")
    f = faces.detach().to(torch.int32).contiguous()
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("expected faces [F,3]")
    if n_verts is None:
        raise ValueError("n_verts is required when no vertices are given")
    return f, int(n_verts)


def build(verts, faces, n_verts=None):
    """r3g_meshtopo_build on the shared context of the mesh's device -> the report dict (`_report`).  verts may be None (then
    n_verts is required and the report holds no volume or area).  The state stays in the context until the next build or
    orient; hold ffi.device_lock(device) across build and mates / bodies."""
    if verts is None:
        f, nv = _faces_only(faces, n_verts)
        vp = ctypes.c_void_p(0)
    else:
        v, f = _mesh_args(verts, faces)
        nv, vp = v.shape[0], ctypes.c_void_p(v.data_ptr())
    dev = f.device.index or 0
    raw = (ctypes.c_int64 * 16)()
    with ffi.device_lock(dev), torch.cuda.device(f.device):
        ffi.check(ffi.lib().r3g_meshtopo_build(ffi.context(dev), vp, nv, ctypes.c_void_p(f.data_ptr()), f.shape[0], raw, ffi.stream_ptr()))
    return _report(raw)


def report(device=0):
    """the report of the last successful build or orient on the device's shared context"""
    raw = (ctypes.c_int64 * 16)()
    with ffi.device_lock(device):
        ffi.check(ffi.lib().r3g_meshtopo_report(ffi.context(device), raw))
    return _report(raw)


def _n_faces(device):
    raw = (ctypes.c_int64 * 16)()
    ffi.check(ffi.lib().r3g_meshtopo_report(ffi.context(device), raw))
    return int(raw[0]) + int(raw[1])


def mates(device=0):
    """mate int32 [F,3] of the last build on the device: the other half-edge of a deg = 2 edge, -1 boundary, -2 non-manifold,
    -3 half-edge of a skipped face"""
    with ffi.device_lock(device), torch.cuda.device(device):
        out = torch.empty((_n_faces(device), 3), dtype=torch.int32, device=torch.device("cuda", device))
        ffi.check(ffi.lib().r3g_meshtopo_mates(ffi.context(device), ctypes.c_void_p(out.data_ptr()), ffi.stream_ptr()))
    return out


def bodies(device=0):
    """(body int32 [F], flip uint8 [F]) of the last build on the device: the lowest face index of each face's body (-1: skipped
    face), and whether `fix_winding` would reverse the face"""
    with ffi.device_lock(device), torch.cuda.device(device):
        n = _n_faces(device)
        body = torch.empty(n, dtype=torch.int32, device=torch.device("cuda", device))
        flip = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", device))
        ffi.check(ffi.lib().r3g_meshtopo_bodies(ffi.context(device), ctypes.c_void_p(body.data_ptr()),
                                                ctypes.c_void_p(flip.data_ptr()), ffi.stream_ptr()))
    return body, flip


def face_adjacency(verts, faces, n_verts=None):
    """trimesh's face_adjacency: the face pairs of the deg = 2 edges -> int64 [M,2], each pair ascending, rows sorted (two faces
    that share more than one such edge appear once per edge)"""
    dev = faces.device.index or 0
    with ffi.device_lock(dev):
        build(verts, faces, n_verts)
        m = mates(dev).reshape(-1).long()
    h = torch.arange(m.shape[0], device=m.device)
    keep = m > h                         # every deg = 2 edge once, at its lower half-edge
    pairs = torch.stack([h[keep] // 3, m[keep] // 3], 1)
    pairs = torch.sort(pairs, dim=1).values
    if pairs.shape[0]:
        order = torch.argsort(pairs[:, 0] * (m.shape[0] // 3 + 1) + pairs[:, 1])
        pairs = pairs[order]
    return pairs


def broken_faces(verts, faces, n_verts=None):
    """trimesh.repair.broken_faces: the ascending indices of the usable faces with an edge that is not shared by exactly two
    faces (boundary or non-manifold) -> int64 [K]"""
    dev = faces.device.index or 0
    with ffi.device_lock(dev):
        build(verts, faces, n_verts)
        m = mates(dev)
    return torch.nonzero(((m == -1) | (m == -2)).any(1)).reshape(-1)


def _orient(verts, faces, outward, n_verts=None):
    if verts is None:
        f, nv = _faces_only(faces, n_verts)
        vp = ctypes.c_void_p(0)
    else:
        v, f = _mesh_args(verts, faces)
        nv, vp = v.shape[0], ctypes.c_void_p(v.data_ptr())
    dev = f.device.index or 0
    nfr, nbr = ctypes.c_int64(0), ctypes.c_int64(0)
    with ffi.device_lock(dev), torch.cuda.device(f.device):
        ffi.check(ffi.lib().r3g_meshtopo_orient(ffi.context(dev), vp, nv, ctypes.c_void_p(f.data_ptr()), f.shape[0], int(outward),
                                                ctypes.byref(nfr), ctypes.byref(nbr), ffi.stream_ptr()))
        rep = report(dev)
    return f, {"faces_reversed": nfr.value, "bodies_reversed": nbr.value, "report": rep}


def fix_winding(verts, faces, n_verts=None):
    """trimesh.repair.fix_winding: reverse faces ((v0, v1, v2) -> (v2, v1, v0)) until every orientable body is consistently
    wound; the lowest face of each body keeps its winding.  -> (faces, info): `faces` is the int32 tensor that was rewritten --
    the argument itself, IN PLACE, when it is a contiguous int32 CUDA tensor, otherwise a converted copy; info =
    dict(faces_reversed, bodies_reversed, report: of the result).  verts may be None (n_verts required)."""
    return _orient(verts, faces, 0, n_verts)


def fix_normals(verts, faces, multibody=False):
    """trimesh.repair.fix_normals: `fix_winding`, then make the normals point outward: with multibody every orientable body of
    negative volume is reversed as a whole, without it every orientable body if the volume of the whole mesh is negative.
    Unorientable bodies are never touched.  -> (faces, info) as `fix_winding`."""
    return _orient(verts, faces, 1 if multibody else 2)
