"""Hole filling on the GPU: boundary loops and the faces that close them (include/r3g.h "mesh fill").

`boundary_loops` chains the boundary half-edges of the mate table of r3g.meshtopo into loops; `fill_holes` appends the faces
that close every loop of at most `max_loop` edges -- a fan from the loop's first vertex, or a fan around a new centroid vertex --
by the kernels of csrc/meshfill_kernels.hip.  Everything is a pure function of the faces (and, for the centroids, of the
vertices).  Boundary half-edges that lie on no simple loop (pinch vertices, inconsistently wound neighbours, edges beside a
non-manifold vertex) are counted as `tangled` and left alone; run `meshtopo.fix_winding` first where the winding is in doubt.

Difference from trimesh.repair.fill_holes: trimesh closes triangular and quadrilateral holes only and picks its own quad
diagonal; this closes any simple loop up to max_loop and cuts a quad from the loop's first vertex (compat/trimesh/repair.py
therefore defaults to max_loop=4).  Out of scope: welding vertices, repairing non-manifold edges, vertex attributes of new vertices.
"""
import ctypes

import torch

from . import ffi, meshtopo
from .meshdist import _mesh_args

REPORT_FIELDS = ("boundary", "loops", "tangled", "filled", "oversize", "longest", "loop_edges", "faces_added", "verts_added",
                 "rounds", "max_loop", "mode", "n_faces", "n_verts")
MODES = {"fan": 0, "centroid": 1}


def _plan(verts, faces, n_verts, max_loop, mode):
    """r3g_meshfill_plan on the shared context of the mesh's device (the caller holds ffi.device_lock) -> (v, f, report dict)"""
    if mode not in MODES:
        raise ValueError("mode must be 'fan' or 'centroid'")
    if verts is None:
        f, nv = meshtopo._faces_only(faces, n_verts)
        v, vp = None, ctypes.c_void_p(0)
    else:
        v, f = _mesh_args(verts, faces)
        nv, vp = v.shape[0], ctypes.c_void_p(v.data_ptr())
    dev = f.device.index or 0
    raw = (ctypes.c_int64 * 16)()
    with torch.cuda.device(f.device):
        ffi.check(ffi.lib().r3g_meshfill_plan(ffi.context(dev), vp, nv, ctypes.c_void_p(f.data_ptr()), f.shape[0], int(max_loop),
                                              MODES[mode], raw, ffi.stream_ptr()))
    return v, f, {k: int(x) for k, x in zip(REPORT_FIELDS, raw)}


def boundary_loops(verts, faces, n_verts=None, max_loop=64):
    """every boundary loop of the mesh, ascending by its lowest half-edge id, each as its vertices in the direction of its
    boundary half-edges -> (loop_start int64 [loops + 1], loop_verts int32 [sum L], status int32 [loops]: 0 would be filled at
    `max_loop`, 1 oversize).  verts may be None (n_verts required)."""
    dev = faces.device.index or 0
    with ffi.device_lock(dev), torch.cuda.device(faces.device):
        _, f, rep = _plan(verts, faces, n_verts, max_loop, "fan")
        start = torch.empty(rep["loops"] + 1, dtype=torch.int64, device=f.device)
        lverts = torch.empty(rep["loop_edges"], dtype=torch.int32, device=f.device)
        status = torch.empty(rep["loops"], dtype=torch.int32, device=f.device)
        ffi.check(ffi.lib().r3g_meshfill_loops(ffi.context(dev), ctypes.c_void_p(start.data_ptr()), ctypes.c_void_p(lverts.data_ptr()),
                                               ctypes.c_void_p(status.data_ptr()), ffi.stream_ptr()))
    return start, lverts, status


def fill_holes(verts, faces, max_loop=64, mode="fan", n_verts=None):
    """trimesh.repair.fill_holes: close every simple boundary loop of at most max_loop edges -> (verts, faces, info).  verts
    and faces are new tensors, the input followed by what was added (mode "fan" adds no vertex; "centroid" adds one per filled
    loop); when nothing was added the arguments are returned as they are.  info = the plan's report (REPORT_FIELDS) plus
    "topology": r3g.meshtopo's report of the result, so info["topology"]["watertight"] answers trimesh's return value.
    verts may be None in mode "fan" (n_verts required)."""
    dev = faces.device.index or 0
    with ffi.device_lock(dev), torch.cuda.device(faces.device):
        v, f, rep = _plan(verts, faces, n_verts, max_loop, mode)
        nv = rep["n_verts"]
        if rep["faces_added"] == 0:
            out_v, out_f = verts, faces
        else:
            new_f = torch.empty((rep["faces_added"], 3), dtype=torch.int32, device=f.device)
            new_v = torch.empty((rep["verts_added"], 3), dtype=torch.float32, device=f.device)
            ffi.check(ffi.lib().r3g_meshfill_emit(ffi.context(dev), ctypes.c_void_p(new_f.data_ptr()),
                                                  ctypes.c_void_p(new_v.data_ptr() if rep["verts_added"] else 0), ffi.stream_ptr()))
            out_f = torch.cat([f, new_f])
            out_v = v if v is None or not rep["verts_added"] else torch.cat([v, new_v])
        topo = meshtopo.build(out_v, out_f, None if out_v is not None else nv)
    info = dict(rep)
    info["topology"] = topo
    return out_v, out_f, info
