"""Dual marching cubes on the GPU (mc_algo="dmc"): one vertex per surface patch of a cell, two triangles per crossed
grid edge.  The semantics are this project's own, fixed to the bit in DESIGN.md section 4c (modelled on Nielson /
Wodniok dual marching cubes with the manifold rule; not pinned to upstream's `diso` extractor).

    verts, faces = dual_marching_cubes(grid, level)            # index space, columns (axis0, axis1, axis2)
    verts, faces = extract_mesh(grid, mc_level, R)             # the frame of upstream's DMCSurfaceExtractor
Inputs and outputs are torch CUDA tensors; the grid never leaves HBM.
"""
import ctypes

import numpy as np
import torch

from . import ffi as _l


def _stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(grid, level, manifold, xform, reverse, ctx=None):
    if not isinstance(grid, torch.Tensor) or grid.ndim != 3:
        raise ValueError("Input volume should be a 3D torch tensor.")
    if not grid.is_cuda:
        raise ValueError("r3g.dmc needs a CUDA(HIP) tensor: the product has no CPU path")
    if min(grid.shape) < 2:
        raise ValueError("Input array must be at least 2x2x2.")
    grid = grid.contiguous().float()
    dev = grid.device.index or 0
    with torch.cuda.device(dev):
        ctx = ctx if ctx is not None else _l.context(dev)
        L = _l.lib()
        nv, nf = ctypes.c_int64(), ctypes.c_int64()
        _l.check(L.r3g_dmc_count(ctx, grid.data_ptr(), grid.shape[0], grid.shape[1], grid.shape[2], float(level),
                                 int(bool(manifold)), ctypes.byref(nv), ctypes.byref(nf), _stream_ptr()))
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=grid.device)
        faces = torch.empty((nf.value, 3), dtype=torch.int32, device=grid.device)
        xf = None
        if xform is not None:
            xf = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64).reshape(3) for a in xform]))
        _l.check(L.r3g_dmc_emit(ctx, verts.data_ptr(), faces.data_ptr(), xf.ctypes.data if xf is not None else None,
                                int(bool(reverse)), _stream_ptr()))
    return verts, faces


def dual_marching_cubes(grid, level, manifold=True):
    """float32 [V,3] in index space, columns (axis0, axis1, axis2), and int32 [F,3] wound outward for a positive-inside
    field.  manifold=False is the cross-check form without the manifold rule.  LevelRangeError (a ValueError) /
    NoSurfaceError (a RuntimeError) as r3g.mc."""
    return _run(grid, level, manifold, None, False)


def extract_mesh(grid, mc_level=0.0, octree_resolution=None, ctx=None):
    """The frame of upstream's dual-marching-cubes extractor, as recalled (confidence medium):
    vertices divided by (n - 1) per axis, then moved so that the midpoint of the mesh's own bounding box is the origin;
    the bounding volume `box_v` is NOT applied.  `mc_level` is honoured (upstream extracts at a fixed 0)."""
    n = [int(s) for s in grid.shape]
    if octree_resolution is not None and any(s != int(octree_resolution) + 1 for s in n):
        raise ValueError("grid shape %s does not match octree_resolution %d" % (tuple(n), int(octree_resolution)))
    gs = np.array([s - 1 for s in n], np.float64)
    v, f = _run(grid, mc_level, True, (gs, np.ones(3), np.zeros(3)), False, ctx)
    v = v - 0.5 * (v.amin(0) + v.amax(0))
    return v, f
