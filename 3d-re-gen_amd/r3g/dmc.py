"""Dual marching cubes on the GPU (mc_algo="dmc"): one vertex per surface patch of a cell, two triangles per crossed
grid edge.  The semantics are this project's own, fixed to the bit in DESIGN.md section 4c (modelled on Nielson /
Wodniok dual marching cubes with the manifold rule; not pinned to upstream's `diso` extractor).

    verts, faces = dual_marching_cubes(grid, level)            # index space, columns (axis0, axis1, axis2)
    verts, faces = extract_mesh(grid, mc_level, R)             # the frame of upstream's DMCSurfaceExtractor
Inputs and outputs are torch CUDA tensors; the grid never leaves HBM.
"""
import numpy as np

from .mc import _extract


def _run(grid, level, manifold, xform, reverse, ctx=None):
    return _extract("r3g_dmc_count", "r3g_dmc_emit", "dmc", grid, level, manifold, xform, reverse, ctx)


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
