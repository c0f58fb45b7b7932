"""Hierarchical volume decoding: the planner of include/r3g.h's r3g_hier_* entry points, without a model.

    levels(256)                                   -> [64, 128, 256]
    count = select(coarse, level, band, finest)   # mask + rank table stay in the context
    idx = indices(count, device)                  # ascending int32 linear indices of the fine lattice
    fine = merge(coarse, values)                  # values at idx, the floor parent everywhere else
    grid, stats = decode(field_fn, R, level, band)   # the level loop over any callable field_fn(idx, R_l) -> values

The algorithm is defined in DESIGN.md ("Hierarchical volume decoding"); `decode` with the geo decoder as field_fn is what
r3g_grid_query_hier does in one call (r3g.model.ShapeModel.grid_query_hier).  Tensors are torch CUDA tensors.
"""
import ctypes

import torch

from . import ffi as _l

DEFAULT_BAND = 0.95
DEFAULT_MIN_RESOLUTION = 63


def levels(R, min_resolution=DEFAULT_MIN_RESOLUTION):
    """resolutions of the levels, coarsest first: halve while the value is even and its half is >= min_resolution"""
    R = int(R)
    out = [R]
    while out[-1] % 2 == 0 and out[-1] // 2 >= min_resolution:
        out.append(out[-1] // 2)
    return out[::-1]


def _ctx(t, ctx):
    return ctx if ctx is not None else _l.context(t.device.index or 0)


def _check_grid(coarse):
    if not isinstance(coarse, torch.Tensor) or coarse.ndim != 3 or len(set(coarse.shape)) != 1:
        raise ValueError("the coarse grid must be a cubic 3D torch tensor")
    if not coarse.is_cuda:
        raise ValueError("r3g.hier needs a CUDA(HIP) tensor: the product has no CPU path")
    if coarse.dtype != torch.float32 or not coarse.is_contiguous():
        raise ValueError("the coarse grid must be contiguous float32")


def select(coarse, level, band=DEFAULT_BAND, is_finest=True, ctx=None):
    """number of points of the (2n-1)^3 lattice that the next level has to evaluate; the mask stays in the context"""
    _check_grid(coarse)
    n = ctypes.c_int64()
    with torch.cuda.device(coarse.device):
        _l.check(_l.lib().r3g_hier_select(_ctx(coarse, ctx), coarse.data_ptr(), coarse.shape[0], float(level), float(band),
                                          int(bool(is_finest)), ctypes.byref(n), _l.stream_ptr()))
    return int(n.value)


def indices(count, device, ctx=None):
    """the preceding select's points: ascending int32 linear indices (i * n + j) * n + k, n = 2 n_coarse - 1"""
    device = torch.device(device)
    idx = torch.empty((int(count),), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _l.check(_l.lib().r3g_hier_indices(ctx if ctx is not None else _l.context(device.index or 0),
                                           idx.data_ptr() if count else None, _l.stream_ptr()))
    return idx


def merge(coarse, values, ctx=None):
    """the fine grid of the preceding select: `values` (in the order of `indices`) at its points, the floor parent elsewhere"""
    _check_grid(coarse)
    n = 2 * coarse.shape[0] - 1
    values = values.to(coarse.device, torch.float32).contiguous()
    fine = torch.empty((n, n, n), dtype=torch.float32, device=coarse.device)
    with torch.cuda.device(coarse.device):
        _l.check(_l.lib().r3g_hier_merge(_ctx(coarse, ctx), coarse.data_ptr(), values.data_ptr() if values.numel() else None,
                                         fine.data_ptr(), _l.stream_ptr()))
    return fine


def decode(field_fn, R, level, band=DEFAULT_BAND, min_resolution=DEFAULT_MIN_RESOLUTION, device="cuda", ctx=None):
    """The level loop with `field_fn(idx, R_l) -> float32 values` standing in for the decoder (idx: ascending int32 linear
    indices into the (R_l + 1)^3 lattice, on `device`).  Returns the (R+1)^3 grid and
    {"levels", "evaluated_per_level", "evaluated", "dense_points"}."""
    device = torch.device(device)
    lv = levels(R, min_resolution)
    n0 = lv[0] + 1
    grid = field_fn(torch.arange(n0 ** 3, dtype=torch.int32, device=device), lv[0]).to(torch.float32).reshape(n0, n0, n0).contiguous()
    per_level = [n0 ** 3]
    for li in range(1, len(lv)):
        count = select(grid, level, band, li == len(lv) - 1, ctx)
        idx = indices(count, device, ctx)
        values = field_fn(idx, lv[li]) if count else torch.empty((0,), dtype=torch.float32, device=device)
        if values.shape != (count,):
            raise ValueError("field_fn returned %s values for %d points" % (tuple(values.shape), count))
        grid = merge(grid, values, ctx)
        per_level.append(count)
    return grid, {"levels": lv, "evaluated_per_level": per_level, "evaluated": sum(per_level), "dense_points": (R + 1) ** 3}
