"""Point cloud -> mesh on the GPU: Poisson surface reconstruction on a uniform lattice (include/r3g.h "Poisson surface",
DESIGN.md section 4l) and the reference's `mesh_pointcloud` built on it.

    mesh, densities, info = reconstruct(points, normals, depth=8)      # oriented normals in, Mesh + per-vertex density out
    mesh = trim(mesh, densities, 0.025)                                # drop the sparsely supported vertices
    mesh = mesh_pointcloud(points, depth=8)                            # the reference's whole function

The splat, the multigrid solve and the sampling are the kernels of csrc/recon_kernels.hip; the surface is r3g.mc / r3g.dmc on
the solved lattice.  The box, the level's division and the quantile are host arithmetic in float64.  CUDA tensors in; there
is no CPU path.
"""
import ctypes
import logging

import numpy as np
import torch

from . import ffi
from .mesh import Mesh

MIN_DEPTH, MAX_DEPTH = 2, 8
FIXED = 2.0 ** 30
# chi rises along the input normals (its gradient fits them), so with outward normals the inside is BELOW the level.  With
# reverse_faces = 1 both extractors wind their faces towards the rising side, i.e. along the input normals: outward normals give
# a positive Mesh.volume, inward ones a negative one (tests/test_recon_cpu.py holds both extractors to it on a sphere).
REVERSE_FACES = {"mc": True, "dmc": True}


def box_from_bounds(lo, hi, depth, scale=1.1):
    """The lattice's cube from the bounding box of the usable points -> (centre float64 [3], side, h).  The cube is centred on
    the box; its side is extent * max(scale, (n - 1) / max(n - 5, 1)) with extent the largest axis extent and n = 2^depth + 1, so
    every point lies at least two cells inside (at depth 2, whose lattice has four cells, the factor is 4 and the points lie one
    and a half cells inside: the nodes they touch are still interior).  depth outside [2, 8] or extent == 0: ValueError."""
    depth = int(depth)
    if not MIN_DEPTH <= depth <= MAX_DEPTH:
        raise ValueError("depth must lie in [%d, %d]" % (MIN_DEPTH, MAX_DEPTH))
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    n = 2 ** depth + 1
    extent = float((hi - lo).max())
    if not (extent > 0.0 and np.isfinite(extent)):
        raise ValueError("the usable points span no extent")
    side = extent * max(float(scale), (n - 1) / max(n - 5, 1))
    centre = 0.5 * (lo + hi)
    return centre, side, side / (n - 1)


def _pair(points, normals):
    from .cloud import _cloud_arg
    p, nr = _cloud_arg(points), _cloud_arg(normals, "normals")
    if p.shape != nr.shape:
        raise ValueError("points and normals differ in shape")
    return p, nr


def usable_mask(points, normals):
    """finite coordinates, finite non-zero normal"""
    return torch.isfinite(points).all(1) & torch.isfinite(normals).all(1) & (normals != 0).any(1)


def box(points, normals, depth, scale=1.1):
    """`box_from_bounds` of the usable points of a cloud on the GPU"""
    p, nr = _pair(points, normals)
    ok = usable_mask(p, nr)
    if not bool(ok.any()):
        raise ValueError("no usable point (finite coordinates, finite non-zero normal)")
    q = p[ok]
    return box_from_bounds(q.min(0).values.cpu().numpy(), q.max(0).values.cpu().numpy(), depth, scale)


def _ctx(t):
    dev = t.device.index or 0
    return dev, ffi.context(dev)


def splat(points, normals, depth, centre, side, want_channels=False):
    """r3g_recon_splat on the shared context of the points' device -> usable points (with want_channels: and a copy of the four
    channels, int64 [4, n, n, n]).  Hold ffi.device_lock(device) from here
    to the last solve / sample that uses it."""
    p, nr = _pair(points, normals)
    dev, ctx = _ctx(p)
    c = np.ascontiguousarray(centre, np.float64).reshape(3)
    used = ctypes.c_int64(0)
    n = 2 ** int(depth) + 1
    ch = torch.empty((4, n, n, n), dtype=torch.int64, device=p.device) if want_channels and MIN_DEPTH <= int(depth) <= MAX_DEPTH else None
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_recon_splat(ctx, ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(nr.data_ptr()), p.shape[0], int(depth),
                                            c.ctypes.data, float(side), ctypes.c_void_p(ch.data_ptr()) if ch is not None else None,
                                            ctypes.byref(used), ffi.stream_ptr()))
    return (used.value, ch) if want_channels else used.value


def solve(depth, device, cycles=10, want_b=False):
    """r3g_recon_solve on the last splat of `device` -> chi float32 [n, n, n] (and b, with want_b)"""
    device = torch.device(device)
    dev = device.index or 0
    n = 2 ** int(depth) + 1
    chi = torch.empty((n, n, n), dtype=torch.float32, device=device)
    b = torch.empty((n, n, n), dtype=torch.float32, device=device) if want_b else None
    with ffi.device_lock(dev), torch.cuda.device(device):
        ffi.check(ffi.lib().r3g_recon_solve(ffi.context(dev), int(cycles), ctypes.c_void_p(b.data_ptr()) if want_b else None,
                                            ctypes.c_void_p(chi.data_ptr()), ffi.stream_ptr()))
    return (chi, b) if want_b else chi


def sample(field, points, normals=None, out=None):
    """r3g_recon_sample: the density channel (field 0) or chi (field 1) of the last splat / solve, trilinearly at `points`
    -> (values float32 [N], fixed-point sum int, count).  With `normals` only usable points take part; others get NaN."""
    from .cloud import _cloud_arg
    p = _cloud_arg(points)
    nr = None if normals is None else _cloud_arg(normals, "normals")
    dev, ctx = _ctx(p)
    v = torch.empty(p.shape[0], dtype=torch.float32, device=p.device) if out is None else out
    s, cnt = ctypes.c_int64(0), ctypes.c_int64(0)
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_recon_sample(ctx, int(field), ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(nr.data_ptr()) if nr is not None else None,
                                             p.shape[0], ctypes.c_void_p(v.data_ptr()), ctypes.byref(s), ctypes.byref(cnt), ffi.stream_ptr()))
    return v, s.value, cnt.value


def level_from_sum(total, count):
    """the level: the fixed-point sum over the usable points, divided on the host"""
    return (total / FIXED) / count


def residual_ratio(chi, b, h):
    """max |b - Laplacian(chi)| over the interior nodes relative to max |b|, by torch in float64 (reported, never steering)"""
    x, r = chi.to(torch.float64), b.to(torch.float64)
    c = x[1:-1, 1:-1, 1:-1]
    lap = (x[:-2, 1:-1, 1:-1] + x[2:, 1:-1, 1:-1] + x[1:-1, :-2, 1:-1] + x[1:-1, 2:, 1:-1] + x[1:-1, 1:-1, :-2] + x[1:-1, 1:-1, 2:]
           - 6.0 * c) / (h * h)
    top = float(r.abs().max())
    return float((r[1:-1, 1:-1, 1:-1] - lap).abs().max()) / top if top > 0 else 0.0


def lattice_xform(depth, centre, side):
    """the marching-cubes output transform of the lattice: (grid_size, bbox_size, bbox_min), vertex = index / (n - 1) * side + lo"""
    n = 2 ** int(depth) + 1
    c = np.asarray(centre, np.float64).reshape(3)
    return np.full(3, float(n - 1)), np.full(3, float(side)), c - 0.5 * float(side)


def reconstruct(points, normals, depth=8, scale=1.1, cycles=10, mc_algo="mc"):
    """Poisson surface of an oriented cloud (Open3D's create_from_point_cloud_poisson, on a uniform lattice of 2^depth + 1
    nodes per axis: depth in [2, 8]) -> (Mesh on the device, densities float32 [V] on the device, info dict).
    The faces are wound along the input normals: outward normals give a positive `Mesh.volume`.  `densities` is the splatted
    point density at each vertex (what `trim` thresholds).  info: depth, n, centre, side, h, usable, level, cycles,
    residual (the final residual's max-norm relative to max |b|)."""
    from . import dmc, mc
    p, nr = _pair(points, normals)
    if mc_algo not in ("mc", "dmc"):
        raise ValueError("mc_algo must be 'mc' or 'dmc'")
    centre, side, h = box(p, nr, depth, scale)
    dev = p.device.index or 0
    with ffi.device_lock(dev):
        used = splat(p, nr, depth, centre, side)
        chi, b = solve(depth, p.device, cycles, want_b=True)
        _, total, count = sample(1, p, nr)
        level = level_from_sum(total, count)
        xf = lattice_xform(depth, centre, side)
        if mc_algo == "dmc":
            verts, faces = dmc._run(chi, level, True, xf, REVERSE_FACES["dmc"])
        else:
            verts, faces = mc._run(chi, level, False, xf, REVERSE_FACES["mc"])
        densities = sample(0, verts)[0]
    info = {"depth": int(depth), "n": 2 ** int(depth) + 1, "centre": centre, "side": side, "h": h, "usable": used, "level": level,
            "cycles": int(cycles), "residual": residual_ratio(chi, b, h), "mc_algo": mc_algo}
    return Mesh.from_device(verts, faces), densities, info


def trim(mesh, densities, quantile=0.025):
    """The reference's clean-up after Poisson (mesh_pointclouds.py:524-527): remove the vertices whose density lies below the
    `quantile` of all densities (numpy's linear quantile, on the host), the faces that used them, then unreferenced vertices.
    -> a new Mesh (host arrays)"""
    d = densities.detach().cpu().numpy() if torch.is_tensor(densities) else np.asarray(densities)
    d = np.asarray(d, np.float64).reshape(-1)
    out = Mesh(np.array(mesh.vertices), np.array(mesh.faces))
    out.metadata = dict(mesh.metadata)
    if len(d) != out.n_vertices:
        raise ValueError("trim: %d densities for %d vertices" % (len(d), out.n_vertices))
    if len(d):
        out.update_vertices(~(d < np.quantile(d, float(quantile))))
        out.remove_unreferenced_vertices()
    return out


def fill_pinched_loops(mesh, max_loop=64):
    """Close the boundary loops that `Mesh.fill_holes` leaves as tangled because two holes touch at a pinch vertex (trimesh's
    own fill_holes takes its cycles from the graph of boundary edges, so it closes such holes too).  On a consistently wound
    mesh: a boundary half-edge u -> v (a face's directed edge without its opposite) is followed, at a vertex with one outgoing
    boundary half-edge, by that one; at a pinch vertex with two fans of faces, by the outgoing half-edge of the OTHER fan (the
    hole lies between the two fans; the own fan's is found by turning about v from face to face).  A closed walk that meets a
    vertex twice (a hole that touches itself there, e.g. around a patch that hangs on one vertex) falls into simple cycles at
    that vertex, as a cycle basis of the boundary graph has them.  Every simple cycle of 3 .. max_loop edges is closed by a fan
    about its centroid (one new vertex, the float64 mean of the cycle's vertices in order; no diagonal, so no existing edge
    is duplicated).  Walks through a vertex with three or more fans are left.  Host arithmetic on the few edges concerned; in
    place -> cycles closed."""
    f = np.asarray(mesh.faces, np.int64)
    v = np.asarray(mesh.vertices, np.float64)
    if not len(f):
        return 0
    nv = len(v)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = e[:, 0] * nv + e[:, 1]
    half = e[~np.isin(key, e[:, 1] * nv + e[:, 0])]                      # directed edges without their opposite
    if not len(half):
        return 0
    out = {}
    for a, b in half.tolist():
        out.setdefault(a, []).append(b)
    pinch = [a for a, bs in out.items() if len(bs) > 1]
    third = {}                                                           # (a, b) -> c for the faces (a, b, c) about pinch vertices
    if pinch:
        for a, b, c in f[np.isin(f, pinch).any(1)].tolist():
            third[(a, b)], third[(b, c)], third[(c, a)] = c, a, b

    def own_fan_exit(u, w):
        """the outgoing boundary half-edge w -> x of the fan that holds u -> w"""
        x = third.get((u, w))
        for _ in range(4096):
            if x is None or (x, w) not in third:
                return x
            x = third[(x, w)]
        return None

    def follow(u, w):
        nxt = out.get(w, [])
        if len(nxt) == 1:
            return nxt[0]
        if len(nxt) == 2:
            own = own_fan_exit(u, w)
            return nxt[1] if nxt[0] == own else nxt[0] if nxt[1] == own else None
        return None

    seen, new_faces, new_verts = set(), [], []
    for a, b in half.tolist():
        if (a, b) in seen:
            continue
        walk, u, w, ok = [a], a, b, True
        while ok and (u, w) not in seen:
            seen.add((u, w))
            x = follow(u, w)
            if x is None:
                ok = False
            elif (w, x) == (a, b):                                       # about to repeat the first half-edge: closed
                break
            else:
                walk.append(w)
                u, w = w, x
        if not ok or (w, x) != (a, b):
            continue
        # a walk that meets a vertex twice (a hole that touches itself there) falls into simple cycles, as a cycle basis has them
        cycles, stack, at = [], [], {}
        for x in walk:
            if x in at:
                cycles.append(stack[at[x]:])
                for y in stack[at[x] + 1:]:
                    del at[y]
                del stack[at[x] + 1:]
            else:
                at[x] = len(stack)
                stack.append(x)
        cycles.append(stack)
        for loop in cycles:
            if not 3 <= len(loop) <= max_loop:
                continue
            c = nv + len(new_verts)
            new_verts.append(v[loop].sum(0) / len(loop))
            new_faces += [[loop[(i + 1) % len(loop)], loop[i], c] for i in range(len(loop))]
    if new_faces:
        mesh.vertices = np.concatenate([v, np.asarray(new_verts)])
        mesh.faces = np.concatenate([f, np.asarray(new_faces, np.int64)])
    return len(new_verts)


def _step(name, fn, log):
    """a repair step as upstream wraps it: a failure is reported and the step skipped"""
    try:
        return fn()
    except Exception as e:          # noqa: BLE001 -- upstream catches Exception around every step
        log.warning("    - %s failed: %s, continuing...", name, e)
        return None


def mesh_pointcloud(points, depth=8, remesh_percentage=0.5, k_normals=30, k_orient=100, trim_quantile=0.025, max_loop=64):
    """The reference's src/scene_optimization/mesh_pointclouds.py::mesh_pointcloud, step for step, without the file it writes:
    estimate_normals(k_normals) -> orient_normals (k_orient, upstream's 100, clamped to 31) -> reconstruct(depth) -> trim ->
    clean_and_remesh: fill_holes, fix_winding, fix_normals(multibody=True), the broken-face count (metadata["broken_faces"]),
    simplify_quadric_decimation(percent=remesh_percentage), process().  Upstream's default depth 9 is 8 here: the lattice is
    uniform and ends at 257^3.  fill_holes closes boundary loops of up to max_loop edges by a fan about the loop's centroid
    (trimesh's own closes triangles and quads only: max_loop=4): the simple loops by `Mesh.fill_holes`, then the loops through
    pinch vertices, which the trim leaves where two removed patches touch, by `fill_pinched_loops`.  Each repair step is wrapped as upstream wraps it: a failing step is logged and skipped.
    -> Mesh"""
    from . import cloud, meshtopo
    log = logging.getLogger(__name__)
    p = cloud._cloud_arg(points)
    if p.shape[0] == 0:
        raise ValueError("mesh_pointcloud: empty point cloud")
    normals = cloud.estimate_normals(p, k_normals)
    normals, _ = cloud.orient_normals(p, normals, k_orient)
    mesh, densities, info = reconstruct(p, normals, depth)
    mesh = trim(mesh, densities, trim_quantile)
    mesh.metadata["recon"] = {k: info[k] for k in ("depth", "level", "residual", "usable")}
    _step("Fill holes", lambda: (mesh.fill_holes(max_loop=max_loop, mode="centroid"), fill_pinched_loops(mesh, max_loop)), log)
    _step("Fix winding", lambda: mesh._orient(0), log)
    _step("Fix normals", lambda: mesh.fix_normals(multibody=True), log)
    broken = _step("Broken faces check", lambda: meshtopo.broken_faces(*mesh.device_buffers()) if not mesh.is_empty else [], log)
    if broken is not None:
        mesh.metadata["broken_faces"] = int(len(broken))
    simplified = _step("Simplification", lambda: mesh.simplify_quadric_decimation(percent=remesh_percentage), log)
    if simplified is not None:
        simplified.metadata = dict(mesh.metadata)
        mesh = simplified
    processed = _step("Mesh cleanup", lambda: mesh.process(validate=False), log)
    return processed if processed is not None else mesh
