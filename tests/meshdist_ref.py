"""Mesh distance: the float64 oracle (brute force over every face in numpy) and the fixtures the CPU and GPU tests share.

DIST_TOL: the distance tolerance, float32 product against this oracle, RELATIVE TO THE FIXTURE'S EXTENT (largest side of the
bounding box of mesh and points together).  Measured as DESIGN.md section 5 says: the largest |d32 - d64| / extent of the
host twin (tests/emu_meshdist.brute) over all CPU fixtures of tests/test_meshdist_cpu.py; the tolerance is four times that.
"""
import numpy as np


DIST_ERR_MEASURED = 4.196e-8     # soup 3.09e-8, small+span 1.74e-8, sphere 4.196e-8 (tests/test_meshdist_cpu.py prints them)
DIST_TOL = 4 * DIST_ERR_MEASURED


def _segment(p, a, b):
    ab, ap = b - a, p - a
    den = (ab * ab).sum(1)
    t = np.clip(np.divide((ap * ab).sum(1), den, out=np.zeros_like(den), where=den > 0), 0.0, 1.0)
    return np.linalg.norm(ap - t[:, None] * ab, axis=1)


def point_triangle_distance(p, tri):
    """float64 distance of points p [N,3] to triangles tri [N,3,3], degenerate ones included: the minimum over the three
    edges and, where the least-squares projection onto the plane falls inside, that point.  The 2x2 normal equations are
    solved with two steps of iterative refinement: mesh_metrics.point_triangle_distance (Ericson's closed form, which
    tests/test_meshdist_cpu.py holds this against on well-shaped triangles) loses 1 / sin^2 of the smallest angle and is
    3e-6 off on the soup's sliver even in float64."""
    p = np.asarray(p, np.float64)
    a, b, c = (np.asarray(tri, np.float64)[:, k] for k in range(3))
    best = np.minimum(np.minimum(_segment(p, a, b), _segment(p, b, c)), _segment(p, a, c))
    ab, ac, ap = b - a, c - a, p - a
    g11, g12, g22 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
    det = g11 * g22 - g12 * g12
    ok = det > 0
    inv = np.divide(1.0, det, out=np.zeros_like(det), where=ok)
    v = np.zeros(len(p))
    w = np.zeros(len(p))
    for _ in range(3):
        r = ap - v[:, None] * ab - w[:, None] * ac
        e1, e2 = (ab * r).sum(1), (ac * r).sum(1)
        v = v + (g22 * e1 - g12 * e2) * inv
        w = w + (g11 * e2 - g12 * e1) * inv
    inside = ok & (v >= 0) & (w >= 0) & (v + w <= 1)
    plane = np.linalg.norm(ap - v[:, None] * ab - w[:, None] * ac, axis=1)
    return np.where(inside, np.minimum(best, plane), best)


def oracle(points, verts, faces, chunk=128):
    """float64 distance of every point to the mesh -> (dist [N], face [N]: the lowest index at the minimum).
    Every face is a candidate; the exact point-triangle distance (point_triangle_distance above, float64) is only
    evaluated for the faces whose bounding sphere reaches as near as the nearest centroid (a float64 bound with a margin, so
    no face that could hold the minimum is left out).  Faces with a non-finite vertex take no part."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    tri = np.asarray(verts, np.float64)[np.asarray(faces)]
    use = np.flatnonzero(np.isfinite(tri).all(axis=(1, 2)))
    tri = tri[use]
    cen = tri.mean(1)
    rad = np.linalg.norm(tri - cen[:, None], axis=2).max(1)
    dist = np.empty(len(p))
    face = np.empty(len(p), np.int64)
    for s in range(0, len(p), chunk):
        q = p[s:s + chunk]
        dc = np.linalg.norm(q[:, None] - cen[None], axis=2)                 # the centroid is a point of the face
        cand = dc - rad[None] <= dc.min(1, keepdims=True) * (1 + 1e-9) + 1e-300
        qi, fi = np.nonzero(cand)
        d = np.full(cand.shape, np.inf)
        d[qi, fi] = point_triangle_distance(q[qi], tri[fi])
        j = d.argmin(1)
        dist[s:s + chunk] = d[np.arange(len(q)), j]
        face[s:s + chunk] = use[j]
    return dist, face


def extent(*arrays):
    pts = np.concatenate([np.asarray(a, np.float64).reshape(-1, 3) for a in arrays])
    pts = pts[np.isfinite(pts).all(1)]
    return float((pts.max(0) - pts.min(0)).max())


def soup(seed=7):
    """400 triangles in [0, 3]^3: 393 small random ones, 5 that span the box, a sliver and a point-triangle
    -> (verts float32 [1200,3], faces int32 [400,3])"""
    rng = np.random.default_rng(seed)
    c = rng.random((393, 1, 3)) * 2.6 + 0.2
    tri = c + (rng.random((393, 3, 3)) - 0.5) * 0.4
    span = np.array([[[0, 0, 0], [3, 3, 0.1], [0.2, 3, 3]],
                     [[3, 0, 0], [0, 3, 3], [3, 3, 2.9]],
                     [[0, 3, 0], [3, 0, 3], [0.1, 0.1, 3]],
                     [[0, 0, 3], [3, 3, 3], [3, 0, 0.3]],
                     [[1.5, 0, 0], [1.5, 3, 0], [1.4, 1.5, 3]]], np.float64)
    sliver = np.array([[[0.5, 0.5, 2.5], [2.5, 0.6, 2.4], [1.5, 0.55 + 1e-6, 2.45]]])
    point = np.full((1, 3, 3), 1.25)
    tri = np.concatenate([tri, span, sliver, point]).astype(np.float32)
    return tri.reshape(-1, 3), np.arange(1200, dtype=np.int32).reshape(400, 3)


def soup_points(n_inside=300, n_outside=100, seed=11):
    """points inside the soup's box and up to three box sizes outside it -> float32 [n,3]"""
    rng = np.random.default_rng(seed)
    inside = rng.random((n_inside, 3)) * 3.0
    outside = rng.random((n_outside, 3)) * 21.0 - 9.0          # [-9, 12]: three box sizes either way
    return np.concatenate([inside, outside]).astype(np.float32)


def many_points(n, seed=5):
    """n points, three quarters inside the soup's box and the rest around it -> float32 [n,3]"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * 3.0
    far = rng.random(n) < 0.25
    p[far] = rng.random((int(far.sum()), 3)) * 21.0 - 9.0
    return p.astype(np.float32)


def small_plus_span(seed=3):
    """2000 small triangles in the unit cube plus one that spans it -> (verts float32, faces int32 [2001,3])"""
    rng = np.random.default_rng(seed)
    c = rng.random((2000, 1, 3)) * 0.96 + 0.02
    tri = c + (rng.random((2000, 3, 3)) - 0.5) * 0.02
    tri = np.concatenate([tri, np.array([[[0, 0, 0], [1, 1, 0], [0, 1, 1]]], np.float64)]).astype(np.float32)
    return tri.reshape(-1, 3), np.arange(6003, dtype=np.int32).reshape(2001, 3)


def sphere_volume(c, n=65, centre=32):
    """c - rho^2 on an n^3 lattice (c = 400 is golden A of mc_volumes), level 0.5"""
    idx = np.indices((n, n, n)).astype(np.int64) - centre
    return (c - (idx ** 2).sum(0)).astype(np.float32)


def sphere_mesh_host(c, n=65, centre=32):
    """the level-0.5 surface of sphere_volume by the oracle's marching cubes (the CPU stand-in for the product's)"""
    from oracle import mc as omc
    v, f = omc.marching_cubes(sphere_volume(c, n, centre), 0.5)
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def sphere_points(v441, f441, n_near, n_far, seed=2):
    """n_near points of the 441 sphere's surface (face centroids) and n_far points up to two box sizes outside the 400 one"""
    rng = np.random.default_rng(seed)
    near = np.asarray(v441, np.float64)[np.asarray(f441)[rng.integers(0, len(f441), n_near)]].mean(1)
    far = (rng.random((n_far, 3)) * 5 - 2) * 40 + 12          # the 400 sphere's box is [12, 52]^3
    return np.concatenate([near, far]).astype(np.float32)


_FIXTURES = None


def cpu_fixtures():
    """the CPU fixtures DIST_ERR_MEASURED is taken over -> [(name, verts, faces, points)] (built once)"""
    global _FIXTURES
    if _FIXTURES is None:
        rng = np.random.default_rng(1)
        sv, sf = soup()
        pv, pf = small_plus_span()
        a, fa = sphere_mesh_host(400)
        b, fb = sphere_mesh_host(441)
        _FIXTURES = [("soup", sv, sf, soup_points()),
                     ("small+span", pv, pf, (rng.random((400, 3)) * 1.6 - 0.3).astype(np.float32)),
                     ("sphere", a, fa, sphere_points(b, fb, 300, 300))]
    return _FIXTURES
