"""Mesh registration: a float64 numpy restatement written from DESIGN.md section 4h (brute-force closest points, SVD /
least-squares solves) and the fixtures the CPU and GPU tests share: the "bean" and its poses.

FIT_ERR_MEASURED: the error of the host twin's full fit (tests/emu_meshfit.fit: float32 closest points, the product's
solver) against the TRUE pose, measured on the cases of `CASES` with 1000 samples (tests/test_meshfit_cpu.py prints the
figures); the tolerance the twin and the device are held to is four times that (the margin is for float32 closest points:
another sampling or summation order moves the float32 roundings, not the method).
"""
import numpy as np

# (rotation error in degrees, translation error, relative scale error), the largest over CASES, measured with the twin
FIT_ERR_MEASURED = (7.92e-7, 5.28e-9, 9.25e-11)     # point10s, the 95 degree restart, point10s
FIT_TOL = tuple(4 * e for e in FIT_ERR_MEASURED)
# weighted rms distance after a fit that found the pose (the twin's largest over CASES) and its tolerance
RMS_MEASURED = 1.69e-8
RMS_TOL = 4 * RMS_MEASURED

AXIS = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
SHIFT = np.array([0.05, -0.03, 0.02])
# (name, deg, scale, method, iterations) of the full fits: the plane method from 10 and 25 degrees, the point method (which
# creeps along the surface: it gets its own cap) from 10 degrees with scale 1.05
CASES = [("plane10", 10.0, None, "plane", 30), ("plane25", 25.0, None, "plane", 30), ("point10s", 10.0, 1.05, "point", 400)]


def bean():
    """UV sphere, 16 latitude bands x 32 longitudes (two poles + 15 rings: 482 vertices, 960 faces, wound outward), each
    unit-sphere vertex (x, y, z) mapped to (x + 0.25 y^2, 0.7 y + 0.15 x z, 0.45 z + 0.2 x^2), rounded to float32.
    No symmetry.  -> (verts float32 [482,3], faces int32 [960,3])"""
    nb, nl = 16, 32
    pts = [(0.0, 0.0, 1.0)]
    for i in range(1, nb):
        th = np.pi * i / nb
        for j in range(nl):
            ph = 2 * np.pi * j / nl
            pts.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    pts.append((0.0, 0.0, -1.0))
    s = np.array(pts)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    v = np.stack([x + 0.25 * y * y, 0.7 * y + 0.15 * x * z, 0.45 * z + 0.2 * x * x], 1).astype(np.float32)
    ring = lambda i, j: 1 + (i - 1) * nl + (j % nl)          # noqa: E731  (ring i = 1..15)
    f = []
    for j in range(nl):
        f.append((0, ring(1, j), ring(1, j + 1)))
    for i in range(1, nb - 1):
        for j in range(nl):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    south = len(pts) - 1
    for j in range(nl):
        f.append((south, ring(nb - 1, j + 1), ring(nb - 1, j)))
    return v, np.array(f, np.int32)


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


def pose(deg, scale=None, axis=AXIS, shift=SHIFT):
    """4 x 4: rotation by deg about axis, scale, translation"""
    m = np.eye(4)
    m[:3, :3] = (1.0 if scale is None else scale) * rotation(axis, deg)
    m[:3, 3] = shift
    return m


def apply(m, p):
    return np.asarray(p, np.float64) @ m[:3, :3].T + m[:3, 3]


def source_points(m, n=1000, seed=0):
    """sample_surface samples of the bean moved by the inverse of m -> (points float32 [S,3], weights float32 [S]); fitting
    them onto the bean should give m back"""
    import torch
    from r3g import meshdist
    v, f = bean()
    pts, _, w = meshdist.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, seed)
    return apply(np.linalg.inv(m), pts.numpy().astype(np.float64)).astype(np.float32), w.numpy().astype(np.float32)


def pose_error(m, truth):
    """(rotation error in degrees, translation error, relative scale error) of m against truth"""
    sm, st = np.cbrt(np.linalg.det(m[:3, :3])), np.cbrt(np.linalg.det(truth[:3, :3]))
    r = (m[:3, :3] / sm) @ (truth[:3, :3] / st).T
    # the angle from the skew part (accurate near 0, where arccos of the trace is not) and the trace
    sk = 0.5 * np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    ang = np.degrees(np.arctan2(np.linalg.norm(sk), 0.5 * (np.trace(r) - 1.0)))
    return float(ang), float(np.linalg.norm(m[:3, 3] - truth[:3, 3])), float(abs(sm / st - 1.0))


def closest_points(p, verts, faces, chunk=256):
    """float64 brute force: for every point the closest point over ALL triangles (Ericson, Real-Time Collision Detection
    5.1.5, by regions) -> (q [N,3], dist [N], face [N])"""
    p = np.asarray(p, np.float64)
    tri = np.asarray(verts, np.float64)[np.asarray(faces)]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    ab, ac = b - a, c - a
    out_q, out_d, out_f = np.empty((len(p), 3)), np.empty(len(p)), np.empty(len(p), np.int64)
    dot = lambda x, y: (x * y).sum(-1)          # noqa: E731
    for s in range(0, len(p), chunk):
        pp = p[s:s + chunk, None, :]
        ap, bp, cp = pp - a, pp - b, pp - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        with np.errstate(divide="ignore", invalid="ignore"):
            den = va + vb + vc
            v, w = vb / den, vc / den
            q = a + v[..., None] * ab + w[..., None] * ac                                       # interior
            t = ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]
            q = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + t * (c - b), q)      # edge bc
            t = (d2 / (d2 - d6))[..., None]
            q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + t * ac, q)         # edge ac
            t = (d1 / (d1 - d3))[..., None]
            q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + t * ab, q)         # edge ab
        q = np.where(((d6 >= 0) & (d5 <= d6))[..., None], c, q)                                  # vertex c
        q = np.where(((d3 >= 0) & (d4 <= d3))[..., None], b, q)                                  # vertex b
        q = np.where(((d1 <= 0) & (d2 <= 0))[..., None], a, q)                                   # vertex a
        dist = np.linalg.norm(pp - q, axis=-1)
        j = dist.argmin(1)
        k = np.arange(len(j))
        out_q[s:s + chunk], out_d[s:s + chunk], out_f[s:s + chunk] = q[k, j], dist[k, j], j
    return out_q, out_d, out_f


def solve_point(p, q, w, with_scale):
    """weighted Umeyama by SVD: the similarity taking p onto q -> 4 x 4"""
    w = w / w.sum()
    mp, mq = (w[:, None] * p).sum(0), (w[:, None] * q).sum(0)
    pc, qc = p - mp, q - mq
    h = (w[:, None, None] * qc[:, :, None] * pc[:, None, :]).sum(0)            # sum w q~ p~^T
    u, sv, vt = np.linalg.svd(h)
    d = np.diag([1.0, 1.0, np.sign(np.linalg.det(u @ vt))])
    r = u @ d @ vt
    s = float((sv * np.diag(d)).sum() / (w * (pc * pc).sum(1)).sum()) if with_scale else 1.0
    m = np.eye(4)
    m[:3, :3] = s * r
    m[:3, 3] = mq - s * r @ mp
    return m


def solve_plane(p, q, n, w, with_scale):
    """one Gauss-Newton step of sum w (n . (q - (p + omega x p + tau + sigma p)))^2 by least squares -> 4 x 4 with the exact
    rotation exp([omega]x)"""
    j = np.concatenate([np.cross(p, n), n, (p * n).sum(1, keepdims=True)], 1)[:, :7 if with_scale else 6]
    r = (n * (q - p)).sum(1)
    sw = np.sqrt(w)
    x = np.linalg.lstsq(j * sw[:, None], r * sw, rcond=1e-12)[0]
    th = np.linalg.norm(x[:3])
    m = np.eye(4)
    m[:3, :3] = (1.0 + x[6] if with_scale else 1.0) * (rotation(x[:3], np.degrees(th)) if th > 0 else np.eye(3))
    m[:3, 3] = x[3:6]
    return m


def icp(points, weights, verts, faces, method="plane", with_scale=False, iterations=6, init=None):
    """the loop of DESIGN.md 4h in float64 throughout -> list of 4 x 4 matrices, one per iteration (the last is the result)"""
    p0 = np.asarray(points, np.float64)
    w = np.ones(len(p0)) if weights is None else np.asarray(weights, np.float64)
    v = np.asarray(verts, np.float64)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    fn = fn / np.linalg.norm(fn, axis=1, keepdims=True)
    cur = np.eye(4) if init is None else np.asarray(init, np.float64)
    out = []
    for _ in range(iterations):
        p = apply(cur, p0)
        q, _, face = closest_points(p, verts, faces)
        d = solve_plane(p, q, fn[face], w, with_scale) if method == "plane" else solve_point(p, q, w, with_scale)
        cur = d @ cur
        out.append(cur)
    return out
