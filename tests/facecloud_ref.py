"""Face-to-cloud distance: the float64 restatement (a brute force over every point and every face in numpy, written from DESIGN.md
section 4p's text, not from the product's source), its torch form for autograd, and the fixtures the CPU and GPU tests share.

DIST_TOL: the distance tolerance, float32 product against this restatement, RELATIVE TO THE FIXTURE'S EXTENT (the largest side of the
bounding box of mesh and cloud together).  Measured as DESIGN.md section 5 says: the largest |sqrt(d2_32) - sqrt(d2_64)| / extent of
the host twin (tests/emu_facecloud.brute) over `cpu_fixtures()`; the tolerance is four times that
(tests/test_facecloud_cpu.py::test_twin_against_float64_distances prints each fixture's figure and asserts the constants).
GRAD_TOL: the same for the gradient: the largest |g_32 - g_64| / max |g_64| over the fixtures, on faces with a safe gap and weights
away from 0 and 1 (test_gradient_against_float64_autograd prints and asserts it)."""
import numpy as np

DIST_ERR_MEASURED = 6.547e-8     # blob 3.451e-9, partial 6.5466e-8, spans 3.073e-8, shell 3.606e-9
DIST_TOL = 4 * DIST_ERR_MEASURED
GRAD_ERR_MEASURED = 4.346e-6     # blob 1.490e-6 (46 faces), partial 4.3453e-6 (6), spans 9.880e-7 (39), shell 1.059e-7 (64)
GRAD_TOL = 4 * GRAD_ERR_MEASURED
GAP_CAP = 0.01               # at most this share of a fixture's faces may have a float64 gap below DIST_TOL


def _segment(p, a, b):
    """closest point of segment a b to p -> (d2, point, t); a == b gives the point a"""
    ab, ap = b - a, p - a
    den = (ab * ab).sum(-1)
    t = np.clip(np.divide((ap * ab).sum(-1), den, out=np.zeros_like(den), where=den > 0), 0.0, 1.0)
    r = a + t[..., None] * ab
    return ((p - r) ** 2).sum(-1), r, t


def point_triangle(p, tri):
    """float64: the closest point of triangles tri [..., 3, 3] to points p [..., 3] -> (d2, r, weights [..., 3]).  The minimum over
    the edges ab, bc, ac (which are all there is of a triangle without area) and, where the least-squares projection onto the plane
    falls strictly inside, that point; the 2 x 2 normal equations take three steps of iterative refinement (slivers)."""
    p = np.asarray(p, np.float64)
    tri = np.asarray(tri, np.float64)
    shape = np.broadcast_shapes(p.shape[:-1], tri.shape[:-2])
    p, tri = np.broadcast_to(p, shape + (3,)), np.broadcast_to(tri, shape + (3, 3))
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    zero = np.zeros(p.shape[:-1])
    d2, r, t = _segment(p, a, b)
    w = np.stack([1 - t, t, zero], -1)
    for (u, v, cols) in ((b, c, (1, 2)), (a, c, (0, 2))):
        e2, er, et = _segment(p, u, v)
        ew = np.zeros(p.shape[:-1] + (3,))
        ew[..., cols[0]], ew[..., cols[1]] = 1 - et, et
        m = e2 < d2
        d2, r, w = np.where(m, e2, d2), np.where(m[..., None], er, r), np.where(m[..., None], ew, w)
    ab, ac, ap = b - a, c - a, p - a
    g11, g12, g22 = (ab * ab).sum(-1), (ab * ac).sum(-1), (ac * ac).sum(-1)
    det = g11 * g22 - g12 * g12
    ok = det > 0
    inv = np.divide(1.0, det, out=np.zeros_like(det), where=ok)
    v, x = zero.copy(), zero.copy()
    for _ in range(3):
        q = ap - v[..., None] * ab - x[..., None] * ac
        e1, e2 = (ab * q).sum(-1), (ac * q).sum(-1)
        v, x = v + (g22 * e1 - g12 * e2) * inv, x + (g11 * e2 - g12 * e1) * inv
    inside = ok & (v > 0) & (x > 0) & (v + x < 1)
    ir = a + v[..., None] * ab + x[..., None] * ac
    i2 = ((p - ir) ** 2).sum(-1)
    m = inside & (i2 < d2)
    iw = np.stack([1 - v - x, v, x], -1)
    return np.where(m, i2, d2), np.where(m[..., None], ir, r), np.where(m[..., None], iw, w)


def usable_faces(verts, faces):
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    ok[ok] = np.isfinite(v[f[ok]]).all(axis=(1, 2))
    return ok


def oracle(points, verts, faces, chunk=64):
    """float64, every usable point against every face -> dict(dist2 [F], index [F] (the lowest index at the minimum; -1 and NaN for an
    unusable face), weights [F,3], diff [F,3], gap [F]: second-best DISTINCT distance minus the best, unsquared (inf with one
    distinct value), usable [F])"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    keep = np.flatnonzero(np.isfinite(p).all(1))
    q = p[keep]
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = usable_faces(v, f)
    F = len(f)
    out = {"dist2": np.full(F, np.nan), "index": np.full(F, -1, np.int64), "weights": np.zeros((F, 3)), "diff": np.zeros((F, 3)),
           "gap": np.full(F, np.inf), "usable": ok}
    use = np.flatnonzero(ok)
    for s in range(0, len(use), chunk):
        ids = use[s:s + chunk]
        tri = v[f[ids]]                                              # [c, 3, 3]
        d2, r, w = point_triangle(q[None, :, :], tri[:, None, :, :])     # [c, N]
        j = d2.argmin(1)                                             # the first, hence the lowest index, at the minimum
        rows = np.arange(len(ids))
        best = d2[rows, j]
        out["dist2"][ids], out["index"][ids] = best, keep[j]
        out["weights"][ids], out["diff"][ids] = w[rows, j], q[j] - r[rows, j]
        d = np.sqrt(d2)
        rest = np.where(d > np.sqrt(best)[:, None], d, np.inf).min(1)
        out["gap"][ids] = rest - np.sqrt(best)
    return out


def extent(*arrays):
    pts = np.concatenate([np.asarray(a, np.float64).reshape(-1, 3) for a in arrays])
    pts = pts[np.isfinite(pts).all(1)]
    return float((pts.max(0) - pts.min(0)).max())


def dist2_torch(verts, faces, points, index):
    """torch (float64 for autograd): the squared distance of point index[f] to face f, the minimum over the three edges and the
    plane's projection where it falls inside -> [F].  `index` is held constant, as the product holds it."""
    import torch
    a, b, c = (verts[faces[:, k]] for k in range(3))
    p = points[index]

    def seg(u, v):
        uv, up = v - u, p - u
        den = (uv * uv).sum(-1)
        t = torch.where(den > 0, (up * uv).sum(-1) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den)).clamp(0, 1)
        return ((up - t[:, None] * uv) ** 2).sum(-1)
    best = torch.minimum(torch.minimum(seg(a, b), seg(b, c)), seg(a, c))
    ab, ac, ap = b - a, c - a, p - a
    g11, g12, g22 = (ab * ab).sum(-1), (ab * ac).sum(-1), (ac * ac).sum(-1)
    det = g11 * g22 - g12 * g12
    safe = torch.where(det > 0, det, torch.ones_like(det))
    e1, e2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    v, w = (g22 * e1 - g12 * e2) / safe, (g11 * e2 - g12 * e1) / safe
    inside = (det > 0) & (v > 0) & (w > 0) & (v + w < 1)
    plane = ((ap - v[:, None] * ab - w[:, None] * ac) ** 2).sum(-1)
    return torch.where(inside, torch.minimum(best, plane), best)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
def grid_mesh(n, size=1.0, z=0.0, centre=(0.0, 0.0)):
    """a flat square plate of side `size` about `centre` at height z, meshed n x n -> (verts float32 [(n+1)^2, 3], faces int32 [2 n^2, 3])"""
    t = np.linspace(-0.5, 0.5, n + 1) * size
    x, y = np.meshgrid(t + centre[0], t + centre[1], indexing="xy")
    v = np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], 1).astype(np.float32)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + n + 1], 1)]).astype(np.int32)
    return v, f


def blob(n_faces, seed, scale=0.08, box=1.0):
    """n_faces small random triangles in [0, box]^3, as a soup with its own vertices"""
    rng = np.random.default_rng(seed)
    c = rng.random((n_faces, 1, 3)) * box
    tri = (c + (rng.random((n_faces, 3, 3)) - 0.5) * scale).astype(np.float32)
    return tri.reshape(-1, 3), np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


_FIXTURES = None


def cpu_fixtures():
    """the fixtures DIST_ERR_MEASURED is taken over -> [(name, verts, faces, points)] (built once).  None has deliberate ties:
      blob:     600 small triangles in the unit cube against 1500 points there
      partial:  the same kind of soup over [0, 3]^3 against a cloud that covers one corner of it, [0, 1]^3 (most faces lie outside
                the cloud's box: the stop rule's other-axes term and the far rings)
      spans:    300 small triangles, five that span the box, a sliver, a point-triangle and a segment-triangle against 1200 points
      shell:    a 12 x 12 plate above a noisy sheet of 2000 points (the pose fit's setting)"""
    global _FIXTURES
    if _FIXTURES is None:
        import meshdist_ref
        rng = np.random.default_rng(21)
        bv, bf = blob(600, 31)
        pv, pf = blob(500, 32, scale=0.3, box=3.0)
        sv, sf = meshdist_ref.soup()
        sv = sv.copy()
        sv[0:3] = np.array([[0.4, 0.4, 0.4], [1.9, 2.0, 2.1], [1.9, 2.0, 2.1]], np.float32)      # face 0 becomes a segment-triangle
        keep = np.r_[0:300, 393:400]
        plate_v, plate_f = grid_mesh(12, 1.0, 0.05)
        sheet = np.concatenate([rng.random((2000, 2)) * 0.8 - 0.4, rng.normal(0, 0.01, (2000, 1))], 1).astype(np.float32)
        _FIXTURES = [("blob", bv, bf, rng.random((1500, 3)).astype(np.float32)),
                     ("partial", pv, pf, rng.random((1200, 3)).astype(np.float32)),
                     ("spans", sv, sf[keep], (rng.random((1200, 3)) * 3.0).astype(np.float32)),
                     ("shell", plate_v, plate_f, sheet)]
    return _FIXTURES


def edge_cloud(n, seed=40):
    """n points in the unit cube; from two points on, the first two are its corners (the box is the unit cube, so a cell at resolution
    16 is 1/16 wide); from 63 on, point 5 is NaN and point 9 repeats point 8 -> float32 [n,3]"""
    rng = np.random.default_rng(seed + n)
    p = rng.random((n, 3)).astype(np.float32)
    if n == 1:
        p[0] = 0.5
    if n >= 2:
        p[0], p[1] = 0.0, 1.0
    if n >= 63:
        p[5] = np.nan
        p[9] = p[8]
    return p


EDGE_HUB = 40      # the vertex of edge_mesh() with 65 corners


def edge_mesh(seed=41):
    """257 faces over 200 vertices for the edges of the contract, the special ones first -> (verts float32 [200,3], faces int32 [257,3]).
    With the unit cube as the cloud's box and resolution 16:
      0  inside one cell                      1  a box of 16 x 4 x 1 = 64 cells (exactly kWideCells: narrow)
      2  a box of 13 x 5 x 1 = 65 cells (wide)  3  over the whole box and beyond        4  far outside the box
      5  a point-triangle (one vertex three times)   6  a segment-triangle              7  three collinear vertices
      8  a NaN vertex   9  a +inf vertex   10  a -inf vertex   11  index -1   12  index V
      13 .. 77  a fan of 65 faces about vertex EDGE_HUB (65 corners); vertex 41 has one corner, vertex 42 none
      78 .. 256 small random triangles over shared vertices, some of them outside the box"""
    rng = np.random.default_rng(seed)
    c = 1.0 / 16
    v = np.zeros((200, 3), np.float32)
    v[0:3] = [[0.51, 0.52, 0.53], [0.53, 0.51, 0.55], [0.52, 0.55, 0.51]]                     # cell (8, 8, 8)
    v[3:6] = [[0.01, 2.1 * c, 3.5 * c], [15.9 * c, 2.2 * c, 3.5 * c], [8.0 * c, 5.9 * c, 3.6 * c]]      # x cells 0..15, y 2..5, z 3
    v[6:9] = [[1.1 * c, 4.1 * c, 9.5 * c], [13.9 * c, 4.2 * c, 9.5 * c], [7.0 * c, 8.9 * c, 9.6 * c]]   # x cells 1..13, y 4..8, z 9
    v[9:12] = [[-0.5, -0.4, 0.3], [1.6, -0.3, 0.5], [0.4, 1.7, 0.45]]
    v[12:15] = [[7.0, 8.0, -9.0], [7.5, 8.0, -9.0], [7.0, 8.5, -9.5]]
    v[15] = [0.25, 0.75, 0.5]
    v[16:18] = [[0.1, 0.2, 0.3], [0.9, 0.8, 0.7]]
    v[18:21] = [[0.2, 0.2, 0.8], [0.4, 0.4, 0.8], [0.6, 0.6, 0.8]]
    v[21], v[22], v[23] = [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]
    v[24:27] = [[0.3, 0.3, 0.3], [0.35, 0.3, 0.3], [0.3, 0.35, 0.3]]
    v[EDGE_HUB] = [0.5, 0.5, 0.25]
    v[41], v[42] = [0.9, 0.1, 0.9], [0.1, 0.9, 0.1]
    ang = np.arange(66) * (2 * np.pi / 66)
    v[43:109] = np.stack([0.5 + 0.2 * np.cos(ang), 0.5 + 0.2 * np.sin(ang), 0.25 + 0.05 * np.sin(3 * ang)], 1)
    v[109:200] = rng.random((91, 3)) * 1.3 - 0.15
    f = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 15, 15], [16, 17, 17], [18, 19, 20],
         [24, 21, 25], [24, 25, 22], [23, 24, 25], [-1, 25, 26], [24, 200, 26]]
    f += [[EDGE_HUB, 43 + k, 44 + k] for k in range(65)]
    f[13][2] = 41                                                                            # vertex 41's one corner
    for _ in range(179):
        a = int(rng.integers(109, 200))
        near = np.argsort(((v[109:200] - v[a]) ** 2).sum(1))[1:12]                            # (small triangles: among a's neighbours)
        f.append([a] + (109 + rng.choice(near, 2, replace=False)).tolist())
    return v, np.asarray(f, np.int32)


_ORACLES = {}


def fixture_oracle(name):
    """`oracle` of a fixture, computed once and shared"""
    if name not in _ORACLES:
        _, v, f, p = next(x for x in cpu_fixtures() if x[0] == name)
        _ORACLES[name] = oracle(p, v, f)
    return _ORACLES[name]
