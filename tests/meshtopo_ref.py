"""numpy / scipy restatement of the mesh topology primitive and the fixtures of its tests.

Nothing here shares code with csrc/meshtopo_core.h: edges come from np.unique over sorted vertex pairs, bodies from
scipy.sparse.csgraph.connected_components, and the winding parity from the components of the signed double cover of the
face-adjacency graph (node (f, p) joins (g, p ^ clash)): a body is orientable iff (root, 0) and (root, 1) fall into different
components, and flip[f] = 1 iff (f, 1) lies in the component of (root, 0)."""
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


class BadIndex(ValueError):
    code = -2


def _six_vol(a, b, c):
    """det[a, b, c] expanded along b, float64, one operation per product and difference (the order csrc/meshtopo_core.h states)"""
    m0 = a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1]
    m1 = a[:, 0] * c[:, 2] - a[:, 2] * c[:, 0]
    m2 = a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0]
    return (b[:, 1] * m1 - b[:, 0] * m0) - b[:, 2] * m2


def _two_area(a, b, c):
    u, v = b - a, c - a
    n0 = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    n1 = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    n2 = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)


def scales(verts, faces, usable):
    """(s_vol, s_area) by the rule of section 4i: M = the largest finite |coordinate| of a referenced vertex, M < 2^e"""
    ref = np.unique(faces[usable])
    c = np.abs(np.asarray(verts, np.float32)[ref]).reshape(-1)
    c = c[np.isfinite(c)]
    bits = int(np.float32(c.max() if len(c) else 0.0).view(np.uint32))
    e = (bits >> 23) - 126
    return 30 - 3 * e, 29 - 2 * e


def _sorted_rows(pairs):
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))].astype(np.int64).reshape(-1, 2)


def build(verts, faces, n_verts=None):
    """-> dict(mate, body, flip, report, broken, adjacency, vol [F] and area [F] (float64 per face, 0 where it does not count),
    s_vol, s_area); report has the fields of the C report that do not depend on the quantisation, plus six_volume / two_area as
    exactly rounded float64 sums"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(verts) if verts is not None else int(n_verts)
    nf = len(f)
    if ((f < 0) | (f >= nv)).any():
        raise BadIndex("a face index lies outside [0, %d)" % nv)
    usable = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    h = (3 * np.flatnonzero(usable)[:, None] + np.arange(3)[None]).reshape(-1)          # half-edge ids of the usable faces
    a, b = f.reshape(-1)[h], f[h // 3, (h % 3 + 1) % 3]
    key = np.minimum(a, b) * nv + np.maximum(a, b)
    _, inv, deg = np.unique(key, return_inverse=True, return_counts=True)
    n_fwd = np.bincount(inv, weights=(a < b), minlength=len(deg)).astype(np.int64)
    mate = np.full(3 * nf, -3, np.int64)
    mate[h] = np.where(deg[inv] == 1, -1, -2)
    order = np.argsort(inv, kind="stable")
    two = order[deg[inv[order]] == 2].reshape(-1, 2)           # the two half-edges (positions in h) of every deg = 2 edge
    h1, h2 = h[two[:, 0]], h[two[:, 1]]
    mate[h1], mate[h2] = h2, h1
    clash = n_fwd[inv[two[:, 0]]] != 1
    # bodies and parity
    f1, f2 = h1 // 3, h2 // 3
    _, comp = connected_components(coo_matrix((np.ones(len(f1)), (f1, f2)), shape=(nf, nf)), directed=False)
    low = np.full(comp.max() + 1 if nf else 0, nf, np.int64)
    np.minimum.at(low, comp, np.arange(nf))
    body = np.where(usable, low[comp], -1)
    rows = np.concatenate([f1, f1 + nf])
    cols = np.concatenate([f2 + nf * clash, f2 + nf * (1 - clash)])
    _, cover = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(2 * nf, 2 * nf)), directed=False)
    root = np.where(usable, body, 0)
    orientable = cover[root] != cover[root + nf]
    flip = (usable & orientable & (cover[np.arange(nf) + nf] == cover[root])).astype(np.uint8)
    roots = np.flatnonzero(usable & (body == np.arange(nf)))
    rep = {"usable": int(usable.sum()), "skipped": int((~usable).sum()), "vref": int(len(np.unique(f[usable]))),
           "edges": int(len(deg)), "boundary": int((deg == 1).sum()), "clash": int(clash.sum()),
           "nonmanifold": int((deg >= 3).sum()), "bodies": int(len(roots)), "unorientable": int((~orientable[roots]).sum())}
    rep["euler"] = rep["vref"] - rep["edges"] + rep["usable"]
    out = {"mate": mate.reshape(nf, 3).astype(np.int32), "body": body.astype(np.int32), "flip": flip, "report": rep,
           "orientable": orientable,
           "broken": np.flatnonzero(((mate.reshape(nf, 3) == -1) | (mate.reshape(nf, 3) == -2)).any(1)),
           "adjacency": _sorted_rows(np.sort(np.stack([f1, f2], 1), axis=1))}      # one row per deg = 2 edge, as trimesh
    if verts is not None:
        v = np.asarray(verts, np.float32).astype(np.float64)
        counts = usable & np.isfinite(v[f]).all((1, 2))
        vol, area = np.zeros(nf), np.zeros(nf)
        t = v[f[counts]]
        with np.errstate(all="ignore"):
            vol[counts] = _six_vol(t[:, 0], t[:, 1], t[:, 2])
            area[counts] = _two_area(t[:, 0], t[:, 1], t[:, 2])
        rep["nonfinite"] = int((usable & ~counts).sum())
        rep["six_volume"], rep["two_area"] = math.fsum(vol), math.fsum(area)
        out["vol"], out["area"] = vol, area
        out["s_vol"], out["s_area"] = scales(verts, f, usable)
    return out


def body_volumes(st):
    """{body: exactly rounded float64 six-volume as `flip` would wind it}, and the number of faces that count, per body"""
    sign = 1.0 - 2.0 * st["flip"]
    vols, n = {}, {}
    for b in np.unique(st["body"][st["body"] >= 0]):
        sel = st["body"] == b
        vols[int(b)] = math.fsum(sign[sel] * st["vol"][sel])
        n[int(b)] = int(sel.sum())
    return vols, n


def orient(verts, faces, outward, n_verts=None):
    """-> (faces rewritten, faces_reversed, bodies_reversed) by the rule of section 4i, from float64 sums"""
    f = np.asarray(faces, np.int32).reshape(-1, 3).copy()
    st = build(verts, f, n_verts)
    rev = st["flip"].astype(bool)
    bodies = 0
    if outward:
        vols, _ = body_volumes(st)
        total = math.fsum(x for b, x in vols.items() if st["orientable"][b])     # the bodies that may be reversed
        for b, x in vols.items():
            if st["orientable"][b] and ((outward == 1 and x < 0) or (outward == 2 and total < 0)):
                rev ^= st["body"] == b
                bodies += 1
    f[rev] = f[rev][:, ::-1]
    return f, int(rev.sum()), bodies


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)


def cube():
    """the unit cube, 12 faces wound outward; vertex 4 x + 2 y + z"""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    quads = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    f = [t for q in quads for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])]
    return v, np.array(f, np.int32)


def cube_reversed(k):
    v, f = cube()
    f[k] = f[k, ::-1]
    return v, f


def shared_edge():
    """two tetrahedra that share the edge (0, 1): that edge has degree 4"""
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], np.float32)
    def tet(a, b, c, d):
        return [[a, c, b], [a, b, d], [b, c, d], [a, d, c]]
    return v, np.array(tet(0, 1, 2, 3) + tet(0, 1, 4, 5), np.int32)


def moebius(n=8):
    ang = 2 * np.pi * np.arange(n) / n
    half = ang / 2
    top = np.stack([(2 + 0.5 * np.cos(half)) * np.cos(ang), (2 + 0.5 * np.cos(half)) * np.sin(ang), 0.5 * np.sin(half)], 1)
    bot = np.stack([(2 - 0.5 * np.cos(half)) * np.cos(ang), (2 - 0.5 * np.cos(half)) * np.sin(ang), -0.5 * np.sin(half)], 1)
    v = np.concatenate([top, bot]).astype(np.float32)
    f = []
    for i in range(n):
        t0, b0 = i, n + i
        t1, b1 = (i + 1, n + i + 1) if i + 1 < n else (n, 0)          # the seam joins top to bottom
        f += [[t0, b0, t1], [b0, b1, t1]]
    return v, np.array(f, np.int32)


def torus(n=8, m=8):
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    a, b = 2 * np.pi * i / n, 2 * np.pi * j / m
    v = np.stack([(2 + np.cos(b)) * np.cos(a), (2 + np.cos(b)) * np.sin(a), np.sin(b)], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda p, q: (p % n) * m + (q % m)
    f = []
    for p in range(n):
        for q in range(m):
            f += [[idx(p, q), idx(p + 1, q), idx(p + 1, q + 1)], [idx(p, q), idx(p + 1, q + 1), idx(p, q + 1)]]
    return v, np.array(f, np.int32)


def ball(centre=(0, 0, 0), radius=1.0):
    """an octahedron subdivided once and pushed onto the sphere: 18 vertices, 32 faces, wound outward"""
    v = [np.array(p, np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    mid, out = {}, []
    def m(a, b):
        k = (min(a, b), max(a, b))
        if k not in mid:
            mid[k] = len(v)
            v.append((v[a] + v[b]) / 2)
        return mid[k]
    for a, b, c in f:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    v = np.array(v)
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * radius + np.asarray(centre, np.float64)
    return v.astype(np.float32), np.array(out, np.int32)


def two_balls(inner_radius=0.5):
    """two disjoint balls: radius 1 about the origin wound outward, radius inner_radius about (4, 0, 0) wound inward"""
    v1, f1 = ball((0, 0, 0), 1.0)
    v2, f2 = ball((4, 0, 0), inner_radius)
    return np.concatenate([v1, v2]), np.concatenate([f1, f2[:, ::-1] + len(v1)]).astype(np.int32)


def cube_and_moebius(cube_first=True):
    """the outward unit cube and a Moebius strip ten times the size lifted far along z, whose det-sum is large and negative:
    one orientable and one unorientable body.  The strip must weigh on no decision about the cube."""
    cv, cf = cube()
    mv, mf = moebius()
    mv = mv * np.float32(10) + np.array([0, 0, 40], np.float32)
    if moebius_det_sum(mv, mf) > 0:
        mf = mf[:, ::-1]
    if cube_first:
        return np.concatenate([cv, mv]), np.concatenate([cf, mf + len(cv)]).astype(np.int32)
    return np.concatenate([mv, cv]), np.concatenate([mf, cf + len(mv)]).astype(np.int32)


def moebius_det_sum(v, f):
    t = np.asarray(v, np.float64)[f]
    return float(_six_vol(t[:, 0], t[:, 1], t[:, 2]).sum())


def double_face():
    """a triangle and its exact reverse: two faces that share all three edges (three adjacency rows for one pair of faces)"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    return v, np.array([[0, 1, 2], [2, 1, 0]], np.int32)


def strip(n=4097):
    """a triangle strip of n faces, consistently wound, with every odd face then reversed"""
    i = np.arange(n)
    j = np.arange(n + 2)
    v = np.stack([j // 2, j % 2, np.zeros(n + 2)], 1).astype(np.float32)
    f = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1))
    f[1::2] = f[1::2, ::-1]
    return v, f.astype(np.int32)


_GOLDEN = {}


def golden_mesh(name):
    """the oracle's marching-cubes mesh of a golden volume of tests/mc_volumes.py (skimage's face order), built once"""
    if name not in _GOLDEN:
        from oracle import mc as omc
        import mc_volumes
        vol, level = mc_volumes.golden_volume(name)
        v, f = omc.marching_cubes(vol, level)
        _GOLDEN[name] = (np.asarray(v, np.float32), np.asarray(f, np.int32))
    return _GOLDEN[name]
