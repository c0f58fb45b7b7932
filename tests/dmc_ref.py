"""Numpy restatement of the dual-marching-cubes definition of DESIGN.md section 4c (test-only).

Written from the text of the definition, not from the kernels: the 256-case tables are derived here from the
face-joining rule, and the mesh is assembled with whole-array numpy operations.  Everything that the definition
fixes to the bit (double crossing points summed in ascending edge order, one rounding to float32, float32 diagonal
test with separately rounded operations) is done in that arithmetic.

    verts, faces, info = dual_marching_cubes(vol, level, manifold=True, xform=None)
"""
import numpy as np

R3G_ERR_LEVEL_RANGE = -10
R3G_ERR_NO_SURFACE = -11


class DmcError(Exception):
    def __init__(self, code):
        super().__init__("dmc error %d" % code)
        self.code = code


# ---- the cell: corners, edges, faces ----------------------------------------------------------------------------
def corner_offsets(c):
    return ((c >> 2) & 1, (c >> 1) & 1, c & 1)


def corner_number(d):
    return 4 * d[0] + 2 * d[1] + d[2]


def edge_corners(e):
    """-> (low corner, high corner, axis) of edge e = 4a + 2u + v"""
    a, u, v = e >> 2, (e >> 1) & 1, e & 1
    d = [0, 0, 0]
    d[(a + 1) % 3] = u
    d[(a + 2) % 3] = v
    lo = corner_number(d)
    d[a] = 1
    return lo, corner_number(d), a


def face_members(f):
    """face f = 2*axis + side -> (its 4 corners, its 4 edges)"""
    ax, side = f >> 1, f & 1
    corners = [c for c in range(8) if corner_offsets(c)[ax] == side]
    edges = [e for e in range(12) if edge_corners(e)[2] != ax and corner_offsets(edge_corners(e)[0])[ax] == side]
    return corners, edges


def case_patches(case):
    """-> (patch index of each of the 12 edges or -1, patch count, tunnelling face or -1)"""
    inside = [(case >> c) & 1 for c in range(8)]
    crossed = [inside[edge_corners(e)[0]] != inside[edge_corners(e)[1]] for e in range(12)]
    parent = list(range(12))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def join(x, y):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)

    ambiguous = []
    for f in range(6):
        corners, edges = face_members(f)
        ce = [e for e in edges if crossed[e]]
        assert len(ce) in (0, 2, 4)
        if len(ce) == 2:
            join(ce[0], ce[1])
        elif len(ce) == 4:
            ambiguous.append(f)
            ins = [c for c in corners if inside[c]]
            assert len(ins) == 2
            for c in ins:
                mine = [e for e in edges if c in edge_corners(e)[:2]]
                assert len(mine) == 2
                join(mine[0], mine[1])
    roots = sorted({find(e) for e in range(12) if crossed[e]})     # a root is its component's smallest edge
    patch = [roots.index(find(e)) if crossed[e] else -1 for e in range(12)]
    tunnel = [f for f in ambiguous if len({patch[e] for e in face_members(f)[1]}) == 1]
    assert len(tunnel) <= 1
    return patch, len(roots), (tunnel[0] if tunnel else -1), len(ambiguous)


_TABLES = None


def tables():
    """-> dict of int arrays: patch [256,12], count [256], tunnel [256], n_ambiguous [256]"""
    global _TABLES
    if _TABLES is None:
        rows = [case_patches(c) for c in range(256)]
        _TABLES = {"patch": np.array([r[0] for r in rows], np.int64), "count": np.array([r[1] for r in rows], np.int64),
                   "tunnel": np.array([r[2] for r in rows], np.int64), "n_ambiguous": np.array([r[3] for r in rows], np.int64)}
    return _TABLES


# ---- the mesh ------------------------------------------------------------------------------------------------
def _shift(a, off, shape):
    """view of a[off0: off0+shape0, ...]"""
    return a[off[0]:off[0] + shape[0], off[1]:off[1] + shape[1], off[2]:off[2] + shape[2]]


def dual_marching_cubes(vol, level, manifold=True, xform=None):
    """-> (float32 [V,3] in (axis0, axis1, axis2) order, int32 [F,3], info).  Raises DmcError with the C ABI's code.
    xform = (grid_size[3], bbox_size[3], bbox_min[3]) as for r3g_mc_emit, or None for index space."""
    G = np.ascontiguousarray(vol, np.float32)
    assert G.ndim == 3 and min(G.shape) >= 2
    level = float(level)
    T = tables()
    n = G.shape
    cs = tuple(x - 1 for x in n)
    Gd = G.astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = Gd > level
        if not np.isnan(Gd).any() and not ((Gd <= level).any() and (Gd >= level).any()):
            raise DmcError(R3G_ERR_LEVEL_RANGE)
    case = np.zeros(cs, np.int64)
    for c in range(8):
        case += _shift(s, corner_offsets(c), cs).astype(np.int64) << c
    active = (case != 0) & (case != 255)
    # manifold rule
    flip = np.zeros(cs, bool)
    if manifold:
        tun = T["tunnel"][case]
        for ax in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[ax] = slice(0, cs[ax] - 1)
            hi[ax] = slice(1, cs[ax])
            both = (tun[tuple(lo)] == 2 * ax + 1) & (tun[tuple(hi)] == 2 * ax)     # shared face: high side of lo, low side of hi
            flip[tuple(lo)] |= both
            flip[tuple(hi)] |= both
    eff = np.where(flip, case ^ 255, case)
    # vertices: one per patch of every active cell, by ascending cell, then patch
    lin = np.flatnonzero(active.reshape(-1))
    ci, cj, ck = np.unravel_index(lin, cs)
    cell = np.stack([ci, cj, ck], 1)
    eff_a = eff.reshape(-1)[lin]
    count = T["count"][eff_a]
    vbase_a = np.concatenate([[0], np.cumsum(count)])[:-1]
    vbase = np.full(int(np.prod(cs)), -1, np.int64)
    vbase[lin] = vbase_a
    acc = np.zeros((len(lin), 4, 3), np.float64)
    num = np.zeros((len(lin), 4), np.int64)
    with np.errstate(all="ignore"):
        for e in range(12):
            lo_c, hi_c, a = edge_corners(e)
            pe = T["patch"][eff_a, e]
            m = np.flatnonzero(pe >= 0)
            if len(m) == 0:
                continue
            plo = cell[m] + np.array(corner_offsets(lo_c))
            phi = cell[m] + np.array(corner_offsets(hi_c))
            va = Gd[plo[:, 0], plo[:, 1], plo[:, 2]]
            vb = Gd[phi[:, 0], phi[:, 1], phi[:, 2]]
            pt = plo.astype(np.float64)
            pt[:, a] = pt[:, a] + (level - va) / (vb - va)
            acc[m, pe[m]] = acc[m, pe[m]] + pt
            num[m, pe[m]] += 1
        keep = np.arange(4)[None, :] < count[:, None]
        assert np.all(num[keep] >= 3)
        pos = acc[keep] / num[keep][:, None].astype(np.float64)
        verts = pos.astype(np.float32)
        if xform is not None:
            gs, bs, bm = (np.asarray(x, np.float64).reshape(3) for x in xform)
            verts = (verts.astype(np.float64) / gs * bs + bm).astype(np.float32)
    # faces: one quad per crossed grid edge with four cells around it, by (linear index of p, axis)
    quads, keys, inside_p = [], [], []
    order = ((-1, -1), (0, -1), (0, 0), (-1, 0))
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        e_a = [0, 0, 0]
        e_a[a] = 1
        shp = list(n)
        shp[a] -= 1
        cr = _shift(s, (0, 0, 0), shp) != _shift(s, e_a, shp)
        ok = np.zeros(shp, bool)
        sl = [slice(None)] * 3
        sl[u] = slice(1, n[u] - 1)
        sl[v] = slice(1, n[v] - 1)
        ok[tuple(sl)] = True
        p = np.argwhere(cr & ok)
        if len(p) == 0:
            continue
        q = np.zeros((len(p), 4), np.int64)
        for m, (du, dv) in enumerate(order):
            c = p.copy()
            c[:, u] += du
            c[:, v] += dv
            cl = np.ravel_multi_index((c[:, 0], c[:, 1], c[:, 2]), cs)
            e = 4 * a + 2 * (-du) + (-dv)
            pch = T["patch"][eff.reshape(-1)[cl], e]
            assert np.all(pch >= 0) and np.all(vbase[cl] >= 0)
            q[:, m] = vbase[cl] + pch
        quads.append(q)
        keys.append(np.ravel_multi_index((p[:, 0], p[:, 1], p[:, 2]), n) * 3 + a)
        inside_p.append(s[p[:, 0], p[:, 1], p[:, 2]])
    info = {"n_flipped": int(flip.sum()), "n_active": int(len(lin)), "n_quads": 0}
    if not quads:
        raise DmcError(R3G_ERR_NO_SURFACE)
    q = np.concatenate(quads)
    srt = np.argsort(np.concatenate(keys), kind="stable")
    q = q[srt]
    ins = np.concatenate(inside_p)[srt]
    q = np.where(ins[:, None], q, q[:, ::-1])
    info["n_quads"] = int(len(q))
    with np.errstate(all="ignore"):
        P = verts[q]                                   # [Q,4,3] float32

        def d2(x, y):
            d = x - y                                  # float32, each operation rounded on its own
            return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        alt = d2(P[:, 1], P[:, 3]) < d2(P[:, 0], P[:, 2])
    t_alt = np.stack([q[:, [1, 2, 3]], q[:, [1, 3, 0]]], 1)
    t_def = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1)
    faces = np.where(alt[:, None, None], t_alt, t_def).reshape(-1, 3).astype(np.int32)
    return verts, faces, info


def upstream_frame(verts, grid_shape):
    """the frame r3g.dmc.extract_mesh returns: vertices / (n - 1) per axis (an xform with grid_size n-1, bbox_size 1,
    bbox_min 0 -- apply it through dual_marching_cubes(xform=...)), then minus the midpoint of their bounding box, float32"""
    v = np.asarray(verts, np.float32)
    mid = (np.float32(0.5) * (v.min(0) + v.max(0))).astype(np.float32)
    return (v - mid).astype(np.float32)


# ---- mesh properties (restatement-independent checks) -----------------------------------------------------------
def edge_face_counts(faces, n_verts):
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    key, cnt = np.unique(e[:, 0] * (n_verts + 1) + e[:, 1], return_counts=True)
    return key, cnt


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
