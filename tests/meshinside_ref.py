"""Point in mesh: the numpy float64 restatement of DESIGN.md section 4g and the fixtures the CPU and GPU tests share.

`crossings` is written from the text of section 4g, not from csrc/meshinside_core.h: projection, canonical edge direction,
edge function, usable, covered, above.  Every difference and product is one float64 operation on the float32 inputs, so its
counts equal the product's exactly.  (Which (point, face) pairs are evaluated at all is decided by the definition's own
bounding-box condition; that only saves time.)

IOU_TOL: tolerance of volume_iou of the 400 and 441 spheres at n = 32 against volume(A) / volume(B) of the two meshes
(mesh_metrics.signed_volume): measured here on the CPU with this restatement (tests/test_meshinside_cpu.py prints it), times two.
"""
import numpy as np

IOU_ERR_MEASURED = 4.009e-3     # |iou - volume(A) / volume(B)| = |0.859527 - 0.863535|, spheres 400 / 441, n = 32, any axis
IOU_TOL = 2 * IOU_ERR_MEASURED
NC_MIN = 0.99                   # normal consistency of the two concentric spheres: the restatement gives 0.9996 both ways on the CPU


def _before(P, Q, ip, iq):
    """P precedes Q in the lexicographic order on the float values (u, v, w), the vertex index last"""
    r = ip < iq
    for k in (2, 1, 0):
        r = np.where(P[:, k] != Q[:, k], P[:, k] < Q[:, k], r)
    return r


def _edge(P, Q, ip, iq, x):
    """E(x) of the undirected edge {P, Q} along its canonical direction U -> V, and whether P -> Q runs against it"""
    fwd = _before(P, Q, ip, iq)
    U = np.where(fwd[:, None], P, Q).astype(np.float64)
    V = np.where(fwd[:, None], Q, P).astype(np.float64)
    x = x.astype(np.float64)
    e = (V[:, 0] - U[:, 0]) * (x[:, 1] - U[:, 1]) - (V[:, 1] - U[:, 1]) * (x[:, 0] - U[:, 0])
    return e, ~fwd


def project(a, axis):
    return np.asarray(a, np.float32).reshape(-1, 3)[:, [(axis + 1) % 3, (axis + 2) % 3, axis]]


def usable_faces(verts, faces, axis):
    """-> (tri float32 [F,3,3] in (u, v, w), usable bool [F], skipped = faces with a non-finite vertex)"""
    f = np.asarray(faces).reshape(-1, 3)
    v = project(verts, axis)
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("face index outside [0, %d)" % len(v))
    tri = v[f]
    fin = np.isfinite(tri).all(axis=(1, 2))
    ok = fin.copy()
    t = np.where(fin[:, None, None], tri, np.float32(0))
    for k in range(3):
        e, _ = _edge(t[:, k], t[:, (k + 1) % 3], f[:, k], f[:, (k + 1) % 3], t[:, (k + 2) % 3])
        ok &= e != 0
    return tri, ok, int((~fin).sum())


def _crossed(p, tri, idx):
    """p [M,3] (u, v, w) float32 inside the closed box of tri [M,3,3]'s projection, idx [M,3] -> crossed bool [M]"""
    A, B, C = tri[:, 0], tri[:, 1], tri[:, 2]
    eab, fab = _edge(A, B, idx[:, 0], idx[:, 1], p)
    oab, _ = _edge(A, B, idx[:, 0], idx[:, 1], C)
    ebc, fbc = _edge(B, C, idx[:, 1], idx[:, 2], p)
    obc, _ = _edge(B, C, idx[:, 1], idx[:, 2], A)
    eca, fca = _edge(C, A, idx[:, 2], idx[:, 0], p)
    oca, _ = _edge(C, A, idx[:, 2], idx[:, 0], B)
    covered = ((eab >= 0) == (oab > 0)) & ((ebc >= 0) == (obc > 0)) & ((eca >= 0) == (oca > 0))
    D = np.where(fab, -oab, oab)
    eab, ebc, eca = np.where(fab, -eab, eab), np.where(fbc, -ebc, ebc), np.where(fca, -eca, eca)
    N = ebc * A[:, 2].astype(np.float64) + eca * B[:, 2].astype(np.float64) + eab * C[:, 2].astype(np.float64)
    pd = p[:, 2].astype(np.float64) * D
    return covered & np.where(D > 0, N > pd, N < pd)


def crossings(points, verts, faces, axis=2, chunk=512):
    """-> (count int32 [N], skipped): the number of usable faces the ray from each point in the +axis direction crosses;
    -1 for a point with a non-finite coordinate"""
    f = np.asarray(faces).reshape(-1, 3)
    tri, ok, skipped = usable_faces(verts, f, axis)
    p = project(points, axis)
    good = np.isfinite(p).all(1)
    count = np.where(good, 0, -1).astype(np.int32)
    use = np.flatnonzero(ok)
    pid = np.flatnonzero(good)
    if not len(use) or not len(pid):
        return count, skipped
    pid = pid[np.argsort(p[pid, 0], kind="stable")]
    pu = p[pid, 0]
    for s in range(0, len(use), chunk):
        fi = use[s:s + chunk]
        t = tri[fi]
        first = np.searchsorted(pu, t[:, :, 0].min(1), "left")
        last = np.searchsorted(pu, t[:, :, 0].max(1), "right")
        n = last - first
        k = np.repeat(np.arange(len(fi)), n)
        j = pid[np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + first[k]]
        inv = (p[j, 1] >= t[k, :, 1].min(1)) & (p[j, 1] <= t[k, :, 1].max(1))
        k, j = k[inv], j[inv]
        hit = _crossed(p[j], t[k], f[fi][k])
        np.add.at(count, j[hit], 1)
    return count, skipped


def contains(points, verts, faces, axes=(2,)):
    """parity on one axis, or the majority of three -> inside bool [N], or (inside, share of points where all three agree)"""
    par = []
    for a in axes:
        c = crossings(points, verts, faces, a)[0]
        par.append((c > 0) & (c % 2 == 1))
    if len(par) == 1:
        return par[0]
    votes = np.sum(par, axis=0)
    agree = (votes == 0) | (votes == len(par))
    return votes * 2 > len(par), float(agree.mean()) if len(agree) else 1.0


def lattice(lo, hi, n):
    """cell centres lo + (i + 1/2) / n * (hi - lo) of an n^3 lattice, float64 rounded once to float32 -> [n^3, 3], x slowest"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ax = [(lo[a] + (np.arange(n, dtype=np.float64) + 0.5) / n * (hi[a] - lo[a])).astype(np.float32) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def volume_iou(a, b, n=128, axes=(2,)):
    """the restatement of r3g.meshinside.volume_iou on host arrays -> dict(iou, inter, union, in_a, in_b, volume_a, volume_b, n)"""
    va, vb = np.asarray(a[0], np.float32).reshape(-1, 3), np.asarray(b[0], np.float32).reshape(-1, 3)
    both = np.concatenate([va, vb])
    both = both[np.isfinite(both).all(1)]
    lo, hi = both.min(0), both.max(0)
    pts = lattice(lo, hi, n)
    ins = []
    for v, f in ((va, a[1]), (vb, b[1])):
        r = contains(pts, v, f, axes)
        ins.append(r if len(axes) == 1 else r[0])
    inter, union = int((ins[0] & ins[1]).sum()), int((ins[0] | ins[1]).sum())
    cell = float(np.prod((hi.astype(np.float64) - lo.astype(np.float64)) / n))
    return {"iou": inter / union if union else 0.0, "inter": inter, "union": union, "in_a": int(ins[0].sum()),
            "in_b": int(ins[1].sum()), "volume_a": int(ins[0].sum()) * cell, "volume_b": int(ins[1].sum()) * cell, "n": n}


def unit_normals(verts, faces):
    """float64 unit face normals [F,3] and whether the face has an area"""
    t = np.asarray(verts, np.float64)[np.asarray(faces)]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    l = np.linalg.norm(n, axis=1)
    ok = np.isfinite(l) & (l > 0)
    return n / np.where(ok, l, 1.0)[:, None], ok


def normal_direction(sample_face, weight, nearest_face, src, dst):
    """one direction of the normal consistency: abs = sum w |n_s . n_f| / W, signed = sum w (n_s . n_f) / W over the samples
    whose own face and nearest face both have an area"""
    ns, oks = unit_normals(*src)
    nf, okf = unit_normals(*dst)
    keep = (nearest_face >= 0) & oks[sample_face] & okf[np.maximum(nearest_face, 0)]
    d = (ns[sample_face[keep]] * nf[nearest_face[keep]]).sum(1)
    w = np.asarray(weight, np.float64)[keep]
    return {"abs": float((w * np.abs(d)).sum() / w.sum()), "signed": float((w * d).sum() / w.sum())}


# ---- fixtures ------------------------------------------------------------------------------------------------------
def cube():
    """the unit cube as 12 triangles, outward winding -> (verts float32 [8,3], faces int32 [12,3]); vertex i = (i&1, i>>1&1, i>>2&1)"""
    v = np.array([[i & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)], np.float32)
    f = np.array([[0, 2, 3], [0, 3, 1],      # z = 0
                  [4, 5, 7], [4, 7, 6],      # z = 1
                  [0, 1, 5], [0, 5, 4],      # y = 0
                  [2, 6, 7], [2, 7, 3],      # y = 1
                  [0, 4, 6], [0, 6, 2],      # x = 0
                  [1, 3, 7], [1, 7, 5]], np.int32)
    return v, f


def box_mesh(lo, hi):
    v, f = cube()
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return (lo + v * (hi - lo)).astype(np.float32), f


CUBE_LITERALS = [((0.5, 0.5, 0.5), 1), ((0.5, 0.5, -1.0), 2), ((0.5, 0.5, 2.0), 0), ((0.0, 0.0, -1.0), "even"), ((2.0, 0.5, 0.5), 0)]


def cube_literal_points(axis):
    """the literals of CUBE_LITERALS are written for axis 2 as (u, v, w); for another axis the coordinates rotate with it"""
    p = np.array([q for q, _ in CUBE_LITERALS], np.float32)
    out = np.empty_like(p)
    out[:, (axis + 1) % 3], out[:, (axis + 2) % 3], out[:, axis] = p[:, 0], p[:, 1], p[:, 2]
    return out


def sphere_lattice(n=4096, seed=3):
    """lattice points at spacing 1.5 over [11, 54.5]^3 (30^3 = 27 000: thousands of rays pass exactly through marching-cubes
    vertices and edges of the 65^3 sphere), cut to n of them -> float32 [n,3]"""
    ax = 11.0 + 1.5 * np.arange(30)
    p = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    if n < len(p):
        p = p[np.sort(np.random.default_rng(seed).choice(len(p), n, replace=False))]
    return p.astype(np.float32)


def plane(z=0.0, axis=2, n=4, size=1.0):
    """an n x n grid of squares (two triangles each) in the plane x[axis] = z, normal +axis -> (verts float32, faces int32)"""
    g = np.linspace(0.0, size, n + 1)
    uu, vv = np.meshgrid(g, g, indexing="ij")
    v = np.zeros(((n + 1) ** 2, 3))
    v[:, (axis + 1) % 3], v[:, (axis + 2) % 3], v[:, axis] = uu.ravel(), vv.ravel(), z
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None]).ravel()
    f = np.concatenate([np.stack([i, i + n + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + 1], 1)])
    return v.astype(np.float32), f.astype(np.int32)
