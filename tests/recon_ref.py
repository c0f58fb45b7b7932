"""numpy / scipy restatement of the Poisson surface's definitions, written from the text and not from
csrc/recon_core.h: the splat into int64 channels, the divergence, the trilinear sample and level, and the 7-point system the
solver approximates.  Test-only; also the clouds the CPU and GPU tests share."""
import numpy as np

F32 = np.float32
FIXED = 2.0 ** 30


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def nodes(depth):
    return 2 ** depth + 1


def usable(points, normals):
    p, n = np.asarray(points, F32), np.asarray(normals, F32)
    return np.isfinite(p).all(1) & np.isfinite(n).all(1) & (n != 0).any(1)


def box(points, normals, depth, scale=1.1):
    """centre, side, h in float64: the cube about the centre of the usable points' bounding box, side = extent * max(scale,
    (n - 1) / (n - 5))"""
    p = np.asarray(points, F32)[usable(points, normals)].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    n = nodes(depth)
    side = float((hi - lo).max()) * max(scale, (n - 1) / (n - 5) if n > 5 else 4.0)      # depth 2: four cells, factor 4
    return 0.5 * (lo + hi), side, side / (n - 1)


def _locate(p, depth, centre, side):
    """cells int [N,3] and fractions float32 [N,3] of finite points: t = (p - lo) * inv_h in float32"""
    n = nodes(depth)
    lo = (np.asarray(centre, np.float64) - 0.5 * side).astype(F32)
    inv_h = F32(1.0 / (side / (n - 1)))
    with np.errstate(over="ignore", invalid="ignore"):
        t = (p - lo) * inv_h
        cell = np.clip(np.floor(t), 0, n - 2).astype(F32)
        f = np.clip(t - cell, F32(0), F32(1)).astype(F32)
    return cell.astype(np.int64), f


def _corner_weights(f):
    """[(d0, d1, d2), w float32 [N]] in lexicographic order: (w0 * w1) * w2"""
    one = F32(1)
    for d0 in (0, 1):
        for d1 in (0, 1):
            for d2 in (0, 1):
                w0 = f[:, 0] if d0 else one - f[:, 0]
                w1 = f[:, 1] if d1 else one - f[:, 1]
                w2 = f[:, 2] if d2 else one - f[:, 2]
                yield (d0, d1, d2), (w0 * w1) * w2


def to_fixed(v):
    return np.rint(np.asarray(v, F32).astype(np.float64) * FIXED).astype(np.int64)


def splat(points, normals, depth, centre, side):
    """-> (channels int64 [4, n, n, n], usable count): np.add.at of llrint(value * 2^30), value in float32"""
    ok = usable(points, normals)
    p, nr = np.asarray(points, F32)[ok], np.asarray(normals, F32)[ok]
    n = nodes(depth)
    ch = np.zeros((4, n, n, n), np.int64)
    cell, f = _locate(p, depth, centre, side)
    n64 = nr.astype(np.float64)
    length = np.sqrt((n64[:, 0] * n64[:, 0] + n64[:, 1] * n64[:, 1]) + n64[:, 2] * n64[:, 2])
    unit = (n64 / length[:, None]).astype(F32)
    for (d0, d1, d2), w in _corner_weights(f):
        at = (cell[:, 0] + d0, cell[:, 1] + d1, cell[:, 2] + d2)
        np.add.at(ch[0], at, to_fixed(w))
        for c in range(3):
            np.add.at(ch[1 + c], at, to_fixed(w * unit[:, c]))
    return ch, int(ok.sum())


def from_fixed(ch):
    return (np.asarray(ch, np.int64).astype(np.float64) / FIXED).astype(F32)


def rhs(channels, depth, side):
    """b = ((d0 + d1) + d2) * inv_2h at interior nodes, d_a the central difference of vector channel a along axis a, float32"""
    n = nodes(depth)
    v = from_fixed(channels[1:])
    inv_2h = F32(1.0 / (2.0 * (side / (n - 1))))
    b = np.zeros((n, n, n), F32)
    i = slice(1, -1)
    d0 = v[0][2:, i, i] - v[0][:-2, i, i]
    d1 = v[1][i, 2:, i] - v[1][i, :-2, i]
    d2 = v[2][i, i, 2:] - v[2][i, i, :-2]
    b[i, i, i] = ((d0 + d1) + d2) * inv_2h
    return b


def sample(field, depth, centre, side, points, normals=None):
    """trilinear sample of a float32 lattice (or the int64 density channel) -> (values float32 [N], NaN where a point takes no
    part; fixed-point sum; count): acc = 0, acc += w * value over the corners in lexicographic order, in float32"""
    field = from_fixed(field) if field.dtype == np.int64 else np.asarray(field, F32)
    p = np.asarray(points, F32).reshape(-1, 3)
    ok = np.isfinite(p).all(1) if normals is None else usable(p, normals)
    q = p[ok]
    cell, f = _locate(q, depth, centre, side)
    acc = np.zeros(len(q), F32)
    for (d0, d1, d2), w in _corner_weights(f):
        acc = acc + w * field[cell[:, 0] + d0, cell[:, 1] + d1, cell[:, 2] + d2]
    out = np.full(len(p), np.nan, F32)
    out[ok] = acc
    good = np.isfinite(acc)
    return out, int(to_fixed(acc[good]).sum()), int(good.sum())


def laplacian_system(depth, side):
    """the 7-point Laplacian on the interior nodes with chi = 0 on the boundary, as a scipy CSR matrix in float64"""
    import scipy.sparse as sp
    n = nodes(depth)
    m = n - 2
    h = side / (n - 1)
    one = sp.diags([np.ones(m - 1), -2.0 * np.ones(m), np.ones(m - 1)], [-1, 0, 1]) if m > 1 else sp.csr_matrix([[-2.0]])
    eye = sp.identity(m)
    lap = sp.kron(sp.kron(one, eye), eye) + sp.kron(sp.kron(eye, one), eye) + sp.kron(sp.kron(eye, eye), one)
    return (lap / (h * h)).tocsr()


def solve_exact(b, depth, side):
    """chi float64 [n, n, n] with Laplacian(chi) = b at the interior nodes, 0 on the boundary (scipy.sparse.linalg.spsolve)"""
    from scipy.sparse.linalg import spsolve
    n = nodes(depth)
    x = spsolve(laplacian_system(depth, side).tocsc(), np.asarray(b, np.float64)[1:-1, 1:-1, 1:-1].reshape(-1))
    chi = np.zeros((n, n, n), np.float64)
    chi[1:-1, 1:-1, 1:-1] = x.reshape(n - 2, n - 2, n - 2)
    return chi


def residual(chi, b, depth, side):
    """max |b - Laplacian(chi)| over the interior nodes, float64"""
    x, r = np.asarray(chi, np.float64), np.asarray(b, np.float64)
    lap = laplacian_system(depth, side) @ x[1:-1, 1:-1, 1:-1].reshape(-1)
    return float(np.abs(r[1:-1, 1:-1, 1:-1].reshape(-1) - lap).max())


# ---- clouds --------------------------------------------------------------------------------------------------------------
def fibonacci_sphere(n, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """n points on a sphere (golden-angle spiral) and their exact outward unit normals, float32"""
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    a = np.pi * (3.0 - np.sqrt(5.0)) * i
    nrm = np.stack([r * np.cos(a), r * np.sin(a), z], 1)
    return (nrm * radius + np.asarray(centre, np.float64)).astype(F32), nrm.astype(F32)


def edge_cases(depth, centre, side, seed=0):
    """points exactly on nodes, on cell faces, inside cells, and unusable ones (NaN coordinates, zero and infinite normals)"""
    rng = np.random.default_rng(seed)
    n = nodes(depth)
    h = side / (n - 1)
    lo = np.asarray(centre, np.float64) - 0.5 * side
    idx = rng.integers(2, n - 2, (40, 3)).astype(np.float64)
    on_nodes = lo + idx[:10] * h
    on_faces = lo + (idx[10:20] + np.array([0.0, 0.37, 0.61])) * h
    inside = lo + (idx[20:] + rng.random((20, 3))) * h
    p = np.concatenate([on_nodes, on_faces, inside]).astype(F32)
    nr = rng.normal(size=p.shape).astype(F32)
    p[5, 1] = np.nan
    nr[17] = 0.0
    nr[25, 2] = np.inf
    p[33, 0] = -np.inf
    return p, nr
