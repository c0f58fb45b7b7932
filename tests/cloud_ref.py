"""numpy restatement of the point-cloud neighbour search and the clouds its tests run on (test-only).

The definition: d2(p, q_i) = ((px-qx)^2 + (py-qy)^2) + (pz-qz)^2 in float32, one rounding per operation; the answer for k is
the k smallest (d2, i) in lexicographic order.  numpy's float32 arithmetic is uncontracted (one ufunc per operation), so the
product must equal this bit for bit."""
import numpy as np

QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def usable(points):
    return np.isfinite(np.asarray(points, np.float32).reshape(-1, 3)).all(1)


def knn(queries, points, k):
    """brute force -> (dist2 float32 [N,k], index int32 [N,k]); np.lexsort on (index, d2) per query.  Fewer than k usable
    points: (+inf, -1) in the remaining slots; a query with a non-finite coordinate: (NaN, -1) everywhere."""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    idx = np.nonzero(usable(p))[0].astype(np.int32)
    t = p[idx]
    d2o = np.full((len(q), k), np.inf, np.float32)
    ixo = np.full((len(q), k), -1, np.int32)
    m = min(k, len(idx))
    for i in range(len(q)):
        if not np.isfinite(q[i]).all():
            d2o[i] = QNAN
            continue
        dx, dy, dz = q[i, 0] - t[:, 0], q[i, 1] - t[:, 1], q[i, 2] - t[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        order = np.lexsort((idx, d2))[:m]
        d2o[i, :m] = d2[order]
        ixo[i, :m] = idx[order]
    return d2o, ixo


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the clouds ---------------------------------------------------------------------------------------------------------------
def uniform(n, seed=0, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def lattice(m=9):
    """m^3 points at exact multiples of 1 / (m - 1): at forced resolution m - 1 every point sits on a cell border"""
    a = np.arange(m, dtype=np.float32) / np.float32(m - 1)
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)


def tripled(n, seed=1):
    """every point stored three times, the copies scattered through the index range"""
    p = np.tile(uniform(n, seed), (3, 1))
    return p[np.random.default_rng(seed + 100).permutation(len(p))]


def coplanar(n, seed=2):
    p = uniform(n, seed)
    p[:, 2] = np.float32(0.25)
    return p


def repeated(n):
    return np.tile(np.array([[0.5, -0.25, 2.0]], np.float32), (n, 1))


def far_queries(n, seed=3):
    """points far outside [-1, 1]^3, on every side, at distances from a few to a million box sizes"""
    r = np.random.default_rng(seed)
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * (10.0 ** r.uniform(0.5, 6.0, (n, 1)))).astype(np.float32)


def with_nonfinite(points, seed=4, share=0.1):
    """a copy with NaN / +inf / -inf in one coordinate of about `share` of the rows -> (points, number of such rows)"""
    p = np.array(points, np.float32)
    r = np.random.default_rng(seed)
    rows = r.choice(len(p), max(1, int(share * len(p))), replace=False)
    p[rows, r.integers(0, 3, len(rows))] = np.array([np.nan, np.inf, -np.inf], np.float32)[r.integers(0, 3, len(rows))]
    return p, len(rows)


def queries_for(points, n, seed=5):
    """n queries: points of the cloud itself (distance 0, ties between copies), jittered ones, and free ones around the box"""
    p = np.asarray(points, np.float32)[usable(points)]
    r = np.random.default_rng(seed)
    own = p[r.integers(0, len(p), n // 3)]
    jit = p[r.integers(0, len(p), n // 3)] + r.normal(0, 0.02, (n // 3, 3)).astype(np.float32)
    free = r.uniform(-1.5, 1.5, (n - 2 * (n // 3), 3)).astype(np.float32)
    return np.concatenate([own, jit, free]).astype(np.float32)


# ---- restatements of what r3g/cloud.py builds on the k-lists ------------------------------------------------------------------
def covariances(points, index):
    """float64 covariance of each row's neighbours, summed in the k-list's order -> [N,3,3]; rows with an index < 0 excluded
    are the caller's business (every index must be >= 0 here)"""
    p = np.asarray(points, np.float32).astype(np.float64)
    nb = p[index]                                   # [N,k,3]
    k = index.shape[1]
    s = np.zeros((len(index), 3))
    for j in range(k):
        s = s + nb[:, j]
    mean = s / k
    d = nb - mean[:, None, :]
    c = np.zeros((len(index), 3, 3))
    for j in range(k):
        c = c + d[:, j, :, None] * d[:, j, None, :]
    return c / k
