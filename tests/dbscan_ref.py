"""DBSCAN as DESIGN.md section 4m defines it, restated in numpy from the text (dense float64 d2, breadth-first components),
and the clouds that tests/test_dbscan_cpu.py and tests/test_dbscan_gpu.py share.  Test-only; nothing here imports the product.

The definition: a point is usable when its three float32 coordinates are finite.  q is a neighbour of p iff, with every
coordinate widened to float64, d2 = ((dx*dx) + dy*dy) + dz*dz <= eps*eps (eps*eps once, in float64); a point is its own
neighbour.  count = neighbours, core = count >= min_samples.  Clusters are the connected components of the core points under
the neighbour relation, numbered in ascending order of their smallest core index.  A non-core point with a core neighbour takes
the smallest cluster number among its core neighbours; everything else is -1."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPORT = ("n_usable", "n_core", "n_border", "n_noise", "n_clusters", "largest", "largest_size")


def dbscan(points, eps, min_samples):
    """-> dict(labels int32 [n], counts uint32 [n], core bool [n], report)"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    labels, counts, core = np.full(n, -1, np.int32), np.zeros(n, np.uint32), np.zeros(n, bool)
    use = np.nonzero(np.isfinite(p).all(1))[0]
    m = len(use)
    x = p[use].astype(np.float64)
    eps2 = np.float64(eps) * np.float64(eps)
    adj = np.zeros((m, m), bool)
    for a in range(0, m, 512):
        dx, dy, dz = (x[a:a + 512, None, c] - x[None, :, c] for c in range(3))
        adj[a:a + 512] = ((dx * dx) + dy * dy) + dz * dz <= eps2
    cnt = adj.sum(1)
    is_core = cnt >= min_samples
    lab = np.full(m, -1, np.int64)
    n_clusters = 0
    for i in range(m):                              # ascending index: a new cluster starts at its smallest core index
        if not is_core[i] or lab[i] >= 0:
            continue
        lab[i] = n_clusters
        front = np.array([i])
        while len(front):
            reach = adj[front].any(0) & is_core & (lab < 0)
            lab[reach] = n_clusters
            front = np.nonzero(reach)[0]
        n_clusters += 1
    big = np.iinfo(np.int64).max
    for a in range(0, m, 512):
        best = np.where(adj[a:a + 512] & is_core[None, :], lab[None, :], big).min(1, initial=big)
        rows = np.arange(a, min(a + 512, m))
        take = ~is_core[rows] & (best != big)
        lab[rows[take]] = best[take]
    labels[use], counts[use], core[use] = lab, cnt, is_core
    sizes = np.bincount(lab[lab >= 0], minlength=n_clusters)
    largest = int(sizes.argmax()) if n_clusters else -1           # argmax: the lowest number on a tie
    n_core, n_border = int(is_core.sum()), int(((lab >= 0) & ~is_core).sum())
    report = dict(zip(REPORT, (m, n_core, n_border, m - n_core - n_border, n_clusters, largest, int(sizes[largest]) if n_clusters else 0)))
    return {"labels": labels, "counts": counts, "core": core, "report": report}


def largest_cluster_rows(labels):
    """the rows that the reference's filter_dbscan keeps: the largest cluster, every row without a cluster"""
    lab = np.asarray(labels)
    if not (lab >= 0).any():
        return np.arange(len(lab))
    sizes = np.bincount(lab[lab >= 0])
    return np.nonzero(lab == sizes.argmax())[0]


# ---- the clouds: name -> (points float32 [n,3], eps, min_samples) ---------------------------------------------------------------------
# The random clouds have n with 0.02 * (n - 1) = k + 0.5: a 2 % quantile bound then lies midway between two order statistics, not
# on top of one (tools/make_dbscan_goldens.py searches the seed that keeps every bound clear of every coordinate).
def _lattice(k, h):
    g = np.arange(k, dtype=np.float64) * h
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def uniform(seed=1, n=1976):
    return np.random.default_rng(seed).uniform(0, 1, (n, 3)).astype(np.float32)


def blobs(seed=2):
    """three Gaussian blobs of which two touch, and a sprinkle of noise, in scrambled order"""
    r = np.random.default_rng(seed)
    parts = [r.normal((0, 0, 0), 0.05, (700, 3)), r.normal((0.17, 0, 0), 0.05, (700, 3)), r.normal((0.8, 0.6, 0.1), 0.05, (500, 3)),
             r.uniform(-0.3, 1.1, (126, 3))]
    p = np.concatenate(parts)
    return p[r.permutation(len(p))].astype(np.float32)


def shell(seed=3):
    """what the reference cleans: a thin noisy sphere shell, a small satellite and stray points"""
    r = np.random.default_rng(seed)
    d = r.normal(size=(2600, 3))
    body = 0.4 * d / np.linalg.norm(d, axis=1, keepdims=True) + r.normal(0, 0.004, (2600, 3))
    sat = r.normal((0.75, 0.1, 0), 0.02, (250, 3))
    p = np.concatenate([body, sat, r.uniform(-0.6, 0.9, (126, 3))])
    return p[r.permutation(len(p))].astype(np.float32)


def far(seed=4):
    """a box much larger than eps: four small clusters at far corners, most cells empty"""
    r = np.random.default_rng(seed)
    c = np.array([(0, 0, 0), (100, 0, 0), (0, 80, 5), (100, 80, 60)], np.float64)
    p = np.concatenate([r.normal(c[j], 0.01, (150, 3)) for j in range(4)] + [r.uniform(0, 100, (26, 3))])
    return p[r.permutation(len(p))].astype(np.float32)


def duplicates():
    p = np.random.default_rng(5).uniform(0, 1, (200, 3)).astype(np.float32)
    return np.concatenate([p] * 5)


def slabs(order):
    """Two 3^3 slabs of spacing eps = 0.25, 2 eps apart, and one point exactly eps from each: a contested border point.  Row 0
    is a border point of the +x slab alone (it appears before every core point).  order "ab": the -x slab first; "ba": the +x
    slab first.  All arithmetic is exact."""
    a = _lattice(3, 0.25) + (-0.75, 0, 0)
    b = _lattice(3, 0.25) + (0.25, 0, 0)
    first = np.array([[1.0, 0.25, 0.25]])
    mid = np.array([[0.0, 0.25, 0.25]])
    return np.concatenate([first] + ([a, b] if order == "ab" else [b, a]) + [mid]).astype(np.float32)


def chain(n=4097):
    """n points at spacing eps = 0.25 along x, in scrambled index order"""
    x = np.arange(n, dtype=np.float64) * 0.25
    p = np.stack([x, np.full(n, 0.5), np.full(n, -0.25)], 1)
    return p[np.random.default_rng(6).permutation(n)].astype(np.float32)


def isolated():
    p = _lattice(5, 1.0)
    return p[np.random.default_rng(7).permutation(len(p))].astype(np.float32)


def nonfinite():
    p = uniform(8, 1500)
    r = np.random.default_rng(9)
    bad = r.choice(len(p), 90, replace=False)
    p[bad[:30], r.integers(0, 3, 30)] = np.nan
    p[bad[30:60], r.integers(0, 3, 30)] = np.inf
    p[bad[60:], r.integers(0, 3, 30)] = -np.inf
    return p


def rounding(eps=0.1, pairs=40):
    """Pairs of points whose distance is within a few 1e-8 of eps, chosen among 20 000 candidates as those on which the float64
    predicate and a float32 d2 disagree: a sparse cloud (min_samples = 2) whose labels hang on the arithmetic of d2."""
    r = np.random.default_rng(12)
    d = r.normal(size=(20000, 3))
    d *= (eps * (1 + r.uniform(-3e-8, 3e-8, 20000)) / np.linalg.norm(d, axis=1))[:, None]
    a = r.uniform(0, 1, (20000, 3)).astype(np.float32)
    b = (a.astype(np.float64) + d).astype(np.float32)
    e = a.astype(np.float64) - b.astype(np.float64)
    wide = ((e[:, 0] * e[:, 0]) + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    f = a - b
    narrow = ((f[:, 0] * f[:, 0]) + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]
    eps2 = np.float64(eps) * np.float64(eps)
    pick = np.nonzero((wide <= eps2) != (narrow.astype(np.float64) <= eps2))[0][:pairs]
    assert len(pick) == pairs and narrow.dtype == np.float32
    return np.concatenate([a[pick], b[pick]])


# name -> (builder, eps, min_samples, takes part in the quantile filter's golden).  "far" does not: its 2 % bounds fall inside a
# cluster whose spacing is far below 1e-5 of the box.
RANDOM = {"uniform": (uniform, 0.08, 5, True), "blobs": (blobs, 0.03, 8, True), "shell": (shell, 0.06, 10, True), "far": (far, 0.02, 5, False)}
_FIXED = None


def fixed_clouds():
    """the clouds that are the same whatever the seed search of tools/make_dbscan_goldens.py finds"""
    global _FIXED
    if _FIXED is None:
        c = {"lattice6": (_lattice(9, 0.25).astype(np.float32), 0.25, 6), "lattice7": (_lattice(9, 0.25).astype(np.float32), 0.25, 7),
             "duplicates": (duplicates(), 0.15, 6), "slabs_ab": (slabs("ab"), 0.25, 4), "slabs_ba": (slabs("ba"), 0.25, 4),
             "chain": (chain(), 0.25, 2), "isolated": (isolated(), 0.25, 1), "nonfinite": (nonfinite(), 0.08, 5),
             "all_nonfinite": (np.full((5, 3), np.nan, np.float32), 0.1, 1), "bigeps": (uniform(10, 300), 10.0, 10), "rounding": (rounding(), 0.1, 2)}
        for n in (0, 1, 63, 64, 65):
            c["n%d" % n] = (uniform(11, 65)[:n], 0.2, 3)
        _FIXED = c
    return _FIXED


def golden():
    """(clouds of RANDOM as recorded, expectations) from tests/golden"""
    with np.load(os.path.join(GOLDEN, "dbscan_clouds.npz")) as z:
        pts = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "dbscan_expect.json")) as f:
        return pts, json.load(f)


_CLOUDS = None


def clouds():
    """every cloud: name -> (points, eps, min_samples)"""
    global _CLOUDS
    if _CLOUDS is None:
        pts, _ = golden()
        c = {k: (pts[k], RANDOM[k][1], RANDOM[k][2]) for k in RANDOM}
        c.update(fixed_clouds())
        _CLOUDS = c
    return _CLOUDS
