"""numpy restatement of the hierarchical volume decoder's planner (DESIGN.md "Hierarchical volume decoding", include/r3g.h).
Test code: the product never imports it.

    levels(R)                       resolutions, coarsest first
    plan(G, lam, beta, last)        bool mask F of the (2n-1)^3 lattice the next level evaluates
    active_indices(F)               its ascending linear indices (int32)
    fill(G, n)                      the floor-parent fill of the finer lattice
    hier(dense_at, R, lam, beta)    the level loop over a field given as dense_at(R_l) -> (R_l+1)^3 array
    mixed_cells / all_corners_active / missed_and_unsafe
Predicates are evaluated in float64 on the float32 samples, as the library and marching cubes do.
"""
import numpy as np


def levels(R, min_res=63):
    out = [int(R)]
    while out[-1] % 2 == 0 and out[-1] // 2 >= min_res:
        out.append(out[-1] // 2)
    return out[::-1]


def dilate(m, times=1):
    """binary dilation by the 3x3x3 box, clipped to the grid (separable: one pass per axis)"""
    m = m.copy()
    for _ in range(times):
        for ax in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, -1), slice(1, None)
            d = m.copy()
            d[tuple(lo)] |= m[tuple(hi)]
            d[tuple(hi)] |= m[tuple(lo)]
            m = d
    return m


def plan(G, lam, beta, last):
    G = np.asarray(G, np.float32)
    with np.errstate(invalid="ignore"):
        g = G.astype(np.float64)
        s = g > lam
        near = np.zeros_like(s)
        for ax in range(3):
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[ax], b[ax] = slice(0, -1), slice(1, None)
            d = s[tuple(a)] != s[tuple(b)]
            near[tuple(a)] |= d
            near[tuple(b)] |= d
        cand = near | (np.abs(g - lam) < beta)
    e = 0 if last else 1
    C = dilate(cand, e)
    n = 2 * (G.shape[0] - 1) + 1
    F = np.zeros((n, n, n), bool)
    F[::2, ::2, ::2] = C
    return dilate(F, 2 - e)


def active_indices(F):
    return np.flatnonzero(F.reshape(-1)).astype(np.int32)


def fill(G, n):
    idx = np.arange(n) >> 1
    return G[np.ix_(idx, idx, idx)].copy()


def hier(dense_at, R, lam, beta, min_res=63):
    """-> (final grid, mask of the finest level or None, evaluated per level)"""
    L = levels(R, min_res)
    G = np.array(dense_at(L[0]), np.float32)
    per_level = [G.size]
    F = None
    for li in range(1, len(L)):
        F = plan(G, lam, beta, li == len(L) - 1)
        N = fill(G, L[li] + 1)
        N[F] = dense_at(L[li])[F]
        per_level.append(int(F.sum()))
        G = N
    return G, F, per_level


def strided(dense):
    """dense_at for a field given as its finest volume: level l is every (R / R_l)-th sample"""
    R = dense.shape[0] - 1

    def at(Rl):
        st = R // Rl
        return dense[::st, ::st, ::st]
    return at


def _corners(a):
    n = a.shape[0] - 1
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                yield a[dx:dx + n, dy:dy + n, dz:dz + n]


def mixed_cells(G, lam):
    with np.errstate(invalid="ignore"):
        s = np.asarray(G, np.float32).astype(np.float64) > lam
    c = np.zeros(tuple(k - 1 for k in s.shape), np.int8)
    for v in _corners(s):
        c += v
    return (c > 0) & (c < 8)


def all_corners_active(F):
    a = np.ones(tuple(k - 1 for k in F.shape), bool)
    for v in _corners(F):
        a &= v
    return a


def missed_and_unsafe(dense, G, F, lam):
    """(dense mixed cells with a corner outside F, mixed cells of the hierarchical grid with a corner outside F)"""
    aa = all_corners_active(F)
    return int((mixed_cells(dense, lam) & ~aa).sum()), int((mixed_cells(G, lam) & ~aa).sum())


# ---- the analytic 257^3 fields of the issue --------------------------------------------------------------------
def analytic_field(name, n=257):
    """-> (float32 volume, level)"""
    I, J, K = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    I, J, K = I.astype(np.int64), J.astype(np.int64), K.astype(np.int64)
    if name == "sphere":            # golden D of tests/mc_volumes.py at n = 257
        h = n // 2
        return (10000 - ((I - h) ** 2 + (J - h) ** 2 + (K - h) ** 2)).astype(np.float32), 0.5
    if name == "ellipsoid":
        return (4 * n * n - (4 * (I - n // 2) ** 2 + 9 * (J - n // 3) ** 2 + 25 * (K - n // 2) ** 2)).astype(np.float32), 0.5
    x, y, z = [(a / (n - 1) * 2 - 1).astype(np.float32) for a in (I, J, K)]

    def sph(cx, cy, cz, r):
        return r - np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)

    def rod(r):
        return r - np.sqrt(y ** 2 + z ** 2) + np.where(np.abs(x) < .9, 0, -1).astype(np.float32)
    if name in ("blobs_sharp", "blobs_soft"):
        sd = np.maximum.reduce([sph(0, 0, 0, .5), sph(.45, .1, 0, .3), sph(-.3, -.4, .2, .25), rod(0.03)])
        return (np.tanh(sd * (128. if name == "blobs_sharp" else 16.)) * 5).astype(np.float32), 0.0
    if name == "thin_rod":
        return (np.tanh(np.maximum(sph(0, 0, 0, .5), rod(0.012)) * 128.) * 5).astype(np.float32), 0.0
    raise KeyError(name)


ANALYTIC = ("sphere", "ellipsoid", "blobs_sharp", "blobs_soft", "thin_rod")
