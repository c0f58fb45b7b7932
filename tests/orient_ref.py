"""Restatement of the normal orientation written from the text, not from csrc/orient_core.h: brute-force
neighbour lists in numpy, Kruskal with a Python union-find under the total order (w, min, max), then a breadth-first walk of
the forest from each tree's top point.  Test-only; also the clouds the CPU and GPU tests share."""
from collections import deque

import numpy as np

F32 = np.float32


def usable(points, normals):
    p, n = np.asarray(points, F32), np.asarray(normals, F32)
    return np.isfinite(p).all(1) & np.isfinite(n).all(1) & (n != 0).any(1)


def unit(normals):
    """float64 division by the float64 length, rounded once to float32"""
    n = np.asarray(normals, F32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        return (n / length[:, None]).astype(F32)


def dot(u, i, j):
    a, b = u[i], u[j]
    return F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))


def neighbours(points, ok, k):
    """{i: the k nearest usable points other than i}: the (k + 1) smallest (d2, index) over the usable points, d2 =
    ((dx^2 + dy^2) + dz^2) in float32; the entry i is dropped, or the last one when i is absent"""
    p = np.asarray(points, F32)
    ids = np.nonzero(ok)[0]
    q = p[ids]
    out = {}
    for i in ids:
        d = q - p[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.lexsort((ids, d2))[:k + 1]
        row = [int(ids[o]) for o in order]
        if i in row:
            row.remove(i)
        elif len(row) == k + 1:
            row.pop()
        out[int(i)] = row
    return out


def orient(points, normals, k):
    """-> (sign int8 [N], tree int32 [N], report dict without `rounds`)"""
    p, nr = np.asarray(points, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3)
    n = len(p)
    ok = usable(p, nr)
    u = unit(nr)
    nb = neighbours(p, ok, k)
    edges = {}
    for i, row in nb.items():
        for j in row:
            a, b = min(i, j), max(i, j)
            if (a, b) not in edges:
                d = dot(u, a, b)
                edges[(a, b)] = (max(F32(1) - abs(d), F32(0)), bool(d < 0))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    forest = {i: [] for i in nb}
    for (a, b), (w, flip) in sorted(edges.items(), key=lambda e: (e[1][0], e[0][0], e[0][1])):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            forest[a].append((b, flip))
            forest[b].append((a, flip))
    sign, tree = np.zeros(n, np.int8), np.full(n, -1, np.int32)
    members = {}
    for i in nb:
        members.setdefault(find(i), []).append(i)
    for group in members.values():
        top = max(group, key=lambda i: (p[i, 2], -i))
        sign[top] = -1 if nr[top, 2] < 0 else 1
        queue = deque([top])
        while queue:
            i = queue.popleft()
            for j, flip in forest[i]:
                if sign[j] == 0:
                    sign[j] = -sign[i] if flip else sign[i]
                    queue.append(j)
        tree[group] = min(group)
    bad = sum(1 for (a, b), (_, flip) in edges.items() if (sign[a] != sign[b]) != flip)
    return sign, tree, {"usable": int(ok.sum()), "trees": len(members), "flipped": int((sign < 0).sum()), "frustrated": bad}


# ---- clouds --------------------------------------------------------------------------------------------------------------
def fibonacci_sphere(n, radius=1.0, centre=(0.0, 0.0, 0.0)):
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    a = np.pi * (3.0 - np.sqrt(5.0)) * i
    nrm = np.stack([r * np.cos(a), r * np.sin(a), z], 1)
    return (nrm * radius + np.asarray(centre, np.float64)).astype(F32), nrm.astype(F32)


def coin_flipped(normals, seed):
    s = np.where(np.random.default_rng(seed).random(len(normals)) < 0.5, -1.0, 1.0).astype(F32)
    return (normals * s[:, None]).astype(F32)


def random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    nr = rng.normal(size=(n, 3))
    return rng.random((n, 3)).astype(F32), (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F32)


def clouds():
    """name -> (points, normals, k): the cases of the issue"""
    out = {}
    p, nr = random_cloud(500, 1)
    out["random500"] = (p, nr, 8)
    g = np.arange(9, dtype=F32) * F32(0.125)
    lat = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    out["lattice9x9"] = (np.concatenate([lat, np.zeros((81, 1), F32)], 1), np.tile(np.array([[0, 0, 1]], F32), (81, 1)), 4)
    p, nr = random_cloud(60, 2)
    out["tripled"] = (np.concatenate([p, p, p]), random_cloud(180, 3)[1], 5)
    out["tripled_k1"] = (np.concatenate([p, p, p]), random_cloud(180, 3)[1], 1)     # the third copy is absent from its own row
    (pa, na), (pb, nb) = fibonacci_sphere(300), fibonacci_sphere(200, 1.0, (10.0, 0.0, 0.0))
    out["two_spheres"] = (np.concatenate([pa, pb]), coin_flipped(np.concatenate([na, nb]), 4), 6)
    p, nr = random_cloud(200, 5)
    nr[3] = np.nan
    nr[40] = 0.0
    nr[77, 1] = np.inf
    p[120, 0] = np.nan
    out["nonfinite"] = (p, nr, 8)
    out["one"] = (np.array([[0.5, 0.25, 0.125]], F32), np.array([[0, 0, -2]], F32), 3)
    out["two"] = (np.array([[0, 0, 0], [1, 0, 0]], F32), np.array([[0, 1, 1], [0, -1, -1]], F32), 3)
    return out
