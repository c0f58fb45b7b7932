"""numpy / Python restatement of the hole-filling primitive and the fixtures of its tests.

Nothing here shares code with csrc/meshfill_core.h or with the mate table of section 4i: the boundary edges come from np.unique
over sorted vertex pairs (an edge that exactly one half-edge of a usable face runs along), succ is a Python dict from a simple
head vertex to the one boundary half-edge that leaves it, and every cycle is walked half-edge by half-edge."""
import numpy as np


class BadIndex(ValueError):
    code = -2


def boundary_half_edges(faces, n_verts):
    """ascending ids h = 3 f + k of the half-edges of usable faces whose undirected edge no other half-edge runs along, with their
    tails and heads"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if ((f < 0) | (f >= n_verts)).any():
        raise BadIndex("a face index lies outside [0, %d)" % n_verts)
    usable = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    h = (3 * np.flatnonzero(usable)[:, None] + np.arange(3)[None]).reshape(-1)
    tail, head = f.reshape(-1)[h], f[h // 3, (h % 3 + 1) % 3]
    key = np.minimum(tail, head) * n_verts + np.maximum(tail, head)
    _, inv, deg = np.unique(key, return_inverse=True, return_counts=True)
    sel = deg[inv.reshape(-1)] == 1
    return h[sel], tail[sel], head[sel]


def loops(faces, n_verts):
    """-> (boundary count, [(leader half-edge id, [a_0 .. a_(L-1)])] ascending by leader)"""
    h, tail, head = boundary_half_edges(faces, n_verts)
    nout, nin = np.bincount(tail, minlength=n_verts), np.bincount(head, minlength=n_verts)
    simple = (nout == 1) & (nin == 1)
    leaves = {int(t): i for i, t in enumerate(tail) if simple[t]}          # simple vertex -> the boundary half-edge that leaves it
    succ = {i: leaves[int(head[i])] for i in range(len(h)) if simple[head[i]]}
    seen, found = set(), []
    for i in range(len(h)):                      # ascending half-edge id: the first visit of a cycle is at its leader
        if i in seen:
            continue
        path, j = [], i
        while j is not None and j not in seen:
            seen.add(j)
            path.append(j)
            j = succ.get(j)
        if j == i:                               # the walk came back to where it began: a cycle, and i is its lowest id
            found.append((int(h[i]), [int(tail[k]) for k in path]))
        # otherwise the walk ended (-1) or ran into a chain seen before: tangled; a later walk cannot enter a cycle, because
        # every vertex on a cycle has a single boundary half-edge coming in
    return len(h), found


def centroid(points):
    """float32 [L,3] in rank order -> float32 [3]: float64 running sum, one addition at a time, / L, rounded to float32"""
    s = np.zeros(3, np.float64)
    with np.errstate(all="ignore"):
        for p in np.asarray(points, np.float32):
            s = s + p.astype(np.float64)
        return (s / np.float64(len(points))).astype(np.float32)


def plan(verts, faces, max_loop=64, mode="fan", n_verts=None):
    """-> dict(report, loop_start, loop_verts, status, new_faces, new_verts) by the text of section 4j"""
    nv = len(verts) if verts is not None else int(n_verts)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0 or max_loop < 3 or mode not in ("fan", "centroid") or (mode == "centroid" and verts is None):
        raise ValueError("invalid")
    boundary, found = loops(f, nv)
    new_faces, new_verts, start, lverts, status = [], [], [0], [], []
    for _, a in found:
        L = len(a)
        lverts += a
        start.append(len(lverts))
        status.append(0 if L <= max_loop else 1)
        if L > max_loop:
            continue
        if mode == "fan":
            new_faces += [(a[0], a[i + 1], a[i]) for i in range(1, L - 1)]
        else:
            c = nv + len(new_verts)
            new_verts.append(centroid(np.asarray(verts, np.float32)[a]))
            new_faces += [(c, a[(i + 1) % L], a[i]) for i in range(L)]
    lens = [len(a) for _, a in found]
    rounds = 0 if boundary == 0 else max(1, int(boundary - 1).bit_length())
    rep = {"boundary": boundary, "loops": len(found), "tangled": boundary - sum(lens), "filled": status.count(0),
           "oversize": status.count(1), "longest": max(lens, default=0), "loop_edges": sum(lens), "faces_added": len(new_faces),
           "verts_added": len(new_verts), "rounds": rounds, "max_loop": int(max_loop), "mode": ("fan", "centroid").index(mode),
           "n_faces": len(f), "n_verts": nv}
    return {"report": rep, "loop_start": np.asarray(start, np.int64), "loop_verts": np.asarray(lverts, np.int32).reshape(-1),
            "status": np.asarray(status, np.int32).reshape(-1), "new_faces": np.asarray(new_faces, np.int32).reshape(-1, 3),
            "new_verts": np.asarray(new_verts, np.float32).reshape(-1, 3)}


def canonical(faces):
    """every face rotated so that its lowest index comes first (the winding is kept), rows sorted"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    k = np.argmin(f, axis=1)
    rot = np.stack([f[np.arange(len(f)), (k + i) % 3] for i in range(3)], 1)
    return rot[np.lexsort((rot[:, 2], rot[:, 1], rot[:, 0]))]


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def cone(n):
    """apex 0 and a rim 1 .. n in the plane z = 0, wound outward (apex up), no base: the rim is one loop of length n"""
    ang = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0, 0, 1]], np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)]).astype(np.float32)
    return v, np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)


def tube(n):
    """an open tube: rims 0 .. n-1 (z = 0) and n .. 2n-1 (z = 1), 2 n faces, two loops of length n"""
    ang = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(ang), np.sin(ang)], 1)
    v = np.concatenate([np.c_[ring, np.zeros(n)], np.c_[ring, np.ones(n)]]).astype(np.float32)
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [[i, j, n + j], [i, n + j, n + i]]
    return v, np.array(f, np.int32)


def bow_tie(n=5):
    """two open cones whose rims share one vertex (rim vertex 1 of the first is rim vertex 1 of the second)"""
    v1, f1 = cone(n)
    v2, f2 = cone(n)
    v2 = v2 + np.array([2, 0, 0], np.float32)
    v2[1:, 0] = 2 - (v2[1:, 0] - 2)                      # mirrored, so that its rim vertex 1 lands on (1, 0, 0) ...
    f2 = f2[:, ::-1] + len(v1)                           # ... and rewound outward
    f2[f2 == len(v1) + 1] = 1
    return np.concatenate([v1, v2]), np.concatenate([f1, f2]).astype(np.int32)


def permuted(faces, seed):
    return np.ascontiguousarray(np.asarray(faces)[np.random.default_rng(seed).permutation(len(faces))])


def trimesh_stand_in():
    """compat/trimesh loaded from its file under a private name (sys.modules keeps no `trimesh`)"""
    import importlib.util
    import os
    import r3g
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(r3g.__file__))), "compat", "trimesh", "__init__.py")
    spec = importlib.util.spec_from_file_location("r3g_compat_trimesh", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
