"""The plane fit's definition restated in numpy float64 (include/r3g.h "plane fit"), and the named clouds
the tests run on.  Written from the definition's text, not from csrc/plane_core.h: the twin (tests/emu_plane.py) must equal it.

A point is usable when its three coordinates are finite.  Hypothesis (i0, i1, i2): v1 = p[i1] - p[i0], v2 = p[i2] - p[i0],
c = v1 x v2, len = sqrt((cx*cx + cy*cy) + cz*cz) in float64 on the float32 coordinates; valid when the indices are in range, the
points usable and len >= 1e-6; unit normal c / len.  q is an inlier iff |((qx-p0x)*nx + (qy-p0y)*ny) + (qz-p0z)*nz| < threshold.
The winner is the valid hypothesis with the largest count, the lowest h on a tie.  Every operation below is one IEEE float64
operation per element, in the definition's order, so counts, winner and mask are exact; the sums of the moments are numpy's
(another order), so centroid, scatter and normal agree to rounding only."""
import numpy as np

REPORT = ("n_usable", "n_valid", "best", "best_count", "few")


def usable(points):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return np.isfinite(p).all(axis=1)


def hypotheses(points, triples):
    """-> (p0 float64 [H,3], normal float64 [H,3], valid bool [H]); invalid rows are zero"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    t = np.asarray(triples, np.int64).reshape(-1, 3)
    n, h = len(p), len(t)
    p0, nr, valid = np.zeros((h, 3)), np.zeros((h, 3)), np.zeros(h, bool)
    ok = usable(p)
    for k in range(h):
        i0, i1, i2 = (int(v) for v in t[k])
        if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= n or not (ok[i0] and ok[i1] and ok[i2]):
            continue
        a, b, c = p[i0].astype(np.float64), p[i1].astype(np.float64), p[i2].astype(np.float64)
        v1, v2 = b - a, c - a
        cx = v1[1] * v2[2] - v1[2] * v2[1]
        cy = v1[2] * v2[0] - v1[0] * v2[2]
        cz = v1[0] * v2[1] - v1[1] * v2[0]
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
        if not ln >= 1e-6:
            continue
        p0[k], nr[k], valid[k] = a, np.array([cx / ln, cy / ln, cz / ln]), True
    return p0, nr, valid


def distances(points, p0, normal):
    """d(h, q) for one hypothesis over all rows, float64 [n] (NaN or inf on unusable rows)"""
    q = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(((q[:, 0] - p0[0]) * normal[0] + (q[:, 1] - p0[1]) * normal[1]) + (q[:, 2] - p0[2]) * normal[2])


def distances_float32(points, p0, normal):
    """the same expression in float32 throughout (what the definition is NOT): the twin's float32 mutant"""
    q = np.asarray(points, np.float32).reshape(-1, 3)
    a, b = np.asarray(p0, np.float64).astype(np.float32), np.asarray(normal, np.float64).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(((q[:, 0] - a[0]) * b[0] + (q[:, 1] - a[1]) * b[1]) + (q[:, 2] - a[2]) * b[2])


def moments(points, mask=None):
    """-> dict(n, skipped, centroid [3], scatter [6] (xx, xy, xz, yy, yz, zz), eigenvalues [3] ascending, normal [3], few)"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    sel = np.ones(len(p), bool) if mask is None else np.asarray(mask).astype(bool)
    ok = usable(p)
    q = p[sel & ok].astype(np.float64)
    n = len(q)
    c = q.sum(axis=0) / n if n else np.zeros(3)
    d = q - c
    s = np.array([(d[:, a] * d[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
    out = {"n": n, "skipped": int((sel & ~ok).sum()), "centroid": c, "scatter": s, "few": int(n < 3)}
    if n < 3:
        out["eigenvalues"], out["normal"] = np.zeros(3), np.array([0.0, 1.0, 0.0])
        return out
    m = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
    val, vec = np.linalg.eigh(m)
    nr = vec[:, 0] / np.linalg.norm(vec[:, 0])
    out["eigenvalues"], out["normal"] = val, (-nr if nr[1] < 0 else nr)
    return out


def ransac(points, triples, threshold):
    """-> dict(counts uint32 [H], mask uint8 [n], report, p0, normal (the winner's), moments (of the inliers))"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    p0, nr, valid = hypotheses(p, triples)
    ok = usable(p)
    counts = np.zeros(len(p0), np.uint32)
    for h in range(len(p0)):
        if valid[h]:
            counts[h] = int(((distances(p, p0[h], nr[h]) < threshold) & ok).sum())
    best = -1
    for h in range(len(p0)):
        if valid[h] and (best < 0 or counts[h] > counts[best]):
            best = h
    mask = np.zeros(len(p), np.uint8)
    if best >= 0:
        mask = ((distances(p, p0[best], nr[best]) < threshold) & ok).astype(np.uint8)
    mom = moments(p, mask)
    report = {"n_usable": int(ok.sum()), "n_valid": int(valid.sum()), "best": best, "best_count": int(counts[best]) if best >= 0 else 0,
              "few": mom["few"]}
    return {"counts": counts, "mask": mask, "report": report, "p0": p0[best] if best >= 0 else np.zeros(3),
            "normal": nr[best] if best >= 0 else np.zeros(3), "moments": mom}


# ---- yaw search, oriented box and plane frame: this project's own definitions ------------------------------------------------
def yaw_rotation(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def centre_of(points, method="bbox"):
    p = np.asarray(points, np.float64)
    if method == "bbox":
        return (p.min(axis=0) + p.max(axis=0)) / 2.0
    if method == "median":
        return np.sort(p, axis=0)[(len(p) - 1) // 2]      # torch.median: the lower of the two middle values
    return p.mean(axis=0)


def chamfer(a, b):
    """mean squared nearest-neighbour distance each way, summed (brute force, float64)"""
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    return d2.min(axis=1).mean() + d2.min(axis=0).mean()


def yaw_losses(verts, target, num_angles=18, centroid_method="bbox"):
    v = np.asarray(verts, np.float64) - centre_of(verts, centroid_method)
    t = np.asarray(target, np.float64) - centre_of(target, centroid_method)
    angles = np.linspace(0.0, 2 * 3.14159, num_angles)
    losses = np.array([chamfer(v @ yaw_rotation(a).T, t) for a in angles])
    return losses, int(np.argmin(losses))


def plane_frame(normal, point):
    """plane->world and world->plane, 4 x 4 float64 on column vectors: plane-y is the normal; z = normalise(y x ref),
    x = normalise(y x z), ref = world X, or world Z when |n_x| > 0.9"""
    y = np.asarray(normal, np.float64).reshape(3)
    y = y / np.linalg.norm(y)
    ref = np.array([0.0, 0.0, 1.0]) if abs(y[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    z = np.cross(y, ref)
    z = z / np.linalg.norm(z)
    x = np.cross(y, z)
    x = x / np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, np.asarray(point, np.float64).reshape(3)
    inv = np.eye(4)
    inv[:3, :3] = m[:3, :3].T
    inv[:3, 3] = -m[:3, :3].T @ m[:3, 3]
    return m, inv


def yaw_obb(points):
    """centroid, rotation about y whose columns 0 and 2 are the principal axes of the xz scatter (larger first), extents of
    (p - centroid) @ rotation"""
    p = np.asarray(points, np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    c = p.mean(axis=0)
    d = p - c
    sxx, sxz, szz = (d[:, 0] ** 2).sum(), (d[:, 0] * d[:, 2]).sum(), (d[:, 2] ** 2).sum()
    theta = 0.5 * np.arctan2(2.0 * sxz, sxx - szz)       # the major axis is (cos, sin) in (x, z)
    co, si = np.cos(theta), np.sin(theta)
    rot = np.array([[co, 0.0, -si], [0.0, 1.0, 0.0], [si, 0.0, co]])
    proj = d @ rot
    return c, rot, proj.max(axis=0) - proj.min(axis=0)


# ---- the named clouds: name -> (points float32 [n,3], triples int32 [H,3], threshold) -----------------------------------------
def uniform(seed, n):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def random_triples(seed, n, h):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, n, (h, 3))
    for k in range(h):
        while len(set(t[k])) < 3:
            t[k] = rng.integers(0, n, 3)
    return t.astype(np.int32)


def slab(seed, n, tilt_deg=0.0, noise=0.01, half=(1.0, 0.5), outliers=0.0, height=0.1):
    """n points: a noisy plane through (0, height, 0), tilted about x, and a share of uniform outliers in [-1, 1]^3, shuffled"""
    rng = np.random.default_rng(seed)
    n_out = int(round(outliers * n))
    m = n - n_out
    q = np.stack([rng.uniform(-half[0], half[0], m), rng.normal(0.0, noise, m), rng.uniform(-half[1], half[1], m)], axis=1)
    a = np.deg2rad(tilt_deg)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    q = q @ rx.T + np.array([0.0, height, 0.0])
    q = np.concatenate([q, rng.uniform(-1.0, 1.0, (n_out, 3))])
    return q[rng.permutation(n)].astype(np.float32)


def _with_float32_witness(p, triples, threshold):
    """move one row of p until the float64 test and the all-float32 test of hypothesis 0 disagree about it (the float32 mutant
    must be visible on this cloud); the row is not one of hypothesis 0's"""
    p = p.copy()
    p0, nr, valid = hypotheses(p, triples[:1])
    assert valid[0]
    for k in range(len(p) - 1, -1, -1):
        if k in set(int(v) for v in triples[0]):
            continue
        q = p[k].astype(np.float64)
        signed = ((q[0] - p0[0, 0]) * nr[0, 0] + (q[1] - p0[0, 1]) * nr[0, 1]) + (q[2] - p0[0, 2]) * nr[0, 2]
        q = (q + (threshold - signed) * nr[0]).astype(np.float32)
        for axis in (1, 2, 0):
            for direction in (np.float32(np.inf), np.float32(-np.inf)):
                r = q.copy()
                for _ in range(256):
                    r[axis] = np.nextafter(r[axis], direction)
                    d64 = distances(r[None], p0[0], nr[0])[0]
                    d32 = distances_float32(r[None], p0[0], nr[0])[0]
                    if (d64 < threshold) != (float(d32) < threshold):
                        p[k] = r
                        return p
    raise AssertionError("no float32 witness found")


_CLOUDS = None


def clouds():
    global _CLOUDS
    if _CLOUDS is not None:
        return _CLOUDS
    out = {}
    # a slab plus uniform outliers
    p = slab(1, 700, outliers=0.4)
    out["slab_outliers"] = (p, random_triples(2, len(p), 48), 0.05)
    # a slab tilted 5 degrees about x, with a row on which float32 arithmetic decides otherwise (hypothesis 0)
    p = slab(3, 512, tilt_deg=5.0, outliers=0.1)
    t = random_triples(4, len(p), 40)
    on = np.flatnonzero(np.abs(p[:, 1] - 0.1 - np.tan(np.deg2rad(5.0)) * p[:, 2]) < 0.02)
    t[0] = [on[np.argmin(p[on, 0])], on[np.argmax(p[on, 0] + p[on, 2])], on[np.argmax(p[on, 0] - p[on, 2])]]
    out["tilted"] = (_with_float32_witness(p, t, 0.05), t, 0.05)
    # two parallel planes with equal counts, 0.5 apart, at threshold 0.5: each plane's hypothesis counts its own rows only (the
    # other plane lies at the threshold exactly, which is not below it), and the two tie
    g = np.stack(np.meshgrid(np.arange(10) / 8.0, np.arange(10) / 8.0, indexing="ij"), axis=-1).reshape(-1, 2)
    a = np.stack([g[:, 0], np.zeros(len(g)), g[:, 1]], axis=1)
    b = np.stack([g[:, 0], np.full(len(g), 0.5), g[:, 1]], axis=1)
    p = np.concatenate([a, b])[np.random.default_rng(5).permutation(2 * len(g))].astype(np.float32)
    lo, hi = np.flatnonzero(p[:, 1] == 0.0), np.flatnonzero(p[:, 1] == 0.5)

    def corner(rows):
        return [rows[np.argmin(p[rows, 0] + p[rows, 2])], rows[np.argmax(p[rows, 0] - p[rows, 2])], rows[np.argmax(p[rows, 2] - p[rows, 0])]]
    out["planes_tie"] = (p, np.array([corner(hi), corner(lo), corner(hi)[::-1], corner(lo)[::-1]], np.int32), 0.5)
    # a collinear cloud: every hypothesis is invalid (the cross products are exactly zero)
    k = np.arange(-40, 41, dtype=np.float64)
    p = np.stack([k, 2.0 * k, 3.0 * k], axis=1).astype(np.float32) / 16.0
    out["collinear"] = (p, random_triples(6, len(p), 16), 0.05)
    # NaN and inf rows, and triples that touch them
    p = slab(7, 300, outliers=0.3)
    p[5] = [np.nan, 0.0, 0.0]
    p[17] = [0.0, np.inf, 0.0]
    p[200] = [0.1, 0.1, -np.inf]
    p[299] = [np.nan, np.nan, np.nan]
    t = random_triples(8, len(p), 24)
    t[3], t[9], t[11] = [5, 40, 41], [42, 17, 43], [44, 45, 299]
    out["nonfinite"] = (p, t, 0.05)
    # duplicate rows: equal coordinates under distinct indices (a triple of them spans nothing), a repeated index, indices out of range
    p = slab(9, 200, outliers=0.2)
    p = np.concatenate([p, p[:60], p[10:20]])
    t = random_triples(10, len(p), 24)
    t[0], t[1], t[2], t[3], t[4] = [3, 203, 50], [7, 7, 90], [len(p), 1, 2], [4, -1, 6], [12, 212, 262]
    out["duplicates"] = (p, t, 0.05)
    # a mirror-symmetric axis-aligned slab with x-spread above z-spread (the reference's fit_plane_svd agrees with the eigenvector here)
    q = np.abs(np.stack([np.random.default_rng(11).uniform(0.05, 1.0, 64), np.random.default_rng(12).uniform(0.0, 0.01, 64),
                         np.random.default_rng(13).uniform(0.05, 0.5, 64)], axis=1)).astype(np.float32)
    signs = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float32)
    p = (q[None, :, :] * signs[:, None, :]).reshape(-1, 3)
    out["mirror_slab"] = (p, random_triples(14, len(p), 32), 0.05)
    for v in out.values():
        v[0].setflags(write=False)
        v[1].setflags(write=False)
    _CLOUDS = out
    return out
