"""Shared inputs of the texture-stage tests (CPU oracle tests and GPU parity tests use the same scenes)."""
import numpy as np


def icosphere(level=2):
    """unit icosphere: vertices float32 [V, 3], faces int32 [F, 3] (closed manifold, outward winding)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
                  [8, 6, 7], [9, 8, 1]], np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        cache, nf, verts = {}, [], list(v)

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = (verts[a] + verts[b]) / 2.0
                verts.append(m / np.linalg.norm(m))
                cache[k] = len(verts) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(verts), np.array(nf, np.int64)
    return v.astype(np.float32), f.astype(np.int32)


def random_soup(nv, nf, seed, perspective=True):
    """random clip-space triangles, some off screen, some behind the near plane, one duplicated (depth tie)"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.3, 1.3, (nv, 3)).astype(np.float32)
    w = (rng.uniform(0.5, 2.0, (nv, 1)) if perspective else np.ones((nv, 1))).astype(np.float32)
    pos = np.concatenate([xyz * w, w], axis=1).astype(np.float32)
    tri = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int32)
    tri[-1] = tri[0]                      # an exact duplicate: the smaller face index must win everywhere
    tri[-2] = [tri[1][0], tri[1][0], tri[1][2]]   # degenerate (zero area)
    return pos, tri


def ortho_clip(verts, rot, half_extent=1.2):
    """orthographic camera looking down -z of the rotated frame; +y is up -> row 0 at the top; depth in [-1, 1]"""
    p = verts.astype(np.float32) @ rot.astype(np.float32).T
    out = np.ones((len(p), 4), np.float32)
    out[:, 0] = p[:, 0] / np.float32(half_extent)
    out[:, 1] = -p[:, 1] / np.float32(half_extent)
    out[:, 2] = -p[:, 2] / np.float32(2.0 * half_extent)
    return out, p


def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)


def face_atlas(faces, tex_size, pad=1.0):
    """per-face chart atlas: every face gets half of a square cell; -> uv float32 [3F, 2], uv_tri int32 [F, 3]"""
    nf = len(faces)
    cells = (nf + 1) // 2
    side = int(np.ceil(np.sqrt(cells)))
    cell = 1.0 / side
    m = pad / tex_size
    uv = np.zeros((3 * nf, 2), np.float32)
    for f in range(nf):
        c, upper = divmod(f, 2)
        x0, y0 = (c % side) * cell, (c // side) * cell
        if not upper:
            tri = [(x0 + m, y0 + m), (x0 + cell - 2.5 * m, y0 + m), (x0 + m, y0 + cell - 2.5 * m)]
        else:
            tri = [(x0 + cell - m, y0 + cell - m), (x0 + 2.5 * m, y0 + cell - m), (x0 + cell - m, y0 + 2.5 * m)]
        uv[3 * f:3 * f + 3] = tri
    return uv, np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)


# ---- edge scenes of the rasteriser (tests/test_tex_truth_cpu.py and tests/test_tex_edges_gpu.py share them) -------------
def screen_to_clip(X, Y, H, W, z=0.0, w=1.0):
    """clip-space vertex whose screen position is (X, Y) up to float32 rounding (needs H, W >= 2)"""
    x = (np.float64(X) - 0.5) / (W - 1) * 2 - 1
    y = (np.float64(Y) - 0.5) / (H - 1) * 2 - 1
    return np.array([x * w, y * w, z * w, w], np.float64).astype(np.float32)


def lattice_scene(H, W, seed, perspective, step=6):
    """a closed cover of the image whose edges and vertices pass through pixel centres: vertices at pixel centres on a
    `step`-pixel lattice that overhangs the image, interior ones moved by up to 2 pixels, each cell cut along a random diagonal,
    each face wound at random; w in [0.5, 2] when perspective.  A moved corner may land on its cell's diagonal or beyond it (a
    zero-area or folded face); the cell stays a simple quadrilateral, which the two faces of either diagonal always contain,
    so the union still contains the image.  -> pos float32 [V, 4], tri"""
    rng = np.random.default_rng(1000 * seed + 7 * H + W + (1 if perspective else 0))
    nx, ny = -(-(W + step) // step) + 1, -(-(H + step) // step) + 1
    kx, ky = np.meshgrid(np.arange(nx) * step - step, np.arange(ny) * step - step)
    off = rng.integers(-2, 3, (2, ny, nx))
    off[:, [0, -1], :] = 0
    off[:, :, [0, -1]] = 0
    kx, ky = (kx + off[0]).reshape(-1), (ky + off[1]).reshape(-1)
    w = rng.uniform(0.5, 2.0, len(kx)) if perspective else np.ones(len(kx))
    z = rng.uniform(-0.5, 0.5, len(kx))
    pos = np.stack([screen_to_clip(kx[i] + 0.5, ky[i] + 0.5, H, W, z[i], np.float64(np.float32(w[i]))) for i in range(len(kx))])
    tri = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            for t in ([a, b, c], [a, c, d]) if rng.integers(2) else ([a, b, d], [b, c, d]):
                r = int(rng.integers(3))
                t = t[r:] + t[:r]
                tri.append(t[::-1] if rng.integers(2) else t)
    return pos, np.array(tri, np.int32)


def _single(H, W, pts, z=0.0):
    return np.stack([screen_to_clip(x, y, H, W, z) for x, y in pts]), np.array([[0, 1, 2]], np.int32)


def raster_edge_scenes():
    """name -> (pos, tri, H, W, expectation): "closed" (every pixel covered), "empty" (nothing drawn), "drawn" (something
    is), None (whatever the truth allows)"""
    out = {}
    for k, (H, W) in enumerate([(1, 1), (1, 7), (7, 1), (2, 2), (16, 16), (17, 17), (33, 200), (1, 255), (1, 257)]):
        pos, tri = random_soup(12, 10, 40 + k, True)
        pos = np.concatenate([pos, [[-3, -3, 0.9, 1], [5, -3, 0.9, 1], [-3, 5, 0.9, 1]]]).astype(np.float32)   # a backdrop
        tri = np.concatenate([tri, [[12, 13, 14]]]).astype(np.int32)
        # with one row or one column the screen scale W - 1 (H - 1) is 0: every vertex lands on 1/2, no face has an area
        out["soup %dx%d" % (H, W)] = (pos, tri, H, W, "empty" if min(H, W) == 1 else "closed")
    for H, W in ((17, 17), (64, 64), (33, 200)):
        for seed in range(3):
            for persp in (False, True):
                pos, tri = lattice_scene(H, W, seed, persp)
                out["lattice %dx%d seed %d %s" % (H, W, seed, "persp" if persp else "ortho")] = (pos, tri, H, W, "closed")
    for bw, bh in ((9, 7), (8, 8), (13, 5)):        # clamped box of 63, 64, 65 pixels: the 64-lane loop's tail
        pos, tri = _single(16, 16, [(2.25, 3.25), (2.25 + bw - 2.5, 3.75), (3.0, 3.25 + bh - 2.5)])
        out["box %d" % (bw * bh)] = (pos, tri, 16, 16, "drawn")
    pos, _ = _single(16, 16, [(1.5, 1.5), (13.5, 2.5), (3.5, 14.5)], 0.25)
    out["64 coincident faces"] = (pos, np.tile(np.array([[0, 1, 2]], np.int32), (64, 1)), 16, 16, "drawn")
    out["huge face"] = (np.array([[-50, -40, 0, 1], [60, -45, 0, 1], [0, 70, 0, 1]], np.float32), np.array([[0, 1, 2]], np.int32), 16, 16, "closed")
    far = np.array([[-1, -1, 0, 1], [3e9, -1, 0, 1], [-1, 1, 0, 1]], np.float32)
    for name, sx, sy, swap in (("+x", 1, 1, False), ("-x", -1, 1, False), ("+y", 1, 1, True), ("-y", 1, -1, True)):
        p = far.copy()
        if swap:
            p[:, [0, 1]] = p[:, [1, 0]]
        p[:, 0] *= sx
        p[:, 1] *= sy
        out["far vertex " + name] = (p, np.array([[0, 1, 2]], np.int32), 16, 16, "drawn")
    out["coordinates 1e30"] = (np.array([[-1e30, -1, 0, 1], [1e30, -1, 0, 1], [0, 1e30, 0, 1]], np.float32), np.array([[0, 1, 2]], np.int32),
                               16, 16, "empty")
    tiny = np.float32(1e-30)
    pos = np.array([[-0.9, -0.9, 0.5, 1], [0.9, -0.9, 0.5, 1], [-0.9, 0.9, 0.5, 1],                # 0-2: an ordinary face, far
                    [0.3 * tiny, 0.2 * tiny, 0, tiny], [0.5, 0.5, 0, 0], [0.5, 0.5, 0, -1],          # 3: w tiny, 4: w zero, 5: w negative
                    [np.nan, 0.1, 0, 1]], np.float32)                                                # 6: a NaN coordinate
    out["w 1e-30, 0, negative"] = (pos, np.array([[0, 1, 3], [0, 1, 4], [0, 1, 5], [0, 1, 2]], np.int32), 16, 16, "drawn")
    out["NaN coordinate"] = (pos, np.array([[0, 1, 6], [0, 1, 2]], np.int32), 16, 16, "drawn")
    up, dn = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2))
    zs = [1.0, -1.0, up, dn, 1.0001, -1.0001]       # Z = z c + 1/2 with c = 0.49999: the last two leave [0, 1], the others stay
    pos, tri = [], []
    for k, z in enumerate(zs):
        pos += [screen_to_clip(x, y, 16, 24, z) for x, y in ((4 * k + 0.25, 0.25), (4 * k + 3.75, 0.25), (4 * k + 0.25, 15.75))]
        tri.append([3 * k, 3 * k + 1, 3 * k + 2])
    out["z/w at +-1 and beyond"] = (np.stack(pos), np.array(tri, np.int32), 16, 24, "drawn")
    out["F = 0"] = (np.zeros((3, 4), np.float32), np.zeros((0, 3), np.int32), 5, 6, "empty")
    out["F = 1"] = (*_single(5, 6, [(0.25, 0.25), (5.75, 0.25), (0.25, 4.75)]), 5, 6, "drawn")
    return out


_SCENES = []


def raster_edge_scenes_cached():
    if not _SCENES:
        _SCENES.append(raster_edge_scenes())
    return _SCENES[0]
