"""float64 torch restatement of the soft silhouette (include/r3g.h "soft silhouettes"), written from the
definition: every face at every pixel by brute force, a stable sort by depth (ties by face index), the sigmoid blend; the
gradient comes from autograd.  It also holds the named scenes that the CPU and GPU tests share and, per scene, the MARGINS: how
far the scene is from each decision that float32 could take the other way.  Test-only; nothing here is product code."""
import math

import numpy as np
import torch

MIN_AREA = 1e-8
MAX_COORD = 1e15


def default_blur(sigma):
    return math.log(1.0 / 1e-4 - 1.0) * sigma


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def drawn_faces(pos, tri):
    """indices of the faces that are drawn (numpy, on the float32 inputs)"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    keep = []
    for f, (a, b, c) in enumerate(tri):
        if min(a, b, c) < 0 or max(a, b, c) >= len(pos):
            continue
        v = pos[[a, b, c]]
        if not np.all(np.abs(v) <= MAX_COORD):      # NaN compares false
            continue
        area = _edge(v[2, 0], v[2, 1], v[0, 0], v[0, 1], v[1, 0], v[1, 1])
        if abs(area) <= MIN_AREA or np.all(v[:, 2] < 0):
            continue
        keep.append(f)
    return np.array(keep, np.int64)


def render(pos, tri, size, K, sigma, blur_radius, want_margins=False):
    """pos: float64 tensor [V, 3] (may require grad), tri int [F, 3] -> dict(alpha [H, W], face int64 [H, W, K], dist, zbuf
    [H, W, K] float64, margins dict when asked)"""
    H, W = size
    sigma, blur_radius = float(np.float32(sigma)), float(np.float32(blur_radius))
    tri_np = np.asarray(tri, np.int64).reshape(-1, 3)
    ids = drawn_faces(pos.detach().numpy(), tri_np)
    N = H * W
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    px, py = xs.reshape(N, 1), ys.reshape(N, 1)
    face = torch.full((N, K), -1, dtype=torch.int64)
    dist = torch.full((N, K), -1.0, dtype=torch.float64)
    zbuf = torch.full((N, K), -1.0, dtype=torch.float64)
    margins = {"blur": math.inf, "bary": math.inf, "key": math.inf, "depth": math.inf, "t": math.inf, "edge": math.inf, "key_ties": 0}
    if len(ids) == 0:
        out = {"alpha": torch.zeros(H, W, dtype=torch.float64), "face": face.reshape(H, W, K), "dist": dist.reshape(H, W, K), "zbuf": zbuf.reshape(H, W, K)}
        if want_margins:
            out["margins"] = margins
        return out
    v = pos[torch.from_numpy(tri_np[ids])]      # [F, 3, 3]
    x, y, z = [v[:, :, c].unsqueeze(0) for c in range(3)]      # [1, F, 3]
    area = _edge(x[..., 2], y[..., 2], x[..., 0], y[..., 0], x[..., 1], y[..., 1])
    b = torch.stack([_edge(px, py, x[..., 1], y[..., 1], x[..., 2], y[..., 2]) / area,
                     _edge(px, py, x[..., 2], y[..., 2], x[..., 0], y[..., 0]) / area,
                     _edge(px, py, x[..., 0], y[..., 0], x[..., 1], y[..., 1]) / area], -1)      # [N, F, 3]
    c = b.clamp(min=0.0)
    c = c / c.sum(-1, keepdim=True).clamp(min=1e-5)
    pz = (c[..., 0] * z[..., 0] + c[..., 1] * z[..., 1]) + c[..., 2] * z[..., 2]
    inside = (b > 0).all(-1)
    d2s, traws, l2oks = [], [], []
    for e in range(3):
        a, bb = e, (e + 1) % 3
        ex, ey = x[..., bb] - x[..., a], y[..., bb] - y[..., a]
        l2 = ex * ex + ey * ey
        ok = l2 > MIN_AREA
        tr = torch.where(ok, ((px - x[..., a]) * ex + (py - y[..., a]) * ey) / torch.where(ok, l2, torch.ones_like(l2)), torch.ones_like(l2 + px))
        t = tr.clamp(0.0, 1.0)
        dx, dy = px - (x[..., a] + t * ex), py - (y[..., a] + t * ey)
        d2s.append(dx * dx + dy * dy)
        traws.append(tr)
        l2oks.append(ok.expand_as(tr))
    d2 = d2s[0]
    for e in (1, 2):
        d2 = torch.where(d2s[e] < d2, d2s[e], d2)      # the first edge wins a tie
    sdist = torch.where(inside, -d2, d2)
    kept = (inside | (d2 < blur_radius)) & ~(pz < 0)
    key = torch.where(kept, pz.detach(), torch.full_like(pz, math.inf))
    order = torch.sort(key, dim=1, stable=True).indices      # faces ascend inside `ids`, so a depth tie falls to the face index
    top = order[:, :K]
    tk = torch.gather(kept, 1, top)
    kk = top.shape[1]
    fid = torch.from_numpy(ids)[top]
    face[:, :kk] = torch.where(tk, fid, torch.full_like(fid, -1))
    gd, gz = torch.gather(sdist, 1, top), torch.gather(pz, 1, top)
    s = torch.sigmoid(-gd / sigma)
    alpha = 1.0 - torch.where(tk, 1.0 - s, torch.ones_like(s)).prod(1)
    dist = torch.cat([torch.where(tk, gd, torch.full_like(gd, -1.0)), dist[:, kk:]], 1)
    zbuf = torch.cat([torch.where(tk, gz, torch.full_like(gz, -1.0)), zbuf[:, kk:]], 1)
    out = {"alpha": alpha.reshape(H, W), "face": face.reshape(H, W, K), "dist": dist.reshape(H, W, K), "zbuf": zbuf.reshape(H, W, K)}
    if want_margins:
        with torch.no_grad():
            def smallest(t, mask=None):      # the smallest non-zero magnitude (an exact 0 is a tie of the input, listed apart)
                t = t.abs()
                if mask is not None:
                    t = t[mask]
                t = t[t > 0]
                return float(t.min()) if t.numel() else math.inf
            front = ~(pz < 0)
            margins["blur"] = smallest(d2 - blur_radius, front & ~inside) if blur_radius > 0 else math.inf      # (d2 < 0 never holds)
            margins["bary"] = smallest(b)
            margins["depth"] = smallest(pz)
            sk = torch.sort(key, dim=1, stable=True).values[:, :K + 1]
            gaps = sk[:, 1:] - sk[:, :-1]
            fin = torch.isfinite(sk[:, 1:]) & torch.isfinite(sk[:, :-1])
            margins["key"] = smallest(gaps, fin)
            margins["key_ties"] = int((gaps[fin] == 0).sum())
            tr, ok = torch.stack(traws, -1), torch.stack(l2oks, -1)
            near = kept.unsqueeze(-1) & ok
            margins["t"] = min(smallest(tr, near), smallest(tr - 1.0, near))
            ds = torch.sort(torch.stack(d2s, -1), dim=-1).values
            margins["edge"] = smallest(ds[..., 1] - ds[..., 0], kept)
        out["margins"] = margins
    return out


def gradient(pos32, tri, size, K, sigma, blur_radius, grad_alpha):
    """d (sum grad_alpha * alpha) / d pos by autograd -> float64 [V, 3]; a non-finite grad_alpha counts as 0.  (Only the vertices
    of drawn faces enter the computation, so a NaN vertex meets no arithmetic.)"""
    pos = torch.tensor(np.asarray(pos32, np.float32).astype(np.float64).reshape(-1, 3), requires_grad=True)
    ga = torch.tensor(np.asarray(grad_alpha, np.float64))
    ga = torch.where(torch.isfinite(ga), ga, torch.zeros_like(ga))
    alpha = render(pos, tri, size, K, sigma, blur_radius)["alpha"]
    if not alpha.requires_grad:
        return np.zeros(tuple(pos.shape))
    (alpha * ga).sum().backward()
    return pos.grad.numpy()


# ---- named scenes: name -> dict(pos float32 [V, 3], tri int32 [F, 3], size (H, W), K, sigma, blur) ------------------------------
def random_scene(seed, size=(33, 31), F=40, K=8, sigma=0.5, blur=None, zlo=0.5, zhi=3.0, spread=0.45):
    """F triangles, each about a random centre, vertices within `spread` of the image's shorter side"""
    rng = np.random.default_rng(seed)
    H, W = size
    ctr = rng.uniform([-2, -2], [W + 2, H + 2], (F, 1, 2))
    xy = ctr + rng.uniform(-1, 1, (F, 3, 2)) * (spread * max(min(H, W), 4))
    z = rng.uniform(zlo, zhi, (F, 3, 1))
    pos = np.concatenate([xy, z], -1).reshape(-1, 3).astype(np.float32)
    tri = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    return dict(pos=pos, tri=tri, size=size, K=K, sigma=sigma, blur=default_blur(sigma) if blur is None else blur)


def shared_scene(seed, size=(33, 31), n=6, K=8, sigma=0.5, blur=None):
    """a jittered n x n lattice of shared vertices, two faces a cell: every inner vertex has six corners (the gather)"""
    rng = np.random.default_rng(seed)
    H, W = size
    gy, gx = np.meshgrid(np.linspace(1.3, H - 1.7, n), np.linspace(0.8, W - 1.9, n), indexing="ij")
    xy = np.stack([gx, gy], -1) + rng.uniform(-0.3, 0.3, (n, n, 2)) * min(H, W) / n
    pos = np.concatenate([xy, rng.uniform(1, 2, (n, n, 1))], -1).reshape(-1, 3).astype(np.float32)
    tri = []
    for i in range(n - 1):
        for j in range(n - 1):
            a = i * n + j
            tri += [[a, a + 1, a + n], [a + 1, a + n + 1, a + n]]
    return dict(pos=pos, tri=np.array(tri, np.int32), size=size, K=K, sigma=sigma, blur=default_blur(sigma) if blur is None else blur)


def _scene(pos, tri, size, K, sigma, blur):
    return dict(pos=np.array(pos, np.float32).reshape(-1, 3), tri=np.array(tri, np.int32).reshape(-1, 3), size=size, K=K, sigma=sigma, blur=blur)


def named_scenes():
    s = {}
    # one face over the whole image: a box of 65 x 63 pixels, sixteen trips of the backward's 256 slots; sigma so large that the
    # pixels deep inside still carry a gradient
    s["full_cover"] = _scene([[-100, -90, 1], [300, -95, 2], [-110, 310, 3]], [[0, 1, 2]], (63, 65), 4, 2000.0, 9.0)
    s["outside"] = _scene([[-50, -60, 1], [-20, -70, 1], [-30, -15, 1], [100, 100, 1], [140, 90, 1], [120, 150, 1], [3.2, 2.1, 1], [15.7, 4.4, 1.5],
                           [6.1, 14.2, 2]], [[0, 1, 2], [3, 4, 5], [6, 7, 8]], (17, 19), 3, 0.5, 4.0)
    s["behind"] = _scene([[2.2, 3.1, -1], [14.3, 2.7, 2], [7.9, 15.2, 3], [3.1, 1.2, -1], [16.2, 5.1, -2], [9.3, 13.4, 4], [1.7, 2.9, -1], [12.2, 3.3, -2],
                          [6.6, 11.1, -3], [4.4, 4.9, 1], [13.1, 6.2, 1], [8.2, 12.8, 1]], [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]], (17, 19), 4,
                         0.5, 4.0)
    # a face without area, and a sliver with an edge of squared length 2.5e-9 whose area is still 0.04
    s["degenerate"] = _scene([[2, 2, 1], [6, 6, 1], [10, 10, 1], [10, 3, 1], [10.00005, 3, 1], [12.3, 880.2, 1], [3.3, 9.1, 2], [9.2, 8.7, 2], [5.5, 14.9, 2]],
                             [[0, 1, 2], [3, 4, 5], [6, 7, 8]], (17, 19), 3, 0.5, 4.0)
    quads_p, quads_t = [], []
    for i in range(40):      # 40 stacked parallel quads, nearest last: more layers than K
        z, o = 3.0 - 0.05 * i, 0.11 * i      # (tilted, so that the two faces of a quad differ in depth off their diagonal)
        b = 4 * i
        quads_p += [[2.3 + o, 2.1, z], [15.2 + o, 2.6, z + 0.17], [15.6 + o, 14.3, z + 0.26], [2.8 + o, 14.9, z + 0.09]]
        quads_t += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    s["stacked"] = _scene(quads_p, quads_t, (17, 23), 20, 0.5, 4.0)
    s["coincident"] = _scene([[2.2, 3.1, 1.5], [14.3, 2.7, 2], [7.9, 15.2, 3], [2.2, 3.1, 1.5], [14.3, 2.7, 2], [7.9, 15.2, 3], [1.1, 1.3, 4], [16.0, 1.2, 4],
                              [8.0, 16.5, 4]], [[3, 4, 5], [0, 1, 2], [6, 7, 8]], (17, 19), 1, 0.5, 4.0)
    # pixel centres exactly on the shared edge x = 8.5 and on the vertices (8.5, 2.5), (8.5, 12.5): dyadic coordinates
    s["on_edge"] = _scene([[8.5, 2.5, 1], [8.5, 12.5, 1], [2.5, 7.5, 1], [14.5, 7.5, 2]], [[0, 2, 1], [0, 1, 3]], (16, 17), 2, 0.5, 4.0)
    s["on_edge_blur0"] = dict(s["on_edge"], blur=0.0)
    # pixel centres at distance exactly 2 from the edge x = 10.5, blur_radius exactly 4
    s["blur_tie"] = _scene([[10.5, 0.5, 1], [10.5, 20.5, 1], [2.5, 10.5, 1]], [[0, 1, 2]], (21, 17), 2, 1.0, 4.0)
    s["blur0"] = random_scene(11, blur=0.0)
    s["saturate"] = random_scene(12, sigma=1e-12, blur=4.0)
    s["wide_blur"] = random_scene(13, size=(33, 31), F=12, sigma=3.0, blur=25.0, spread=0.2)
    s["sharp"] = random_scene(14, sigma=0.02, blur=4.0)
    return s
