"""The edge cases of the texture-stage pixel kernels and their checks against tests/tex_truth.py, written once for both users:
tests/test_tex_truth_cpu.py hands in oracle/tex_ref.py (and mutants of it, which must fail), tests/test_tex_edges_gpu.py an
adapter that launches the HIP kernels into guard buffers and compares them with the oracle bit for bit on the way.

`impl` is anything with the oracle's functions (numpy in, numpy out): rasterize, interpolate, view_weight, bake,
bake_gather, bake_finalize, inpaint.  Every check returns (failures: list of str, figures: dict); it never raises for a
wrong result, so that the mutation test can count what each mutant breaks.  Every index array built here is in range."""
import numpy as np

import tex_support as ts
import tex_truth as tt
from oracle import tex_ref

F32 = np.float32
U = tt.U

# excluded share of (pixel, face) pairs per rasteriser scene: measured on the CPU (tests/test_tex_truth_cpu.py prints them,
# profiles/tex_edge_parity.md records them) and capped just above.  With one row or one column no face has an area.
SHARE_CAP = {"soup 1x1": 1.0, "soup 1x7": 1.0, "soup 7x1": 1.0, "soup 1x255": 1.0, "soup 1x257": 1.0, "soup 2x2": 0.12,
             "soup 16x16": 0.03, "soup 17x17": 0.055, "soup 33x200": 0.085, "lattice": 0.05, "box 63": 0.01, "box 64": 0.005,
             "box 65": 0.01, "64 coincident faces": 0.02, "huge face": 0.005, "far vertex": 1.0, "coordinates 1e30": 1.0,
             "w 1e-30, 0, negative": 0.035, "NaN coordinate": 0.06, "z/w at +-1 and beyond": 0.005, "F = 0": 0.0, "F = 1": 0.005}

_TRUTHS = {}


def raster_truth(name):
    """the scene and its truth, computed once per process"""
    if name not in _TRUTHS:
        pos, tri, H, W, expect = ts.raster_edge_scenes_cached()[name]
        _TRUTHS[name] = (pos, tri, H, W, expect, tt.RasterTruth(pos, tri, H, W))
    return _TRUTHS[name]


def share_cap(name):
    for k in (name, name.split(" ")[0], " ".join(name.split(" ")[:2])):
        if k in SHARE_CAP:
            return SHARE_CAP[k]
    raise KeyError(name)


def check_raster_scene(impl, name):
    pos, tri, H, W, expect, truth = raster_truth(name)
    fi, bary = impl.rasterize(pos, tri, H, W)
    fails, m = tt.check_raster(truth, fi, bary, closed=(expect == "closed"))
    m["share"] = truth.excluded_share
    if truth.excluded_share > share_cap(name):
        fails.append("excluded share %.4f above its cap %.4f" % (truth.excluded_share, share_cap(name)))
    covered = int((np.asarray(fi) > 0).sum())
    if expect == "empty" and covered:
        fails.append("%d pixels drawn where nothing can be" % covered)
    if expect == "drawn" and not covered:
        fails.append("nothing drawn")
    if name.startswith("far vertex"):
        # the truth calls this face a sliver (4) and asks nothing of it, so ask here, exactly: a centre more than 0.01 pixel
        # inside all three exact edges is drawn.  (The far vertex is off by thousands of pixels in float32, which moves the
        # edges by that times 16 / 2e10 near the image, and the near vertices by 1e-5 pixel.)
        f = [int(i) for i in tri[0]]
        v = [tt.exact_screen(pos[i], H, W) for i in f]
        for iy in range(H):
            for ix in range(W):
                e = tt.exact_edges(pos, f, H, W, ix, iy)
                deep = all(float(e[k]) > 0.01 * float((v[(k + 1) % 3][0] - v[(k + 2) % 3][0]) ** 2 + (v[(k + 1) % 3][1] - v[(k + 2) % 3][1]) ** 2) ** 0.5
                           for k in range(3))
                if deep and not fi[iy, ix]:
                    fails.append("far vertex: pixel (%d, %d) lies 0.01 pixel inside every exact edge and is empty" % (iy, ix))
        m["far_drawn"] = covered
    if name == "z/w at +-1 and beyond":
        drawn = set(np.unique(fi)) - {0}
        if drawn != {1, 2, 3, 4}:
            fails.append("z/w: faces drawn %s, expected 1-4 (z/w = +-1 and one float beyond stay inside the depth range)" % sorted(drawn))
    if name == "64 coincident faces" and set(np.unique(fi)) - {0} != {1}:
        fails.append("coincident faces: %s drawn, only face 1 may be" % sorted(set(np.unique(fi)) - {0}))
    return fails, m


# ---- interpolate --------------------------------------------------------------------------------------------------
INTERP_CASES = [(C, n) for C in (1, 3, 5, 64) for n in (0, 255, 256, 257)]


def interp_case(C, npix):
    rng = np.random.default_rng(100 * C + npix)
    V, F = 9, 7
    attr = rng.normal(size=(V, C)).astype(F32)
    tri = rng.integers(0, V, (F, 3)).astype(np.int32)
    fi = rng.integers(0, F + 1, npix).astype(np.int32)
    fi[::5] = 0                                       # empty pixels: their rows must come out as zeros
    b = rng.random((npix, 3)).astype(F32)
    b /= np.maximum(b.sum(1, keepdims=True), F32(1e-3))
    return attr, tri, fi, b.astype(F32)


def check_interpolate(impl, C, npix):
    attr, tri, fi, b = interp_case(C, npix)
    out = np.asarray(impl.interpolate(attr, tri, fi, b))
    fails, m = [], {"ratio": 0.0}
    if out.shape != (npix, C):
        return ["shape %s" % (out.shape,)], m
    ref, bound = tt.interpolate_truth(attr, tri, fi, b)
    if npix:
        if np.abs(out[fi == 0]).sum() != 0:
            fails.append("rows of empty pixels are not zero")
        with np.errstate(all="ignore"):
            r = np.abs(out - ref) / np.where(bound > 0, bound, 1)
        r = np.where(bound > 0, r, np.where(out == ref, 0, np.inf))
        m["ratio"] = float(np.nanmax(r)) if not np.isnan(out).any() else np.inf
        if not m["ratio"] <= 1:
            fails.append("error / bound %.3g" % m["ratio"])
    return fails, m


# ---- view weight --------------------------------------------------------------------------------------------------
def view_weight_cases():
    """name -> (findices, depth, normal, cos_threshold, depth_edge, view_w, power, expected centre: "kept" | "zero" | "nan" | None)"""
    out = {}
    up = lambda a: np.nextafter(F32(a), F32(np.inf))   # noqa: E731

    def scene(H, W, normal=(0, 0, 1), centre_normal=None, depth=None):
        fi = np.ones((H, W), np.int32)
        n = np.tile(np.array(normal, F32), (H, W, 1))
        if centre_normal is not None:
            n[H // 2, W // 2] = centre_normal
        d = np.full((H, W), 0.5, F32) if depth is None else depth
        return fi, d, n
    for H, W in ((1, 5), (5, 1), (2, 2)):
        out["%dx%d all border" % (H, W)] = scene(H, W) + (0.1, 0.01, 1.0, 4.0, "allzero")
    out["3x3 one interior"] = scene(3, 3) + (0.1, 0.01, 0.8, 3.0, "kept")
    d = np.full((3, 3), 0.5, F32)
    d[1, 2] = 0.75
    out["depth step == depth_edge"] = scene(3, 3, depth=d) + (0.1, 0.25, 1.0, 2.0, "kept")
    d2 = d.copy()
    d2[1, 2] = up(0.75)
    out["depth step one float more"] = scene(3, 3, depth=d2) + (0.1, 0.25, 1.0, 2.0, "zero")
    out["cos == threshold"] = scene(3, 3, centre_normal=(3, 0, 4)) + (float(F32(0.8)), 0.01, 1.0, 2.0, "kept")
    out["cos one float below threshold"] = scene(3, 3, centre_normal=(3, 0, 4)) + (float(up(0.8)), 0.01, 1.0, 2.0, "zero")
    out["zero-length normal"] = scene(3, 3, centre_normal=(0, 0, 0)) + (0.1, 0.01, 1.0, 2.0, "zero")
    out["NaN normal"] = scene(3, 3, centre_normal=(np.nan, 0, 1)) + (0.1, 0.01, 1.0, 2.0, "zero")
    out["negative cos, fractional power"] = scene(3, 3, centre_normal=(0, 0, -1)) + (-1.0, 0.01, 1.0, 0.5, "nan")
    fi, dd, n = scene(3, 3)
    fi[0, 1] = 0
    out["a neighbour is empty"] = (fi, dd, n, 0.1, 0.01, 1.0, 2.0, "zero")
    return out


def check_view_weight(impl, name):
    fi, d, n, thr, edge, vw, power, expect = view_weight_cases()[name]
    w = np.asarray(impl.view_weight(fi, d, n, thr, edge, vw, power))
    keep, decided, value = tt.view_weight_truth(fi, d, n, thr, edge, vw, power)
    fails, m = [], {}
    if w.shape != fi.shape:
        return ["shape"], m
    got_keep = ~(w == 0)                               # a NaN weight counts as kept (the bakers ignore it)
    if (got_keep != keep)[decided].any():
        fails.append("keep mask differs from the exact rule at %s" % np.argwhere((got_keep != keep) & decided)[0])
    k = keep & decided
    if not np.allclose(w[k], value[k], rtol=2e-6, atol=0, equal_nan=True):
        fails.append("value outside rtol 2e-6 of view_w cos^power")
    c = w[fi.shape[0] // 2, fi.shape[1] // 2]
    if expect == "allzero" and np.abs(w).sum() != 0:
        fails.append("a border pixel has a weight")
    if expect == "kept" and not c > 0:
        fails.append("centre dropped (%r)" % c)
    if expect == "zero" and c != 0:
        fails.append("centre kept (%r)" % c)
    if expect == "nan" and not np.isnan(c):
        fails.append("centre is %r, the power of a negative cosine is NaN" % c)
    return fails, m


# ---- bake ---------------------------------------------------------------------------------------------------------
BAKE_T = (1, 2, 3, 64)
WEIGHTS = [2.0 ** -18, 2.0 ** -17, 65535.0, 1e9, np.inf, 0.0, -1.0, np.nan, 1.0, 0.5]


def _own_face_pixels(u, v):
    """pixel i is covered by a face of its own whose three UV corners are all (u_i, v_i), barycentrics (1, 0, 0): its texture
    coordinate is u_i exactly"""
    n = len(u)
    uv = np.stack([u, v], 1).astype(F32)
    uv_tri = np.repeat(np.arange(n, dtype=np.int32)[:, None], 3, 1)
    bary = np.tile(np.array([1, 0, 0], F32), (n, 1))
    return uv, uv_tri, np.arange(1, n + 1, dtype=np.int32), bary


def bake_case(T):
    us = [0.0, 1.0, -0.5, 1.5, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.3]
    if T == 2:
        us += [0.5, 0.499, 0.501]                                               # u (T-1) + 1/2 == 1 exactly: rounds up
    if T == 3:
        us += [0.25, 0.75, 0.249, 0.251, 0.749, 0.751]                          # exactly on a k + 1/2 boundary (rounds up), and either side
    if T == 64:
        us += [(k + 0.5) / 63 + s * 1e-4 for k in (0, 31, 62) for s in (-1, 1)]  # either side of a k + 1/2 boundary
    u = np.array([a for a in us for _ in WEIGHTS], F32)
    w = np.array([b for _ in us for b in WEIGHTS], F32)
    v = np.roll(u, 3 * len(WEIGHTS))
    rng = np.random.default_rng(T)
    img = rng.random((len(u), 3), dtype=F32)                                      # k 2^-24: c 2^16 + 1/2 is exact in float32
    img[1::7, 0], img[2::7, 1], img[3::7, 2], img[4::11, 1] = -0.5, 1.5, np.nan, 0.25
    return (img, w) + _own_face_pixels(u, v)


def many_into_one_case():
    """4096 pixels into the centre texel of a 3 x 3 texture"""
    n = 4096
    u = np.full(n, 0.3, F32)
    img = np.repeat((np.arange(n, dtype=np.float64) / n).astype(F32)[:, None], 3, 1)
    return (img, np.full(n, 0.75, F32)) + _own_face_pixels(u, u)


def _acc_equal(acc, truth_acc):
    got = np.asarray(acc).astype(np.uint64).astype(object)
    return bool((got == truth_acc).all())


def check_bake(impl, T):
    img, w, uv, uv_tri, fi, bary = bake_case(T)
    acc = impl.bake(img, w, fi, bary, uv, uv_tri, T)
    want, near = tt.bake_truth(img, w, fi, bary, uv, uv_tri, T)
    fails = []
    if near:
        fails.append("the case puts %d texture coordinates next to a rounding boundary (a mistake of the test)" % near)
    if not _acc_equal(acc, want):
        d = np.argwhere(np.asarray(acc).astype(np.uint64).astype(object) != want)
        fails.append("accumulators differ from the closed-form integer sums at %d entries, first %s" % (len(d), d[0]))
    return fails, {}


def check_bake_many(impl):
    img, w, uv, uv_tri, fi, bary = many_into_one_case()
    acc = np.asarray(impl.bake(img, w, fi, bary, uv, uv_tri, 3)).astype(np.uint64)
    n, wq = 4096, 3 * 2 ** 14                            # 0.75 2^16
    colour = wq * sum(k * 16 for k in range(n))          # round(k / 4096 2^16) = 16 k
    want = np.zeros((3, 3, 4), object)
    want[...] = 0
    want[1, 1] = [colour, colour, colour, n * wq]
    return ([] if (acc.astype(object) == want).all() else ["4096 pixels into one texel: %s, closed form %s" % (acc[1, 1], want[1, 1])]), {}


# ---- bake_gather --------------------------------------------------------------------------------------------------
def gather_cases():
    """name -> dict of bake_gather arguments.  Texel i is covered by a face of its own whose clip position is clip[i]."""
    out = {}
    up = lambda a: np.nextafter(F32(a), F32(np.inf))   # noqa: E731

    def case(clips, H, W, depth=0.25, eps=0.25, weight=1.0, seed=0):
        clips = np.array(clips, F32)
        T = int(np.ceil(np.sqrt(len(clips))))
        fu = np.zeros(T * T, np.int32)
        fu[:len(clips)] = np.arange(1, len(clips) + 1)
        bu = np.tile(np.array([1, 0, 0], F32), (T * T, 1))
        rng = np.random.default_rng(seed)
        return dict(findices_uv=fu.reshape(T, T), bary_uv=bu.reshape(T, T, 3), clip_uv=clips,
                    uv_tri=np.repeat(np.arange(len(clips), dtype=np.int32)[:, None], 3, 1), image=rng.random((H, W, 3), dtype=F32),
                    weight=np.full((H, W), weight, F32), findices=np.ones((H, W), np.int32), depth=np.full((H, W), depth, F32),
                    depth_eps=eps)
    out["1x1 view"] = case([[0.3, -0.2, 0.1, 1], [5, 5, 0.1, 1], [-0.9, 0.9, 0.4, 2], [0, 0, 0.9, 1]], 1, 1)
    # 4 x 4 view: x = 0 lands on sx = 2.0 (a pixel border), x = 1 on 3.5 (the centre of the last column: the bilinear
    # neighbour 4 is clamped to 3), x = -1 on 0.5, beyond +-1 outside
    xs = [0.0, 1.0, -1.0, 1.2, -1.2, 1.5, -1.5, 0.37, float(np.nextafter(F32(1), F32(2)))]
    out["borders and last row/column"] = case([[x, y, 0.1, 1] for x in xs for y in xs], 4, 4, seed=1)
    out["z == depth + eps and one float more"] = case([[0.1, 0.1, 0.5, 1], [0.1, 0.1, up(0.5), 1], [0.1, 0.1, 0.25, 1], [0.1, 0.1, 1.0, 2]], 4, 4, seed=2)
    out["w zero, negative, NaN; NaN coordinates"] = case([[0.1, 0.1, 0.1, 0], [0.1, 0.1, 0.1, -1], [0.1, 0.1, 0.1, np.nan], [np.nan, 0.1, 0.1, 1],
                                                          [0.1, np.nan, 0.1, 1], [0.1, 0.1, np.nan, 1], [0.2, 0.2, 0.1, 1], [np.inf, 0, 0.1, 1],
                                                          [1e30, 1e30, 0.1, 1]], 4, 4, seed=3)
    c = case([[2 * (k + 0.2) / 11 - 1, 0.3, 0.1, 1] for k in range(len(WEIGHTS))], 4, 12, seed=4)    # texel k looks at column k
    c["weight"] = np.tile(np.array(WEIGHTS + [1.0, 1.0], F32), (4, 1))           # the view-weight edge values, one per column
    out["weights"] = c
    c = case([[0.2, 0.2, 0.1, 1], [-0.5, 0.5, 0.1, 1], [0.9, -0.9, 0.1, 1]], 4, 4, seed=5)
    c["image"][1, 2, 0] = np.nan                                                  # a NaN colour poisons the samples that touch it
    c["image"][0, 0] = (-0.5, 1.5, 0.5)
    out["colours below 0, above 1, NaN"] = c
    return out


def check_gather(impl, name):
    a = gather_cases()[name]
    acc = np.asarray(impl.bake_gather(a["findices_uv"], a["bary_uv"], a["clip_uv"], a["uv_tri"], a["image"], a["weight"], a["findices"],
                                      a["depth"], a["depth_eps"])).astype(np.uint64)
    wq, col, decided = tt.bake_gather_truth(a["findices_uv"], a["bary_uv"], a["clip_uv"], a["uv_tri"], a["image"], a["weight"], a["findices"],
                                            a["depth"], a["depth_eps"])
    fails, m = [], {"undecided": int((~decided).sum())}
    got_w = acc[..., 3].astype(np.int64)
    if (got_w != wq)[decided].any():
        p = np.argwhere((got_w != wq) & decided)[0]
        fails.append("weight channel differs at texel %s: %d, truth %d" % (p, got_w[tuple(p)], wq[tuple(p)]))
    # colour: wq * round(c 2^16), c the float64 bilinear sample; float32 forms it with 6 roundings of values <= max|c|
    cc = np.clip(col, 0, 1)
    tol = wq[..., None] * (1 + 65536 * 8 * U * max(1.0, float(np.nanmax(np.abs(np.nan_to_num(a["image"], nan=0.0))))))
    diff = np.abs(acc[..., :3].astype(np.float64) - wq[..., None] * np.floor(cc * 65536 + 0.5))
    ok = decided & (got_w == wq)
    if (diff > tol)[ok].any():
        fails.append("colour channels off by more than one fixed-point step")
    if name == "z == depth + eps and one float more" and (got_w.reshape(-1) > 0).tolist() != [True, False, True, True]:
        # every product of this case is exact in float32 (barycentrics 1, 0, 0), so the truth's rounding margin does not apply
        fails.append("depth test: texels %s took a sample; z == depth + eps is in front, one float more is behind" % (got_w.reshape(-1) > 0).tolist())
    if name == "w zero, negative, NaN; NaN coordinates" and (np.nonzero(got_w.reshape(-1))[0].tolist() != [6]):
        fails.append("texels %s took a sample, only texel 6 has finite coordinates in front of the camera" % np.nonzero(got_w.reshape(-1))[0].tolist())
    return fails, m


# ---- finalize -----------------------------------------------------------------------------------------------------
def finalize_case():
    T = 4
    rng = np.random.default_rng(5)
    acc = np.zeros((T, T, 4), np.uint64)
    w = rng.integers(1, 2 ** 20, (T, T)).astype(np.uint64)
    acc[..., 3] = w
    acc[..., :3] = (rng.random((T, T, 3)) * 65536).astype(np.uint64) * w[..., None]
    acc[0, 0] = (12345, 0, 2 ** 40, 0)                                            # zero weight: texture 0, mask 0
    acc[0, 1] = (2 ** 63 - 1, 2 ** 63 - 2 ** 39, 2 ** 62 + 1, 2 ** 47)            # accumulators next to 2^63
    acc[0, 2] = (2 ** 63 + 2 ** 40, 1, 0, 2 ** 48 - 1)                            # and above it (the top bit is part of the value)
    acc[0, 3] = (1, 65536, 65537, 1)
    return acc


def check_finalize(impl):
    acc = finalize_case()
    tex, mask = impl.bake_finalize(acc)
    want_t, want_m = tt.finalize_truth(acc.astype(object))
    fails, m = [], {}
    if not np.array_equal(np.asarray(mask), want_m):
        fails.append("mask differs")
    tex = np.asarray(tex, F32)
    if np.isnan(tex).any() or (tex < 0).any():
        fails.append("texture has a NaN or a negative value")
    else:
        m["ulps"] = int(tt.ulp_distance(tex, want_t).max())
        if m["ulps"] > 1:
            fails.append("texture %d ulps from the correctly rounded quotient (allowed 1)" % m["ulps"])
    return fails, m


# ---- inpaint ------------------------------------------------------------------------------------------------------
CONST = np.array([0.25, 0.5, 0.75], F32)


def strip(rounds, T=128):
    """a triangle strip of 2 R + 1 faces whose first face alone is seeded: the last vertex is R edges away"""
    V = 2 * rounds + 3
    verts = np.array([[0.1 * (k // 2), 0.1 * (k % 2), 0.01 * k] for k in range(V)], F32)
    tri = np.array([[k, k + 1, k + 2] for k in range(V - 2)], np.int32)
    return verts, tri


def _pulled_texels(uv, uv_tri, face, T):
    """the three texels face `face` takes its corner colours from, by the truth's exact rule"""
    out = []
    for k in range(3):
        cen = [sum(tt.frac(uv[uv_tri[face, j], c]) for j in range(3)) / 3 for c in range(2)]
        t = [tt.texel_exact(tt.frac(uv[uv_tri[face, k], c]) * tt.Fraction(3, 4) + cen[c] / 4, T)[0] for c in range(2)]
        out.append((t[1], t[0]))
    return out


def inpaint_cases():
    """name -> dict(args of inpaint..., expect=...)"""
    out = {}

    def atlas_case(verts, tri, T, seed_faces, dilate=0, paint="pulled"):
        uv, uv_tri = ts.face_atlas(tri, T)
        uvc = np.concatenate([uv * 2 - 1, np.zeros((len(uv), 1), F32), np.ones((len(uv), 1), F32)], 1)
        fu, bu = tex_ref.rasterize(uvc, uv_tri, T, T)
        mask = np.zeros((T, T), np.uint8)
        if paint == "all":
            mask[...] = 1
        for f in seed_faces:                           # only the texels the seeding rule looks at: a rule that looks elsewhere finds nothing
            for y, x in _pulled_texels(uv, uv_tri, f, T):
                mask[y, x] = 1
        tex = np.where(mask[..., None] > 0, CONST, F32(0)).astype(F32)
        return dict(tex=tex, mask=mask, findices_uv=fu, bary_uv=bu, verts=verts, pos_tri=tri, uv=uv, uv_tri=uv_tri, dilate_iters=dilate)
    for R in (7, 8, 9, 16, 17):                        # both sides of the host's batch of 8 rounds, and of two batches
        v, t = strip(R)
        out["strip %d rounds" % R] = atlas_case(v, t, 128, [0])
    v, t = strip(3)
    out["nothing painted"] = atlas_case(v, t, 64, [])
    out["everything painted"] = atlas_case(v, t, 64, [], paint="all")
    out["V = 3, F = 1"] = atlas_case(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32), np.array([[0, 1, 2]], np.int32), 32, [0])
    v2 = v.copy()
    v2[4] = v2[3]                                      # coincident vertices: distance 0, the weight is 1 / 1e-6
    out["coincident vertices"] = atlas_case(v2, t, 64, [0])
    v3 = v.copy()
    v3[-1] = (100, 100, 100)                           # further than the weight's resolution (d^2 > 2048): never reached, and the loop ends
    out["vertex out of reach"] = atlas_case(v3, t, 64, [0])
    t4 = t.copy()
    t4[-1] = (t4[-1][0], t4[-1][0], t4[-1][2])         # a face with a repeated vertex
    out["repeated vertex"] = atlas_case(v, t4, 64, [0])
    for d in (0, 1, 2):                                # the odd count ends in the scratch buffer: the copy back
        out["strip, dilate %d" % d] = atlas_case(v, t, 64, [0], dilate=d)
    for T in (1, 2, 3):                                # dilation at the borders of a tiny texture: one painted texel, nothing covered
        for d in (1, 2):
            mask = np.zeros((T, T), np.uint8)
            mask[0, 0] = 1
            tex = np.where(mask[..., None] > 0, CONST, F32(0)).astype(F32)
            out["T = %d, dilate %d" % (T, d)] = dict(tex=tex, mask=mask, findices_uv=np.zeros((T, T), np.int32), bary_uv=np.zeros((T, T, 3), F32),
                                                    verts=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32), pos_tri=np.array([[0, 1, 2]], np.int32),
                                                    uv=np.array([[0.9, 0.9], [0.95, 0.9], [0.9, 0.95]], F32) if T > 1 else np.full((3, 2), 0.5, F32),
                                                    uv_tri=np.array([[0, 1, 2]], np.int32), dilate_iters=d)
    return out


def check_inpaint(impl, name):
    a = inpaint_cases()[name]
    run = lambda d: impl.inpaint(a["tex"], a["mask"], a["findices_uv"], a["bary_uv"], a["verts"], a["pos_tri"], a["uv"], a["uv_tri"], d)   # noqa: E731
    tex, mask, rounds = run(a["dilate_iters"])
    tex, mask = np.asarray(tex, F32), np.asarray(mask)
    T = mask.shape[0]
    fails, m = [], {"rounds": int(rounds)}
    seeded = tt.seeded_vertices(a["mask"], a["uv"], a["uv_tri"], a["pos_tri"], T)
    seeded = np.concatenate([seeded, np.zeros(len(a["verts"]) - len(seeded), bool)])
    want_rounds, reached = tt.propagation_rounds(seeded, a["verts"], a["pos_tri"])
    if rounds != want_rounds:
        fails.append("%d propagation rounds, the breadth-first distance is %d" % (rounds, want_rounds))
    # before the dilation: painted texels keep mask 1 and their colour; a covered unpainted texel is filled (2) exactly when a
    # reached corner of its face has a positive barycentric; nothing else changes
    if a["dilate_iters"]:
        tex0, mask0, _ = run(0)
        tex0, mask0 = np.asarray(tex0, F32), np.asarray(mask0)
    else:
        tex0, mask0 = tex, mask
    fu, bu = a["findices_uv"], a["bary_uv"]
    tri = np.asarray(a["pos_tri"], np.int64).reshape(-1, 3)
    want = a["mask"].copy()
    cov = (fu > 0) & (a["mask"] == 0)
    t = tri[np.where(fu > 0, fu - 1, 0)]
    fill = cov & ((reached[t] & (bu > 0)).any(-1))
    want[fill] = 2
    if not np.array_equal(mask0, want):
        fails.append("mask before dilation differs from the rule at %d texels" % (mask0 != want).sum())
    want_t, want_m = tt.dilate_truth(np.where(want[..., None] > 0, CONST.astype(np.float64), 0.0), want, a["dilate_iters"])
    if not np.array_equal(mask, want_m):
        fails.append("mask after %d dilation steps differs at %d texels" % (a["dilate_iters"], (mask != want_m).sum()))
    filled = mask > 0
    err = float(np.abs(tex[filled].astype(np.float64) - CONST).max()) if filled.any() else 0.0
    m["const_err"] = err
    if not err <= 2.0 ** -16:
        fails.append("a constant texture moved by %.3g (allowed 2^-16)" % err)
    if not np.array_equal(tex[a["mask"] > 0], a["tex"][a["mask"] > 0]):
        fails.append("a painted texel changed")
    if np.abs(tex[~filled]).sum() != 0:
        fails.append("an unfilled texel is not zero")
    return fails, m
