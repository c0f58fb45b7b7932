"""oracle/tex_ref.py against the independent ground truth of tests/tex_truth.py on every edge scene of tests/tex_edge_checks.py
(no GPU: tests/test_tex_edges_gpu.py holds the HIP kernels bit-equal to this oracle and to the same truth), the mutants of
the oracle that the truth must reject, and the parent's coverage rule kept as a function to show what changed."""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import tex_ref  # noqa: E402
import tex_edge_checks as ec  # noqa: E402
import tex_support as ts  # noqa: E402
import tex_truth as tt  # noqa: E402

F32 = np.float32
SCENES = list(ts.raster_edge_scenes_cached())


def all_checks():
    """(label, thunk taking impl) of every check of the suite"""
    out = [("raster: " + n, lambda impl, n=n: ec.check_raster_scene(impl, n)) for n in SCENES]
    out += [("interpolate C %d npix %d" % c, lambda impl, c=c: ec.check_interpolate(impl, *c)) for c in ec.INTERP_CASES]
    out += [("view_weight: " + n, lambda impl, n=n: ec.check_view_weight(impl, n)) for n in ec.view_weight_cases()]
    out += [("bake T %d" % T, lambda impl, T=T: ec.check_bake(impl, T)) for T in ec.BAKE_T]
    out += [("bake 4096 into one", lambda impl: ec.check_bake_many(impl))]
    out += [("bake_gather: " + n, lambda impl, n=n: ec.check_gather(impl, n)) for n in ec.gather_cases()]
    out += [("finalize", lambda impl: ec.check_finalize(impl))]
    out += [("inpaint: " + n, lambda impl, n=n: ec.check_inpaint(impl, n)) for n in ec.inpaint_cases()]
    return out


CHECKS = all_checks()


@pytest.mark.parametrize("label", [c[0] for c in CHECKS])
def test_the_oracle_meets_the_truth(label):
    fails, m = dict(CHECKS)[label](tex_ref)
    print(label, m)
    assert not fails, "\n".join(fails)
    if label.startswith("raster: ") and ec.raster_truth(label[8:])[4] == "closed":
        assert ec.raster_truth(label[8:])[5].may_cover.all()       # the scene is what it claims: its exact union holds every sample
        assert m["holes"] == 0


def test_the_float64_classes_agree_with_exact_rationals():
    """the class of tex_truth (float64 within a covered error) against Fractions on a scene small enough for them"""
    pos, tri, H, W, _, truth = ec.raster_truth("lattice 17x17 seed 1 persp")
    rng = np.random.default_rng(0)
    for f in rng.choice(np.nonzero(~truth.degenerate)[0], 12, replace=False):
        for iy in range(0, H, 2):
            for ix in range(0, W, 2):
                e = tt.exact_edges(pos, [int(i) for i in tri[f]], H, W, ix, iy)
                cls = int(truth.at(np.array(f), np.array(ix + 0.5), np.array(iy + 0.5))["cls"])
                if cls == tt.INSIDE:
                    assert all(v > 0 for v in e)
                elif cls == tt.OUTSIDE:
                    assert any(v < 0 for v in e)
                else:       # ambiguous: within a rounding of an edge, never deep inside or far outside
                    assert min(abs(float(v)) for v in e) < 1e-2


# ---- the parent's coverage rule ---------------------------------------------------------------------------------------
def parent_covers(x, y, area, px, py):
    """what the rasteriser did before the edge functions: the three screen barycentrics, each face dividing by its own area"""
    with np.errstate(all="ignore"):
        b0 = ((x[1] - px) * (y[2] - py) - (x[2] - px) * (y[1] - py)) / area
        b1 = ((x[2] - px) * (y[0] - py) - (x[0] - px) * (y[2] - py)) / area
        b2 = F32(1.0) - b0 - b1
    return (b0 >= 0) & (b1 >= 0) & (b2 >= 0)


@contextlib.contextmanager
def patched(**kw):
    old = {k: getattr(tex_ref, k) for k in kw}
    for k, v in kw.items():
        setattr(tex_ref, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(tex_ref, k, v)


def test_the_new_rule_differs_from_the_parents_only_where_it_may():
    """holes of the parent's rule on the lattice scenes, none with the edge functions; elsewhere the two images differ only
    at pixels where the truth calls one of the two faces ambiguous (counts are printed for profiles/tex_edge_parity.md)"""
    scenes = {n: ts.raster_edge_scenes_cached()[n][:4] for n in SCENES if n.startswith("lattice")}
    for nv, nf, (H, W), persp, seed in [(40, 60, (64, 64), True, 1), (300, 900, (97, 131), True, 2), (50, 80, (33, 200), False, 3),
                                        (3, 3, (16, 16), False, 4)]:          # the scenes of tests/test_tex_gpu.py
        scenes["random_soup %d" % seed] = ts.random_soup(nv, max(nf, 3), seed, persp) + (H, W)
    holes_parent = {(17, 17): 0, (64, 64): 0, (33, 200): 0}
    total = dict(changed=0, filled=0, ambiguous=0)
    for name, (pos, tri, H, W) in scenes.items():
        new, _ = tex_ref.rasterize(pos, tri, H, W)
        with patched(_covers=parent_covers):
            old, _ = tex_ref.rasterize(pos, tri, H, W)
        if name.startswith("lattice"):
            holes_parent[(H, W)] += int((old == 0).sum())
            assert (new > 0).all()
        diff = new != old
        truth = ec.raster_truth(name)[5] if name.startswith("lattice") else tt.RasterTruth(pos, tri, H, W)
        ys, xs = np.nonzero(diff)
        filled = old[ys, xs] == 0
        amb = np.zeros(len(ys), bool)
        for img in (new, old):
            f = img[ys, xs] - 1
            ok = f >= 0
            if ok.any():
                amb[ok] |= truth.at(f[ok], xs[ok] + 0.5, ys[ok] + 0.5)["cls"] == tt.AMBIGUOUS
        assert (filled | amb).all(), "%s: a pixel changed that is neither a hole of the parent nor ambiguous" % name
        print("%-34s changed %4d  holes filled %4d  ambiguous %4d" % (name, diff.sum(), filled.sum(), (amb & ~filled).sum()))
        total["changed"] += int(diff.sum()); total["filled"] += int(filled.sum()); total["ambiguous"] += int((amb & ~filled).sum())   # noqa: E702
    print("parent's holes on the lattice scenes by size:", holes_parent, "totals:", total)
    assert all(v > 0 for v in holes_parent.values())          # the defect: every size shows it


# ---- mutants -------------------------------------------------------------------------------------------------------------
def _mut_exclusive(x, y, area, px, py):
    e0 = tex_ref._edge(x[1], y[1], x[2], y[2], px, py)
    e1 = tex_ref._edge(x[2], y[2], x[0], y[0], px, py)
    e2 = tex_ref._edge(x[0], y[0], x[1], y[1], px, py)
    return np.where(area > 0, (e0 > 0) & (e1 > 0) & (e2 > 0), (e0 < 0) & (e1 < 0) & (e2 < 0))


def _mut_box(lo, hi, n):
    return int(np.maximum(np.floor(lo), F32(0))), int(np.minimum(np.floor(hi), F32(n - 1)))


def _mut_larger_index():
    orig = tex_ref.rasterize

    def rasterize(pos4, tri, H, W):
        tri = np.asarray(tri).reshape(-1, 3)
        fi, bary = orig(pos4, tri[::-1], H, W)
        return np.where(fi > 0, len(tri) + 1 - fi, 0).astype(np.int32), bary
    return rasterize


def _mut_dilate_in_place(tex, mask):
    """Gauss-Seidel: a texel filled earlier in the same sweep already counts as a neighbour"""
    T = mask.shape[0]
    tex, mask = tex.copy(), mask.copy()
    for y in range(T):
        for x in range(T):
            if mask[y, x]:
                continue
            nb = [(yy, xx) for yy in range(max(0, y - 1), min(T, y + 2)) for xx in range(max(0, x - 1), min(T, x + 2))
                  if (yy, xx) != (y, x) and mask[yy, xx]]
            if nb:
                tex[y, x] = sum(tex[p] for p in nb) / F32(len(nb))
                mask[y, x] = 3
    return tex, mask


def mutants():
    orig_screen, orig_texel = tex_ref._screen, tex_ref._texel
    return {
        "exclusive > 0 coverage": dict(_covers=_mut_exclusive),
        "pixel centre without the + 0.5": dict(_centre=lambda i: i.astype(F32)),
        "screen scale W for W - 1": dict(_screen=lambda pos4, tri, H, W: orig_screen(pos4, tri, H + 1, W + 1)),
        "bounding box without the +-1": dict(_box=_mut_box),
        "larger face index on a depth tie": dict(rasterize=_mut_larger_index()),
        "no division by w": dict(_persp=lambda b, w: tuple(b[k] / (b[0] + b[1] + b[2]) for k in range(3))),
        "depth test dropped": dict(_token=lambda depth, f: np.full(depth.shape, f + 1, np.uint64)),
        "floor for round in the texel rule": dict(_texel=lambda u, T: orig_texel(np.asarray(u, F32) - F32(0.5) / F32(max(T - 1, 1)), T)),
        "weight clamp missing": dict(_wq=lambda w: (np.asarray(w, F32).astype(np.float64) * 65536 + 0.5).astype(np.uint64)),
        "dilation reads the current step's state": dict(_dilate_step=_mut_dilate_in_place),
        "seeding from the corner's own texel": dict(_corner_uv=lambda uv, uv_c: (uv[uv_c, 0].astype(F32), uv[uv_c, 1].astype(F32))),
    }


# The bounding box's +-1 is a margin, not a rule.  In exact arithmetic a sample inside a face lies within the extent of its
# vertices, so ix + 1/2 >= min x gives ix >= floor(min x) and ix + 1/2 <= max x gives ix <= floor(max x): the unpadded box
# already holds every sample that can be inside.  In float32 a sample outside that extent has (p - x_k) of one exact sign
# for all three vertices, and no scene here, lattice or soup, has the three rounded edge tests agree on such a sample.  The
# mutant is therefore expected to change NOTHING: that is asserted on every scene, image for image.
EQUIVALENT = {"bounding box without the +-1"}


@pytest.mark.parametrize("name", list(mutants()))
def test_every_mutant_of_the_oracle_fails_the_truth(name):
    with np.errstate(all="ignore"), patched(**mutants()[name]):
        killed = []
        for label, check in CHECKS:
            try:
                fails, _ = check(tex_ref)
            except Exception as e:      # a mutant may also break the oracle outright (an index out of range)
                fails = ["raised %r" % e]
            if fails:
                killed.append("%s: %s" % (label, fails[0]))
    print("%s: fails %d checks; first: %s" % (name, len(killed), killed[:2]))
    if name in EQUIVALENT:
        assert not killed
        for n in SCENES:
            pos, tri, H, W = ts.raster_edge_scenes_cached()[n][:4]
            with patched(**mutants()[name]):
                a = tex_ref.rasterize(pos, tri, H, W)
            b = tex_ref.rasterize(pos, tri, H, W)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    else:
        assert killed, "the mutant %r passes every check" % name


def test_the_box_scenes_hold_63_64_and_65_pixels():
    for n in (63, 64, 65):
        pos, tri, H, W = ts.raster_edge_scenes_cached()["box %d" % n][:4]
        x, y, _, _, _, ok = tex_ref._screen(pos, tri.astype(np.int64), H, W)
        assert ok[0]
        ix0, ix1 = tex_ref._box(x[0].min(), x[0].max(), W)
        iy0, iy1 = tex_ref._box(y[0].min(), y[0].max(), H)
        assert (ix1 - ix0 + 1) * (iy1 - iy0 + 1) == n


def test_no_conversion_of_nan_or_out_of_range_floats():
    """numpy warns ("invalid value encountered in cast") when a NaN or an out-of-range float is converted to an integer:
    the oracle runs every NaN / inf / 1e30 scene with that warning turned into an error"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        for n in ("coordinates 1e30", "NaN coordinate", "w 1e-30, 0, negative", "far vertex +x", "far vertex -y"):
            pos, tri, H, W = ts.raster_edge_scenes_cached()[n][:4]
            with np.errstate(all="ignore"):
                tex_ref.rasterize(pos, tri, H, W)
        with np.errstate(all="ignore"):
            for T in ec.BAKE_T:
                img, w, uv, uv_tri, fi, bary = ec.bake_case(T)
                tex_ref.bake(img, w, fi, bary, uv, uv_tri, T)
            for a in ec.gather_cases().values():
                tex_ref.bake_gather(a["findices_uv"], a["bary_uv"], a["clip_uv"], a["uv_tri"], a["image"], a["weight"], a["findices"], a["depth"],
                                    a["depth_eps"])
