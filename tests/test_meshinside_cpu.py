"""Point in mesh without a GPU: the host twin of csrc/meshinside_core.h (tests/emu_meshinside.py) against the numpy
restatement of DESIGN.md section 4g (tests/meshinside_ref.py) and against itself (columns == brute force), the properties a
closed surface must show, and the tensor arithmetic of r3g/meshinside.py."""
import numpy as np
import pytest

import emu_meshinside as emu
import meshdist_ref as mref
import meshinside_ref as ref

_CACHE = {}
RHO = float(np.sqrt(399.5))          # the level-0.5 surface of 400 - rho^2


def sphere():
    """the 400 sphere (65^3, 14 936 faces) and the 4 096 lattice points at spacing 1.5 (built once)"""
    if "sphere" not in _CACHE:
        v, f = mref.sphere_mesh_host(400)
        _CACHE["sphere"] = (v, f, ref.sphere_lattice())
    return _CACHE["sphere"]


def sphere_counts(axis):
    """the twin's brute-force counts of the sphere's lattice points (computed once per axis, read-only)"""
    if ("counts", axis) not in _CACHE:
        v, f, p = sphere()
        c = emu.brute(p, v, f, axis)[0]
        c.setflags(write=False)
        _CACHE["counts", axis] = c
    return _CACHE["counts", axis]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_unit_cube_literals(axis):
    from r3g import meshinside  # noqa: F401  (the feature's import: this file fails as a whole without it)
    v, f = ref.cube()
    assert f.shape == (12, 3)
    p = ref.cube_literal_points(axis)
    for count in (emu.brute(p, v, f, axis)[0], emu.grid(p, v, f, axis)[0], ref.crossings(p, v, f, axis)[0]):
        for c, (_, want) in zip(count, ref.CUBE_LITERALS):
            assert (c % 2 == 0 and c >= 0) if want == "even" else c == want, (axis, count)
    if axis == 2:                                       # the literals as the coordinates they are written in
        assert np.array_equal(p, np.array([[0.5, 0.5, 0.5], [0.5, 0.5, -1], [0.5, 0.5, 2], [0, 0, -1], [2, 0.5, 0.5]], np.float32))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_winding_does_not_matter(axis):
    v, f = mref.soup()
    p = mref.many_points(1000)
    flipped = f.copy()
    flipped[::2] = flipped[::2, ::-1]
    assert np.array_equal(emu.brute(p, v, f, axis)[0], emu.brute(p, v, flipped, axis)[0])
    cv, cf = ref.cube()
    q = (np.random.default_rng(0).random((500, 3)) * 2 - 0.5).astype(np.float32)
    q[:100] = np.round(q[:100] * 2) / 2                 # on the faces, edges and diagonals
    half = cf.copy()
    half[:6] = half[:6, ::-1]
    assert np.array_equal(emu.brute(q, cv, cf, axis)[0], emu.brute(q, cv, half, axis)[0])


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("fixture", ["cube", "soup", "sphere"])
def test_twin_equals_the_restatement(fixture, axis):
    if fixture == "cube":
        v, f = ref.cube()
        g = np.arange(-2, 7) * 0.25                     # every point of a lattice through the cube's faces, edges and corners
        p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    elif fixture == "soup":
        v, f = mref.soup()
        p = mref.many_points(4097)
    else:
        v, f, p = sphere()
        assert f.shape == (14936, 3) and p.shape == (4096, 3)
    want, skipped = ref.crossings(p, v, f, axis)
    got = sphere_counts(axis) if fixture == "sphere" else emu.brute(p, v, f, axis)[0]
    assert skipped == 0 and got.dtype == np.int32
    assert np.array_equal(got, want)
    assert want.max() >= 2                              # the fixture does exercise the count


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("resolution", [1, 3, 16, 0])
def test_columns_equal_brute_force(resolution, axis):
    v, f = mref.soup()
    p = mref.many_points(4097)
    want = emu.brute(p, v, f, axis)[0]
    got, info = emu.grid(p, v, f, axis, resolution)
    assert np.array_equal(got, want)
    assert info["resolution"] == (resolution or info["resolution"]) and info["skipped"] == 0
    rev, info_r = emu.grid(p, v, f, axis, resolution, reverse_fill=True)        # the order inside a column decides nothing
    assert np.array_equal(rev, want) and info_r == info
    if resolution == 0:
        assert info["resolution"] < 20 and info["pairs"] <= 8 * len(f)           # floor(sqrt(400)) = 20, backed off: spanning faces
        assert emu.grid(p[:1], v, f, axis, 20)[1]["pairs"] > 8 * len(f)
    if resolution == 16:
        assert info["tests"] < len(p) * len(f) / 4                               # and the columns do prune
    sv, sf, sp = sphere()
    got, info = emu.grid(sp, sv, sf, axis, resolution)
    assert np.array_equal(got, sphere_counts(axis))
    if resolution == 0:
        assert info["resolution"] == 61                                          # floor(sqrt(14936) / 2): halved once


def test_closed_surface_properties_on_the_sphere():
    v, f, p = sphere()
    rho = np.linalg.norm(p.astype(np.float64) - 32, axis=1)
    far = np.abs(rho - RHO) > 1.0
    assert far.sum() > 3000 and (rho[far] < RHO).sum() > 1000
    parity = []
    for axis in range(3):
        c = sphere_counts(axis)
        assert c.min() >= 0 and c.max() <= 2
        par = c % 2 == 1
        assert np.array_equal(par[far], rho[far] < RHO)             # nothing misclassified beyond one voxel of the surface
        parity.append(par)
        below = p.copy()
        below[:, axis] = 5.0                                        # the rays start below the box
        cb = emu.brute(below, v, f, axis)[0]
        assert set(np.unique(cb)) == {0, 2}, np.bincount(cb)        # no odd count
    assert np.array_equal(parity[0], parity[1]) and np.array_equal(parity[0], parity[2])
    inside, agreement = emu.contains(p, v, f, (0, 1, 2))
    assert agreement == 1.0 and np.array_equal(inside, parity[0])


def test_open_mesh_lowers_the_agreement_and_raises_nothing():
    v, f, p = sphere()
    hemi = f[(v[f][:, :, 2] > 32).all(1)]
    assert 0 < len(hemi) < len(f)
    inside, agreement = emu.contains(p, v, hemi, (0, 1, 2))
    assert agreement < 1.0 and inside.dtype == bool
    inside_r, agreement_r = ref.contains(p, v, hemi, (0, 1, 2))
    assert np.array_equal(inside, inside_r) and agreement == agreement_r


def test_bad_inputs():
    v, f = ref.cube()
    p = np.array([[0.25, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.25, np.inf, 0.5], [0.25, 0.5, -np.inf]], np.float32)
    for axis in range(3):
        for c in (emu.brute(p, v, f, axis)[0], emu.grid(p, v, f, axis)[0], ref.crossings(p, v, f, axis)[0]):
            assert c.tolist() == [1, -1, -1, -1]
    # a NaN vertex: its faces are skipped and counted, the rest still answers
    v2 = np.concatenate([v, np.array([[np.nan, 0, 0], [0.2, 0.2, 3], [0.3, 0.2, 3]], np.float32)])
    f2 = np.concatenate([f, np.array([[8, 9, 10]], np.int32)])
    for fn in (lambda a: emu.brute(p, v2, f2, a), lambda a: (lambda r: (r[0], r[1]["skipped"]))(emu.grid(p, v2, f2, a)),
               lambda a: ref.crossings(p, v2, f2, a)):
        c, skipped = fn(2)
        assert skipped == 1 and c.tolist() == [1, -1, -1, -1]
    # a face with zero projected area (a wall along the ray, and a face of three equal vertices) is ignored, not skipped
    v3 = np.concatenate([v, np.array([[0.25, 0.5, 2], [0.25, 0.5, 3], [0.25, 0.5, 4], [0.25, 0.0, 2], [0.25, 1.0, 2], [0.25, 0.5, 5]],
                                     np.float32)])
    f3 = np.concatenate([f, np.array([[8, 9, 10], [11, 12, 13], [8, 8, 8]], np.int32)])
    assert not ref.usable_faces(v3, f3, 2)[1][12:].any()
    for c, skipped in (emu.brute(p[:1], v3, f3, 2), ref.crossings(p[:1], v3, f3, 2)):
        assert skipped == 0 and c.tolist() == [1]
    g, info = emu.grid(p[:1], v3, f3, 2, 4)
    assert g.tolist() == [1] and info["skipped"] == 0
    # a bad index
    for bad_value in (8, -1, 2 ** 31 - 1):
        bad = f.copy()
        bad[5, 1] = bad_value
        with pytest.raises(ValueError):
            emu.brute(p, v, bad, 2)
        with pytest.raises(ValueError):
            emu.grid(p, v, bad, 2)
    with pytest.raises(ValueError):                                 # every face skipped, no face, a bad axis
        emu.brute(p, np.full_like(v, np.nan), f, 2)
    with pytest.raises(ValueError):
        emu.grid(p, v, f[:0], 2)
    with pytest.raises(ValueError):
        emu.grid(p, v, f, 3)
    with pytest.raises(ValueError):
        emu.grid(p, v, f, 2, 1025)


def test_volume_iou_of_nested_boxes():
    a = ref.box_mesh((0, 0, 0), (4, 4, 4))
    b = ref.box_mesh((1, 1, 1), (3, 3, 3))
    for axes in ((0,), (1,), (2,), (0, 1, 2)):
        s = ref.volume_iou(a, b, 8, axes)             # centres 0.25 + 0.5 i: all 512 inside a, 4 per axis strictly inside (1, 3)
        assert (s["in_a"], s["in_b"], s["inter"], s["union"]) == (512, 64, 64, 512) and s["iou"] == 0.125
        assert s["volume_a"] == 64.0 and s["volume_b"] == 8.0 and s["n"] == 8
    far = ref.box_mesh((10, 10, 10), (11, 11, 11))
    s = ref.volume_iou(b, far, 2)                     # disjoint: the 2^3 centres (3.5 or 8.5) over [1, 11]^3 miss both boxes
    assert s["union"] == 0 and s["iou"] == 0.0
    import torch
    from r3g import meshinside
    ax = meshinside.lattice_axis(1.0, 11.0, 4, "cpu")                # the product's lattice is the restatement's
    assert ax.dtype == torch.float32 and np.array_equal(ax.numpy(), ref.lattice((1, 1, 1), (11, 11, 11), 4)[::16, 0])
    lo, hi = np.float32(0.1), np.float32(7.3)
    assert np.array_equal(meshinside.lattice_axis(lo, hi, 37, "cpu").numpy(), ref.lattice((lo,) * 3, (hi,) * 3, 37)[:37, 2])


def test_iou_error_of_the_spheres_is_the_recorded_one():
    import mesh_metrics
    v, f, _ = sphere()
    b, fb = mref.sphere_mesh_host(441)
    s = ref.volume_iou((v, f), (b, fb), 32)
    ratio = abs(mesh_metrics.signed_volume(v, f)) / abs(mesh_metrics.signed_volume(b, fb))
    err = abs(s["iou"] - ratio)
    print("volume_iou restatement, spheres 400 / 441, n = 32: iou %.6f, volume ratio %.6f, error %.4e" % (s["iou"], ratio, err))
    assert (s["inter"], s["union"], s["in_a"], s["in_b"]) == (14832, 17256, 14832, 17256)
    assert err <= ref.IOU_ERR_MEASURED * 1.001 and ref.IOU_TOL == 2 * ref.IOU_ERR_MEASURED


def _scores(src, dst, samples=400, stride=1):
    """both implementations of one direction on host data (every stride-th sample); the nearest face by the distance twin"""
    import torch
    import emu_meshdist
    from r3g import meshdist, meshinside
    tv, tf = torch.from_numpy(src[0]), torch.from_numpy(src[1])
    pts, fidx, w = (x[::stride] for x in meshdist.sample_surface(tv, tf, samples))
    face = emu_meshdist.brute(pts.numpy(), dst[0], dst[1])[1]
    a = ref.normal_direction(fidx.numpy(), w.numpy(), face.astype(np.int64), src, dst)
    b = meshinside.normal_scores(fidx, w, torch.from_numpy(face), (tv, tf), (torch.from_numpy(dst[0]), torch.from_numpy(dst[1])))
    assert a["abs"] == pytest.approx(b["abs"], abs=1e-12) and a["signed"] == pytest.approx(b["signed"], abs=1e-12)
    return b


def test_normal_consistency_of_planes():
    base = ref.plane(0.0)
    s = _scores(base, ref.plane(0.25))                               # parallel, offset by 0.25
    assert s["abs"] == 1.0 and s["signed"] == 1.0
    v, f = ref.plane(0.25)
    s = _scores(base, (v, f[:, ::-1].copy()))                        # the same plane wound the other way
    assert s["abs"] == 1.0 and s["signed"] == -1.0
    s = _scores(base, ref.plane(0.5, axis=0))                        # perpendicular
    assert s["abs"] == 0.0 and s["signed"] == 0.0
    v, f = ref.plane(0.25)                                           # a zero-area nearest face is left out of both sums
    v2 = np.concatenate([v, np.array([[0.5, 0.5, 0.01]] * 1, np.float32)])
    f2 = np.concatenate([f, np.array([[len(v), len(v), len(v)]], np.int32)])
    s = _scores(base, (v2, f2))
    assert s["abs"] == 1.0 and s["signed"] == 1.0


def test_normal_consistency_bound_of_the_spheres_holds_for_the_restatement():
    v, f, _ = sphere()
    b, fb = mref.sphere_mesh_host(441)
    for src, dst in (((v, f), (b, fb)), ((b, fb), (v, f))):
        s = _scores(src, dst, samples=1500, stride=12)         # at least one sample per face: every 12th of ~15 000
        print("normal consistency, concentric spheres:", s)
        assert s["abs"] == pytest.approx(s["signed"], abs=1e-12) and s["abs"] >= ref.NC_MIN
