"""Mesh distance without a GPU: the host twin of csrc/meshdist_core.h (tests/emu_meshdist.py) against itself (grid walk ==
brute force, bit for bit) and against the float64 oracle (tests/meshdist_ref.py), and the tensor arithmetic of r3g/meshdist.py."""
import math

import numpy as np
import pytest

import emu_meshdist as emu
import meshdist_ref as ref


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_grid_equals_brute(verts, faces, points, resolution, reverse_fill=False):
    a2, af, _ = emu.brute(points, verts, faces)
    b2, bf, info = emu.grid(points, verts, faces, resolution, reverse_fill)
    assert np.array_equal(bits(a2), bits(b2)), resolution
    assert np.array_equal(af, bf), resolution
    return info


@pytest.mark.parametrize("resolution", [1, 4, 16, 0])
def test_grid_walk_equals_brute_force_on_the_soup(resolution):
    v, f = ref.soup()
    p = ref.soup_points()
    info = assert_grid_equals_brute(v, f, p, resolution)
    assert info["resolution"] == (resolution or info["resolution"]) and info["skipped"] == 0
    assert_grid_equals_brute(v, f, p, resolution, reverse_fill=True)     # the order inside a cell decides nothing
    if resolution == 16:
        assert info["tests"] < len(p) * len(f) / 4                       # and the grid does prune


def test_automatic_resolution_backs_off_for_a_spanning_triangle():
    from r3g import meshdist  # noqa: F401  (the feature's import: this file fails as a whole without it)
    v, f = ref.cpu_fixtures()[1][1:3]
    p = ref.cpu_fixtures()[1][3]
    info = assert_grid_equals_brute(v, f, p, 0)
    first = int(math.isqrt(len(f) // 2))                     # floor(sqrt(F / 2)) = 31
    assert first == 31 and info["resolution"] < first        # 31^3 pairs of the spanning triangle alone: backed off
    assert info["pairs"] <= 8 * len(f)
    forced = emu.grid(p, v, f, first)[2]
    assert forced["pairs"] > 8 * len(f)                      # what the back-off avoided


def test_degenerate_triangles_have_a_distance():
    p = np.array([3.0, 4.0, 0.0], np.float32)
    point = np.zeros(9, np.float32)
    assert emu.tri_dist2(p, point) == 25.0                                               # three equal vertices
    seg = np.array([0, 0, 0, 6, 0, 0, 3, 0, 0], np.float32)                                # collinear: the segment [0, 6] x 0
    assert emu.tri_dist2(p, seg) == 16.0
    assert emu.tri_dist2(np.array([-3.0, 4.0, 0.0], np.float32), seg) == 25.0              # beyond its end
    two = np.array([1, 1, 1, 1, 1, 1, 1, 1, 3], np.float32)                                # two equal vertices
    assert emu.tri_dist2(np.array([1.0, 2.0, 2.0], np.float32), two) == 1.0
    tri = np.array([0, 0, 0, 4, 0, 0, 0, 4, 0], np.float32)
    assert emu.tri_dist2(np.array([1.0, 1.0, 2.0], np.float32), tri) == 4.0                # interior
    assert emu.tri_dist2(np.array([2.0, -1.0, 0.0], np.float32), tri) == 1.0               # edge
    assert emu.tri_dist2(np.array([-1.0, -1.0, 1.0], np.float32), tri) == 3.0              # vertex


def test_non_finite_inputs_on_the_twin():
    v, f = ref.soup()
    v = v.copy()
    v[3 * 7] = np.nan                                       # face 7 loses a vertex
    v[3 * 9 + 1, 2] = np.inf
    p = ref.soup_points()[:50].copy()
    p[5, 1] = np.nan
    p[6, 0] = -np.inf
    a2, af, skipped = emu.brute(p, v, f)
    assert skipped == 2 and not np.isin(af, [7, 9]).any()
    assert np.isnan(a2[[5, 6]]).all() and (af[[5, 6]] == -1).all() and np.isfinite(np.delete(a2, [5, 6])).all()
    for res in (1, 5, 0):
        b2, bf, info = emu.grid(p, v, f, res)
        assert info["skipped"] == 2 and np.array_equal(bits(a2), bits(b2)) and np.array_equal(af, bf)
    with pytest.raises(ValueError):
        emu.brute(p, v[:100], f)                            # an index outside [0, V)
    with pytest.raises(ValueError):
        emu.brute(p, np.full_like(v, np.nan), f)            # every face skipped


def test_float32_twin_against_the_float64_oracle():
    """the measurement behind meshdist_ref.DIST_TOL: prints each fixture's figure, then asserts the recorded constants"""
    worst = 0.0
    for name, v, f, p in ref.cpu_fixtures():
        d64, _ = ref.oracle(p, v, f)
        a2, _, _ = emu.brute(p, v, f)
        err = float(np.abs(np.sqrt(a2.astype(np.float64)) - d64).max()) / ref.extent(v, p)
        print("meshdist float32 vs float64, %s: %.3e of the extent" % (name, err))
        assert err <= ref.DIST_TOL, name
        worst = max(worst, err)
    assert worst == pytest.approx(ref.DIST_ERR_MEASURED, rel=0.02)     # the constant is the measurement, not a guess
    assert ref.DIST_TOL == 4 * ref.DIST_ERR_MEASURED


def test_the_oracle_agrees_with_the_closed_form_on_well_shaped_triangles():
    import mesh_metrics
    rng = np.random.default_rng(8)
    tri = rng.random((20000, 3, 3))
    n = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    tri = tri[n > 0.05]                                      # no slivers: there Ericson's form is accurate too
    p = rng.random((len(tri), 3)) * 3 - 1
    assert np.abs(ref.point_triangle_distance(p, tri) - mesh_metrics.point_triangle_distance(p, tri)).max() < 1e-12


def test_sphere_fixture_is_the_one_the_issue_describes():
    v, f = ref.cpu_fixtures()[2][1:3]
    assert v.shape == (7470, 3) and f.shape == (14936, 3)
    r = np.linalg.norm(v.astype(np.float64) - 32, axis=1)
    assert 19.97 < r.min() and r.max() < 20.0


# ---- r3g/meshdist.py: the parts that are plain tensor arithmetic -------------------------------------------------------
def test_summarise_two_and_three_points():
    import torch
    from r3g import meshdist
    s = meshdist.summarise(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 1.0]),
                           torch.tensor([2.0, 4.0, 10.0]), torch.tensor([1.0, 3.0, 0.0]), taus=(2.0, 0.5))
    ab, ba = s["ab"], s["ba"]
    assert ab["mean"] == 2.0 and ab["rms"] == pytest.approx(math.sqrt(5.0)) and ab["max"] == 3.0 and ab["p99"] == 3.0
    assert ab["within"] == {2.0: 0.5, 0.5: 0.0}
    assert ba["mean"] == 3.5 and ba["rms"] == pytest.approx(math.sqrt(13.0)) and ba["max"] == 10.0      # weight 0 counts in max
    assert ba["p99"] == 4.0                                                                               # ... not in p99
    assert ba["within"] == {2.0: 0.25, 0.5: 0.0}
    assert s["chamfer_l1"] == 5.5 and s["chamfer_l2"] == pytest.approx(18.0) and s["hausdorff"] == 10.0
    assert s["fscore"][2.0] == pytest.approx(2 * 0.5 * 0.25 / 0.75) and s["fscore"][0.5] == 0.0
    full = meshdist.summarise(torch.tensor([0.125, 0.25]), torch.tensor([2.0, 1.0]), torch.tensor([0.5]), torch.tensor([1.0]), (0.5,))
    assert full["fscore"][0.5] == 1.0 and full["ab"]["mean"] == pytest.approx(0.5 / 3)


def test_sample_surface_counts_weights_and_positions():
    import torch
    from r3g import meshdist
    v, f = ref.cpu_fixtures()[0][1:3]
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    n = 5000
    pts, face, w = meshdist.sample_surface(tv, tf, n, seed=3)
    tri = v.astype(np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    want = np.maximum(1, np.ceil(area * n / area.sum())).astype(np.int64)
    got = np.bincount(face.numpy(), minlength=len(f))
    assert np.array_equal(got, want) and got.min() >= 1 and len(pts) == want.sum() <= n + len(f)
    assert pts.dtype == torch.float32 and w.dtype == torch.float64
    assert float(w.sum()) == pytest.approx(area.sum(), rel=1e-12)
    assert np.allclose(np.bincount(face.numpy(), weights=w.numpy()), area, rtol=1e-12, atol=0)
    d = ref.point_triangle_distance(pts.numpy().astype(np.float64), tri[face.numpy()])
    assert d.max() <= ref.DIST_TOL * ref.extent(v)                       # every sample on its own face
    again = meshdist.sample_surface(tv, tf, n, seed=3)
    assert torch.equal(pts, again[0]) and not torch.equal(pts, meshdist.sample_surface(tv, tf, n, seed=4)[0])
    big = face.numpy() == int(np.argmax(area))                            # a large face's samples spread over it
    bary_spread = pts.numpy()[big].std(0).max()
    assert bary_spread > 0.3


def test_voxel_size_and_cpu_tensors_are_refused():
    import torch
    from r3g import meshdist
    assert meshdist.voxel_size(1.01, 256) == pytest.approx(2.02 / 257)
    v, f = ref.soup()
    with pytest.raises(ValueError):
        meshdist.nearest(torch.zeros(4, 3), torch.from_numpy(v), torch.from_numpy(f))
