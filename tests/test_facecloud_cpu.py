"""Face-to-cloud distance on the CPU: the host twin of csrc/facecloud_core.h (tests/emu_facecloud.py: (a) brute force, (b) the cloud's
grid and the ring walk in host loops) against itself, against the float64 restatement of tests/facecloud_ref.py, against literals
worked out by hand, and against deliberate mutants; the gradient formula against float64 autograd; the stand-alone program under
ASan and UBSan."""
import subprocess

import numpy as np
import pytest

import emu_build
import emu_facecloud as emu
import facecloud_ref as R
import mesh_metrics

RESOLUTIONS = (1, 3, 16, 0)
NAMES = tuple(x[0] for x in R.cpu_fixtures())
UNIT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
ONE = np.array([[0, 1, 2]], np.int32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[:4], b[:4]))


def fixture(name):
    return next(x for x in R.cpu_fixtures() if x[0] == name)[1:]


_BRUTE = {}


def brute(name):
    """twin (a) of a fixture, computed once and left unchanged"""
    if name not in _BRUTE:
        v, f, p = fixture(name)
        out = emu.brute(p, v, f)
        for a in out[:4]:
            a.setflags(write=False)
        _BRUTE[name] = out
    return _BRUTE[name]


# ---- the grid only prunes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_grid_walk_equals_brute_force_bit_for_bit(name):
    """(b) == (a) on dist2, index, weights and diff: every resolution, both fill orders, the narrow and the wide enumeration"""
    v, f, p = fixture(name)
    a = brute(name)
    for res in RESOLUTIONS:
        tests = {}
        for mode in ("narrow", "wide", "device"):
            for rev in (False, True):
                b = emu.grid(p, v, f, res, rev, mode)
                assert same(a, b), (name, res, mode, rev)
                assert b[4]["usable"] == a[4]["usable"] == len(f)
                tests.setdefault(mode, b[4]["tests"])
                assert tests[mode] == b[4]["tests"]                     # the order inside a cell decides nothing, not even the work
        assert max(tests.values()) <= a[4]["tests"]


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 4097))
def test_grid_walk_equals_brute_force_on_the_edge_scene(n):
    """the scene of the GPU test: a cloud of one point (a box without extent), of two, NaN points, invalid and degenerate faces"""
    p = R.edge_cloud(n)
    v, f = R.edge_mesh()
    a = emu.brute(p, v, f)
    assert a[4]["usable"] == len(f) - 5 and (a[1][8:13] == -1).all() and (bits(a[0][8:13]) == 0x7fc00000).all()
    assert not bits(a[2][8:13]).any() and not bits(a[3][8:13]).any()
    good = a[1][np.r_[0:8, 13:len(f)]]
    assert (good >= 0).all() and (good < n).all() and (n < 63 or 5 not in good)      # (point 5 is NaN from 63 points on)
    for res in RESOLUTIONS:
        for mode in ("narrow", "wide", "device"):
            assert same(a, emu.grid(p, v, f, res, mode == "wide", mode)), (n, res, mode)


def test_the_placements_of_the_edge_scene():
    """at resolution 16 over the unit cube face 1's box is exactly kWideCells cells and stays narrow, face 2's is one more"""
    p = R.edge_cloud(4097)
    v, f = R.edge_mesh()
    assert emu.wide_cells() == 64
    assert [emu.grid(p, v, f[k:k + 1], 16)[4]["wide"] for k in range(5)] == [0, 0, 1, 1, 0]
    far = emu.grid(p, v, f[4:5], 16)[4]
    lazy = emu.grid(p, v, f[4:5], 16, mutant="stop_without_other")[4]
    assert far["max_ring"] <= 2 and lazy["max_ring"] == 15      # (the other-axes term ends the far face's walk early)


# ---- tri_nearest_w ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_tri_nearest_w_equals_tri_closest_in_bits(name):
    """the same bits of d2 and r as section 4f's tri_closest, on every face against its winner and against 8 more points each; the
    weights are those of r and sum to one"""
    v, f, p = fixture(name)
    rng = np.random.default_rng(5)
    tri = v[f]
    pts = np.concatenate([p[brute(name)[1]][:, None], p[rng.integers(0, len(p), (len(f), 8))]], 1)
    tri = np.repeat(tri[:, None], 9, 1).reshape(-1, 3, 3)
    d2w, rw, w, d2c, rc = emu.tri_pairs(pts.reshape(-1, 3), tri)
    assert np.array_equal(bits(d2w), bits(d2c)) and np.array_equal(bits(rw), bits(rc))
    assert np.array_equal(bits(d2w.reshape(-1, 9)[:, 0]), bits(brute(name)[0]))
    assert (w >= 0).all() and np.abs(w.sum(1) - 1).max() <= 2 ** -22
    back = np.einsum("na,nak->nk", w.astype(np.float64), tri.astype(np.float64))
    assert np.abs(back - rw).max() <= 1e-5 * R.extent(v)


# ---- against float64 --------------------------------------------------------------------------------------------------------------
def test_the_restatement_against_ericson_on_well_shaped_triangles():
    rng = np.random.default_rng(3)
    tri = rng.random((2000, 3, 3))
    e = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    tri = tri[e > 0.1]
    p = rng.random((len(tri), 3)) * 2 - 0.5
    d2, r, w = R.point_triangle(p, tri)
    assert np.abs(np.sqrt(d2) - mesh_metrics.point_triangle_distance(p, tri)).max() <= 1e-12
    assert np.abs(np.einsum("na,nak->nk", w, tri) - r).max() <= 1e-12 and np.abs(w.sum(1) - 1).max() <= 1e-12


def test_twin_against_float64_distances():
    """the measurement behind facecloud_ref.DIST_TOL: prints each fixture's figure, then asserts the recorded constants"""
    worst = 0.0
    for name in NAMES:
        v, f, p = fixture(name)
        o = R.fixture_oracle(name)
        err = float(np.abs(np.sqrt(brute(name)[0].astype(np.float64)) - np.sqrt(o["dist2"])).max()) / R.extent(v, p)
        print("facecloud twin vs float64, %s: %.4e of the extent" % (name, err))
        worst = max(worst, err)
        assert err <= R.DIST_TOL, name
    assert R.DIST_ERR_MEASURED * 0.99 <= worst <= R.DIST_ERR_MEASURED
    assert R.DIST_TOL == 4 * R.DIST_ERR_MEASURED


@pytest.mark.parametrize("name", NAMES)
def test_twin_against_float64_indices(name):
    """the index is the restatement's on every face whose float64 gap exceeds the tolerance; at most 1 % of the faces fall below it"""
    v, f, p = fixture(name)
    o = R.fixture_oracle(name)
    safe = o["gap"] / R.extent(v, p) > R.DIST_TOL
    print("facecloud %s: %d of %d faces below the gap" % (name, int((~safe).sum()), len(f)))
    assert (~safe).mean() <= R.GAP_CAP
    assert np.array_equal(brute(name)[1][safe], o["index"][safe])
    w_err = np.abs(brute(name)[2][safe] - o["weights"][safe]).max()
    d_err = np.abs(brute(name)[3][safe] - o["diff"][safe]).max() / R.extent(v, p)
    print("facecloud %s: weights within %.3e, diff within %.3e of the extent" % (name, w_err, d_err))


# ---- literals that do not rest on the restatement ---------------------------------------------------------------------------------
def both(points, verts, faces):
    a = emu.brute(points, verts, faces)
    for res in (1, 3, 0):
        assert same(a, emu.grid(points, verts, faces, res, mode="narrow")) and same(a, emu.grid(points, verts, faces, res, mode="wide"))
    return a


def test_literal_point_above_the_centroid():
    third = np.float32(1.0) / np.float32(3.0)
    d2, ix, w, df, _ = both(np.array([[third, third, 2.0], [5, 5, 5]], np.float32), UNIT, ONE)
    assert d2[0] == 4.0 and ix[0] == 0
    assert (np.abs(w[0] - third) <= 4 * np.spacing(third)).all()
    assert np.abs(df[0] - [0, 0, 2]).max() <= 1e-7


def test_literal_mirrored_points_and_duplicates_take_the_lower_index():
    p = np.array([[9, 9, 9], [0.25, 0.25, -0.5], [0.25, 0.25, 0.5], [0.25, 0.25, 0.5], [0.25, 0.25, -0.5]], np.float32)
    d2, ix, w, df, _ = both(p, UNIT, ONE)
    assert d2[0] == 0.25 and ix[0] == 1 and df[0].tolist() == [0, 0, -0.5] and w[0].tolist() == [0.5, 0.25, 0.25]
    d2, ix, _, df, _ = both(p[[0, 2, 3, 1]], UNIT, ONE)
    assert d2[0] == 0.25 and ix[0] == 1 and df[0].tolist() == [0, 0, 0.5]


def test_literal_point_on_the_face():
    d2, ix, w, df, _ = both(np.array([[3, 3, 3], [0.25, 0.5, 0.0]], np.float32), UNIT, ONE)
    assert d2[0] == 0.0 and ix[0] == 1 and not df[0].any() and w[0].tolist() == [0.25, 0.25, 0.5]


def test_literal_segment_and_point_triangles():
    v = np.array([[0, 0, 0], [2, 0, 0], [2, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    d2, ix, w, df, rep = both(np.array([[1, 1, 0], [1, 1, 3]], np.float32), v, f)
    assert d2.tolist() == [1.0, 1.0] and ix.tolist() == [0, 0] and rep["usable"] == 2
    assert w[0].tolist() == [0.5, 0.5, 0.0] and df[0].tolist() == [0, 1, 0]
    assert w[1].tolist() == [1.0, 0.0, 0.0] and df[1].tolist() == [0, 0, -1]


def test_literal_edge_bc():
    """closest point on edge bc at s = 1/4: weights (0, 3/4, 1/4)"""
    v = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0]], np.float32)
    d2, ix, w, df, _ = both(np.array([[3, 0.5, 0], [-7, 0, 0]], np.float32), v, ONE)
    assert d2[0] == 1.0 and ix[0] == 0 and w[0].tolist() == [0.0, 0.75, 0.25] and df[0].tolist() == [1, 0, 0]


def test_literal_cloud_of_one_point():
    d2, ix, w, df, _ = both(np.array([[0.25, 0.25, 0.5]], np.float32), UNIT, ONE)
    assert d2[0] == 0.25 and ix[0] == 0 and df[0].tolist() == [0, 0, 0.5]
    nan = np.float32(np.nan)
    d2, ix, _, _, _ = both(np.array([[nan, 0, 0], [0.25, 0.25, 0.5], [0, nan, 0]], np.float32), UNIT, ONE)
    assert d2[0] == 0.25 and ix[0] == 1


# ---- the gradient -----------------------------------------------------------------------------------------------------------------
def _safe_faces(name):
    """faces with a safe gap whose closest point lies well inside (weights away from 0 and 1)"""
    v, f, p = fixture(name)
    o = R.fixture_oracle(name)
    w = o["weights"]
    return (o["gap"] / R.extent(v, p) > R.DIST_TOL) & (w.min(1) > 0.05) & (w.max(1) < 0.95) & (o["dist2"] > 1e-6 * R.extent(v, p) ** 2)


def _grad64(name, sel):
    import torch
    v, f, p = fixture(name)
    o = R.fixture_oracle(name)
    vt = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    ft = torch.tensor(f[sel].astype(np.int64))
    d2 = R.dist2_torch(vt, ft, torch.tensor(p, dtype=torch.float64), torch.tensor(o["index"][sel]))
    assert np.abs(d2.detach().numpy() - o["dist2"][sel]).max() <= 1e-12 * R.extent(v, p) ** 2
    d2.sum().backward()
    return vt.grad.numpy()


def test_gradient_against_float64_autograd():
    """FaceCloudDistance's formula, evaluated by the twin (gather over the corner lists, g = 1 on the chosen faces), against float64
    autograd of the restatement: prints each fixture's relative error, then asserts the recorded constants"""
    worst, total = 0.0, 0
    for name in NAMES:
        v, f, p = fixture(name)
        sel = _safe_faces(name)
        total += int(sel.sum())
        a = brute(name)
        got = emu.gather(len(v), sel.astype(np.float32), a[1], a[2], a[3], *emu.corner_csr(f, len(v)))
        want = _grad64(name, sel)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print("facecloud gradient, %s: %d faces, relative error %.4e" % (name, int(sel.sum()), err))
        worst = max(worst, err)
        assert err <= R.GRAD_TOL, name
    assert total >= 100
    assert R.GRAD_ERR_MEASURED * 0.99 <= worst <= R.GRAD_ERR_MEASURED and R.GRAD_TOL == 4 * R.GRAD_ERR_MEASURED


def test_restatement_against_its_own_central_differences():
    """blob is a soup (every vertex has one corner), so coordinate k of every chosen face moves at once: 18 evaluations"""
    import torch
    v, f, p = fixture("blob")
    o = R.fixture_oracle("blob")
    sel = np.flatnonzero(_safe_faces("blob"))[:40]
    grad = _grad64("blob", sel)[f[sel]]                      # [n, 3, 3]
    pt, ix = torch.tensor(p, dtype=torch.float64), torch.tensor(o["index"][sel])
    ft = torch.tensor(f[sel].astype(np.int64))
    h = 1e-6
    for a in range(3):
        for k in range(3):
            vals = []
            for sign in (1, -1):
                v64 = v.astype(np.float64)
                v64[f[sel, a], k] += sign * h
                vals.append(R.dist2_torch(torch.tensor(v64), ft, pt, ix).numpy())
            num = (vals[0] - vals[1]) / (2 * h)
            assert np.abs(num - grad[:, a, k]).max() <= 1e-7 * max(1.0, np.abs(grad).max())


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
def test_mutants_are_caught():
    """Each deliberate departure of the twin is exposed by a named fixture.  Three of them change an output: the tie rule (the mirrored
    points), the weights of edge bc (the edge-bc literal) and a ring without its corners (blob at resolution 16).  The other three
    cannot change an output while the definition's remaining safeguards are in force -- dropping kBinMargin or the slack only
    tightens bounds that the other one still covers on every fixture found, and dropping the stop rule's other-axes term only walks
    further -- so they are exposed where the device is held to the twin as well: in the report's test count and largest ring."""
    mirror = np.array([[9, 9, 9], [0.25, 0.25, -0.5], [0.25, 0.25, 0.5]], np.float32)
    assert emu.brute(mirror, UNIT, ONE)[1][0] == 1 and emu.brute(mirror, UNIT, ONE, "tie_less_equal")[1][0] == 2
    v = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0]], np.float32)
    edge = np.array([[3, 0.5, 0], [-7, 0, 0]], np.float32)
    assert emu.brute(edge, v, ONE, "swap_bc")[2][0].tolist() == [0.0, 0.25, 0.75]
    assert emu.grid(edge, v, ONE, mutant="swap_bc")[2][0].tolist() == [0.0, 0.25, 0.75]
    bv, bf, bp = fixture("blob")
    clean = emu.grid(bp, bv, bf, 16, mode="narrow")
    assert same(clean, brute("blob"))
    for mode in ("narrow", "wide"):
        assert not same(emu.grid(bp, bv, bf, 16, mode=mode, mutant="ring_without_corners"), brute("blob"))
    for mutant in ("no_bin_margin", "no_slack"):
        got = emu.grid(bp, bv, bf, 16, mode="narrow", mutant=mutant)
        assert got[4]["tests"] < clean[4]["tests"], mutant
    pv, pf, pp = fixture("partial")
    clean = emu.grid(pp, pv, pf, 16, mode="narrow")
    got = emu.grid(pp, pv, pf, 16, mode="narrow", mutant="stop_without_other")
    assert same(got, clean) and got[4]["tests"] > clean[4]["tests"] and got[4]["max_ring"] > clean[4]["max_ring"]


# ---- the stand-alone program under the sanitizers -----------------------------------------------------------------------------------
def test_selftest_program_under_asan_and_ubsan():
    if not emu_build.sanitizers_link():
        pytest.skip("this toolchain does not link -fsanitize=address,undefined")
    exe = emu.selftest_binary(sanitize=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "facecloud_emu lattice: ok" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
