"""Poisson surface on the host: the twin of csrc/recon_core.h (tests/emu_recon.py) against the numpy /
scipy restatement (tests/recon_ref.py) -- channels, divergence and level exactly, the multigrid solve against a sparse direct
solve within a measured tolerance that two mutants miss -- then a sphere end to end through the host marching cubes, `trim`,
the step order of `mesh_pointcloud` with the GPU calls stubbed, and the twin as a stand-alone sanitizer build.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-re-gen_amd"))

import emu_build
import emu_dmc
import emu_mc
import emu_recon as emu
import recon_ref as R

# the twin's error after the default 10 cycles against scipy's spsolve of the same system, max-norm relative to max |chi|, measured
# on the right-hand sides of _random_b: 3.12e-7 at depth 3, 6.56e-7 at depth 4.  The tests allow four times that.  (The mutants
# land at 1.1e-4 and above.)
SOLVE_MEASURED = {3: 3.12e-7, 4: 6.56e-7}
SOLVE_TOL = {d: 4.0 * v for d, v in SOLVE_MEASURED.items()}
# the largest | |v| - 1 | over the vertices of the depth-5 surface of the 20 000-point unit sphere, measured: 4.49e-3 (h = 7.14e-2)
SPHERE_MEASURED = 4.49e-3
SPHERE_TOL = 2.0 * SPHERE_MEASURED


def _random_b(depth):
    n = R.nodes(depth)
    b = np.zeros((n, n, n), np.float32)
    b[1:-1, 1:-1, 1:-1] = np.random.default_rng(depth).normal(size=(n - 2,) * 3)
    return b, 2.0


def _rel_err(chi, exact):
    return float(np.abs(chi.astype(np.float64) - exact).max() / np.abs(exact).max())


# ---- splat, divergence, level: exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,side", [(2, 4.0), (3, 8.0), (4, 16.0), (3, 2.3)])
def test_channels_equal_the_restatement_exactly(depth, side):
    """h = 1 for the first three boxes, so the cloud's first points sit exactly on nodes and the next on cell faces"""
    centre = (0.0, 0.0, 0.0) if side != 2.3 else (0.3, -1.7, 5.1)
    p, nr = R.edge_cases(depth, centre, side, seed=depth)
    ch, used = emu.splat(p, nr, depth, centre, side)
    ch_ref, used_ref = R.splat(p, nr, depth, centre, side)
    assert used == used_ref == 36
    assert np.array_equal(ch, ch_ref)
    assert np.array_equal(ch, emu.splat(p, nr, depth, centre, side, reverse=True)[0])
    if side != 2.3:
        on_node = p[0]
        at = tuple(np.rint((on_node - (-0.5 * side))).astype(int))
        assert ch[0][at] >= 2 ** 30                                       # a point on a node gives it its whole weight
    b = emu.rhs(ch, depth, centre, side)
    assert np.array_equal(R.bits(b), R.bits(R.rhs(ch, depth, side)))


def test_a_single_point_and_refusals():
    p, nr = np.array([[0.25, 0.5, -0.75]], np.float32), np.array([[0, 0, 3]], np.float32)
    ch, used = emu.splat(p, nr, 3, (0, 0, 0), 8.0)
    assert used == 1 and np.array_equal(ch, R.splat(p, nr, 3, (0, 0, 0), 8.0)[0])
    assert int((ch[0] != 0).sum()) == 8 and ch[1].any() == 0 and ch[2].any() == 0 and (ch[3] == ch[0]).all()
    for depth in (1, 9):
        with pytest.raises(ValueError):
            emu.splat(p, nr, depth, (0, 0, 0), 8.0)
    nan = np.full((3, 3), np.nan, np.float32)
    assert emu.splat(nan, nan, 3, (0, 0, 0), 8.0)[1] == 0


def test_level_sum_equals_the_restatement_exactly():
    depth, centre, side = 4, (0.1, 0.2, -0.3), 3.0
    p, nr = R.edge_cases(depth, centre, side, seed=9)
    field = np.random.default_rng(3).normal(size=(R.nodes(depth),) * 3).astype(np.float32)
    v, s, c = emu.sample(field, depth, centre, side, p, nr)
    v_ref, s_ref, c_ref = R.sample(field, depth, centre, side, p, nr)
    assert (s, c) == (s_ref, c_ref) and c == 36
    assert np.array_equal(R.bits(v), R.bits(v_ref))
    assert emu.sample(field, depth, centre, side, p, nr, reverse=True)[1:] == (s, c)
    ch = emu.splat(p, nr, depth, centre, side)[0]
    d, _, cnt = emu.sample(ch[0], depth, centre, side, p)                  # the density channel; without normals 38 points are finite
    d_ref, _, cnt_ref = R.sample(ch[0], depth, centre, side, p)
    assert cnt == cnt_ref == 38 and np.array_equal(R.bits(d), R.bits(d_ref))


# ---- the solver ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", (3, 4))
def test_solver_against_a_sparse_direct_solve(depth):
    b, side = _random_b(depth)
    exact = R.solve_exact(b, depth, side)
    err = _rel_err(emu.vcycles(b, depth, side, 10), exact)
    print("depth %d: relative max-norm error after 10 cycles %.3e (allowed %.3e)" % (depth, err, SOLVE_TOL[depth]))
    assert err <= SOLVE_TOL[depth]
    for mutant in (1, 2):                                                   # wrong restriction weights; no post-smoothing
        bad = _rel_err(emu.vcycles(b, depth, side, 10, mutant), exact)
        print("  mutant %d: %.3e" % (mutant, bad))
        assert bad > SOLVE_TOL[depth]


@pytest.mark.parametrize("depth", (3, 4))
def test_residual_falls_with_each_of_the_first_six_cycles(depth):
    b, side = _random_b(depth)
    res = [R.residual(emu.vcycles(b, depth, side, c), b, depth, side) for c in range(8)]
    print("residuals", ["%.2e" % r for r in res])
    for c in range(6):
        assert res[c + 1] < res[c]


def test_zero_cycles_is_zero_and_the_boundary_stays_zero():
    b, side = _random_b(3)
    assert not emu.vcycles(b, 3, side, 0).any()
    chi = emu.vcycles(b, 3, side, 3)
    shell = np.ones_like(chi, bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert not chi[shell].any()


# ---- a sphere, end to end ------------------------------------------------------------------------------------------------------
def _sphere_mesh(flip=False, algo="mc"):
    from r3g import recon
    p, nr = R.fibonacci_sphere(20000)
    nr = -nr if flip else nr
    depth = 5
    centre, side, h = recon.box_from_bounds(p.min(0), p.max(0), depth)
    assert np.array_equal(centre, R.box(p, nr, depth)[0]) and side == R.box(p, nr, depth)[1]
    ch, used = emu.splat(p, nr, depth, centre, side)
    chi = emu.vcycles(emu.rhs(ch, depth, centre, side), depth, side, 10)
    _, total, count = emu.sample(chi, depth, centre, side, p, nr)
    level = recon.level_from_sum(total, count)
    xf = recon.lattice_xform(depth, centre, side)
    if algo == "mc":
        v, f, _ = emu_mc.marching_cubes(chi, level, False, xf, recon.REVERSE_FACES["mc"])
    else:
        v, f = emu_dmc.dual_marching_cubes(chi, level, True, xf, recon.REVERSE_FACES["dmc"])[:2]
    return v, f, h, level


def _volume(v, f):
    a, b, c = (v[f[:, i]].astype(np.float64) for i in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def test_sphere_end_to_end():
    v, f, h, level = _sphere_mesh()
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    uniq, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 2).all()                                               # every edge lies in two faces
    assert len(np.unique(f)) - len(uniq) + len(f) == 2                       # Euler number of a sphere
    vol = _volume(v, f)
    assert vol > 0 and abs(vol - 4.0 * np.pi / 3.0) < 0.02
    worst = float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0).max())
    print("largest | |v| - 1 | = %.3e (allowed %.3e, h = %.3e)" % (worst, SPHERE_TOL, h))
    assert SPHERE_TOL < h and SPHERE_MEASURED < h / 2
    assert worst <= SPHERE_TOL
    # all normals reversed: chi and the level change sign exactly, so the surface is the same and only the winding turns
    v2, f2, _, level2 = _sphere_mesh(flip=True)
    assert level2 == -level
    assert np.array_equal(np.unique(v, axis=0), np.unique(v2, axis=0)) and len(f2) == len(f)
    assert _volume(v2, f2) == pytest.approx(-vol, rel=1e-12)


def test_dual_marching_cubes_winds_along_the_normals_too():
    v, f, _, _ = _sphere_mesh(algo="dmc")
    assert _volume(v, f) > 4.0
    v, f, _, _ = _sphere_mesh(flip=True, algo="dmc")
    assert _volume(v, f) < -4.0


def test_box_from_bounds():
    from r3g import recon
    centre, side, h = recon.box_from_bounds((-1, -2, 0), (1, 2, 1), 3)
    assert np.array_equal(centre, [0.0, 0.0, 0.5]) and side == 4.0 * 2.0 and h == 1.0        # (n - 1) / (n - 5) = 2 beats 1.1
    centre, side, h = recon.box_from_bounds((0, 0, 0), (1, 1, 1), 8)
    assert side == pytest.approx(1.1) and h == pytest.approx(1.1 / 256)
    for bad in (1, 9):
        with pytest.raises(ValueError):
            recon.box_from_bounds((0, 0, 0), (1, 1, 1), bad)
    with pytest.raises(ValueError):
        recon.box_from_bounds((1, 1, 1), (1, 1, 1), 4)


# ---- trim and the top layer ----------------------------------------------------------------------------------------------------
def test_trim_on_hand_made_densities():
    from r3g import recon
    from r3g.mesh import Mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0], [5, 5, 5]], np.float64)
    f = np.array([[0, 1, 2], [1, 3, 2], [1, 4, 3]])
    m = Mesh(v, f)
    out = recon.trim(m, np.array([5.0, 5.0, 5.0, 5.0, 0.1, 9.0]), 0.2)      # the quantile is 5.0: vertex 4 alone lies below
    assert np.array_equal(out.faces, [[0, 1, 2], [1, 3, 2]])
    assert np.array_equal(out.vertices, v[:4])                               # vertex 5 was referenced by nothing
    assert m.n_vertices == 6 and m.n_faces == 3                              # the input is left alone
    same = recon.trim(m, np.ones(6), 0.025)                                  # nothing lies below the quantile of equal densities
    assert same.n_faces == 3 and same.n_vertices == 5
    with pytest.raises(ValueError):
        recon.trim(m, np.ones(5))


def _edge_counts(f):
    und, counts = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0, return_counts=True)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return counts, len(np.unique(directed, axis=0)) == len(directed)


def test_fill_pinched_loops_on_two_holes_that_touch():
    """a 5 x 5 lattice of vertices, two cells removed that share the vertex (2, 2) alone: two 4-loops through a pinch vertex"""
    from r3g import recon
    from r3g.mesh import Mesh
    idx = lambda i, j: 5 * i + j
    v = np.array([[i, j, 0] for i in range(5) for j in range(5)], np.float64)
    f = []
    for i in range(4):
        for j in range(4):
            if (i, j) in ((1, 1), (2, 2)):
                continue
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    m = Mesh(v, np.array(f))
    assert recon.fill_pinched_loops(m, max_loop=4) == 2                      # the outer boundary, 16 edges, is left
    assert m.n_vertices == 27 and m.n_faces == 28 + 8
    assert sorted(map(tuple, m.vertices[25:].tolist())) == [(1.5, 1.5, 0.0), (2.5, 2.5, 0.0)]
    counts, wound = _edge_counts(m.faces)
    assert wound and int((counts == 1).sum()) == 16 and counts.max() == 2
    normals = np.cross(m.vertices[m.faces[:, 1]] - m.vertices[m.faces[:, 0]], m.vertices[m.faces[:, 2]] - m.vertices[m.faces[:, 0]])
    assert (normals[:, 2] > 0).all()                                          # the new faces look the way the old ones do
    assert recon.fill_pinched_loops(m, max_loop=4) == 0 and m.n_faces == 36
    assert recon.fill_pinched_loops(Mesh(v, np.array(f)), max_loop=3) == 0   # nothing fits


def test_trimmed_sphere_closes_through_its_pinch_vertices():
    """the 4 096-point sphere at depth 5 on the host twins: the 2.5 % trim leaves holes that touch (tangled for the mesh fill,
    one of them around a patch that hangs on a single vertex); with them closed every edge lies in two faces, wound one way"""
    import emu_meshfill
    from r3g import recon
    from r3g.mesh import Mesh
    p, nr = R.fibonacci_sphere(4096)
    centre, side, _ = R.box(p, nr, 5)
    ch, _ = emu.splat(p, nr, 5, centre, side)
    chi = emu.vcycles(emu.rhs(ch, 5, centre, side), 5, side, 10)
    _, total, count = emu.sample(chi, 5, centre, side, p, nr)
    v, f, _ = emu_mc.marching_cubes(chi, recon.level_from_sum(total, count), False, recon.lattice_xform(5, centre, side), True)
    m = recon.trim(Mesh(v, f), emu.sample(ch[0], 5, centre, side, v)[0], 0.025)
    v2, f2, rep = emu_meshfill.fill_holes(m.vertices, m.faces, 64, "centroid")
    assert rep["tangled"] > 0 and rep["filled"] == rep["loops"]
    m2 = Mesh(v2, f2)
    assert (_edge_counts(m2.faces)[0] == 1).sum() == rep["tangled"]
    assert recon.fill_pinched_loops(m2, 64) >= 2
    counts, wound = _edge_counts(m2.faces)
    assert wound and (counts == 2).all()
    assert _volume(m2.vertices, m2.faces) > 4.0


def test_mesh_pointcloud_runs_the_references_steps_in_order(monkeypatch):
    from r3g import cloud, meshtopo, recon
    from r3g.mesh import Mesh
    calls = []

    class Points:
        shape = (4, 3)

    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])

    def note(name, ret=None):
        def fn(*a, **kw):
            calls.append((name, kw))
            return ret(*a, **kw) if callable(ret) else ret
        return fn

    monkeypatch.setattr(cloud, "_cloud_arg", lambda p, what="points": p)
    monkeypatch.setattr(cloud, "estimate_normals", note("estimate_normals", "normals"))
    monkeypatch.setattr(cloud, "orient_normals", note("orient_normals", ("oriented", {})))
    monkeypatch.setattr(recon, "reconstruct", lambda p, n, depth: calls.append(("reconstruct", {"normals": n, "depth": depth})) or (
        Mesh(v, f), np.ones(4), {"depth": depth, "level": 0.5, "residual": 1e-6, "usable": 4}))
    monkeypatch.setattr(Mesh, "fill_holes", note("fill_holes", True))
    monkeypatch.setattr(Mesh, "_orient", lambda self, outward: calls.append(("_orient", outward)) or 0)
    monkeypatch.setattr(Mesh, "device_buffers", lambda self, device=None: (None, None))
    monkeypatch.setattr(meshtopo, "broken_faces", note("broken_faces", [7, 9]))
    monkeypatch.setattr(Mesh, "simplify_quadric_decimation", lambda self, **kw: calls.append(("simplify", kw)) or self.copy())
    monkeypatch.setattr(Mesh, "process", lambda self, validate=False: calls.append(("process", validate)) or self)
    out = recon.mesh_pointcloud(Points(), depth=5, remesh_percentage=0.25)
    assert [c[0] for c in calls] == ["estimate_normals", "orient_normals", "reconstruct", "fill_holes", "_orient", "_orient",
                                     "broken_faces", "simplify", "process"]
    assert calls[2][1] == {"normals": "oriented", "depth": 5}
    assert calls[3][1] == {"max_loop": 64, "mode": "centroid"}
    assert calls[4][1] == 0 and calls[5][1] == 1                             # fix_winding, then fix_normals(multibody=True)
    assert calls[7][1] == {"percent": 0.25} and calls[8][1] is False
    assert out.metadata["broken_faces"] == 2 and out.metadata["recon"]["depth"] == 5
    # a failing step is reported and skipped, as upstream wraps it
    calls.clear()
    monkeypatch.setattr(Mesh, "fill_holes", lambda self, **kw: (_ for _ in ()).throw(RuntimeError("no")))
    out = recon.mesh_pointcloud(Points(), depth=5)
    assert [c[0] for c in calls][-3:] == ["broken_faces", "simplify", "process"] and out.n_faces == 4


def test_point_cloud_normals_and_to_mesh(monkeypatch):
    from r3g import cloud, recon
    pc = cloud.PointCloud(np.zeros((3, 3)))
    assert pc.normals is None
    pc.normals = [[0, 0, 1]] * 3
    assert pc.normals.shape == (3, 3) and pc.normals.dtype == np.float64
    with pytest.raises(ValueError):
        pc.normals = np.zeros((2, 3))
    with pytest.raises(ValueError):
        cloud.PointCloud(np.zeros((3, 3)), normals=np.zeros((4, 3)))
    seen = {}
    monkeypatch.setattr(recon, "mesh_pointcloud", lambda p, **kw: seen.update(kw=kw, n=tuple(p.shape)) or "mesh")
    assert cloud.PointCloud(np.zeros((5, 3))).to_mesh(device="cpu", depth=4) == "mesh"      # without normals: the reference's function
    assert seen == {"kw": {"depth": 4}, "n": (5, 3)}


def test_twin_as_a_stand_alone_sanitizer_build():
    if not emu_build.sanitizers_link():
        pytest.skip("no sanitizer runtime for g++ on this machine")
    out = subprocess.run([emu.selftest_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
