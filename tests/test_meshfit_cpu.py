"""Mesh registration without a GPU: the host twin (tests/emu_meshfit.py: csrc/meshdist_core.h + csrc/meshfit_core.h in host
loops) against the float64 restatement (tests/meshfit_ref.py) and against known poses of the bean; the solver's corner
cases; the Python surface's argument checks."""
import numpy as np
import pytest

import emu_meshfit as emu
import meshdist_ref as dref
import meshfit_ref as ref

_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def case_points(deg, scale=None, axis=ref.AXIS):
    key = (deg, scale, tuple(axis))
    if key not in _CACHE:
        m = ref.pose(deg, scale, axis)
        p, w = ref.source_points(m, 1000)
        p.setflags(write=False)
        w.setflags(write=False)
        _CACHE[key] = (m, p, w)
    return _CACHE[key]


def restated(deg):
    """the restatement's six plane iterations on every fourth sample (brute force over all faces: seconds), computed once"""
    key = ("icp", deg)
    if key not in _CACHE:
        m, p, w = case_points(deg)
        v, f = ref.bean()
        _CACHE[key] = ref.icp(p[::4], w[::4], v, f, "plane", False, 6)
    return _CACHE[key]


def soup_pairs():
    """(points, triangles) one each: all 4097 points against faces in turn, and every face (the sliver and the
    point-triangle among them) against 64 points"""
    v, f = dref.soup()
    p = dref.many_points(4097)
    fi = np.concatenate([np.arange(len(p)) % len(f), np.repeat(np.arange(len(f)), 64)])
    pp = np.concatenate([p, np.tile(p[:64], (len(f), 1))])
    return pp, v[f[fi]]


def test_bean_is_the_fixture_the_issue_describes():
    v, f = ref.bean()
    assert v.shape == (482, 3) and v.dtype == np.float32 and f.shape == (960, 3)
    tri = v.astype(np.float64)[f]
    assert np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6 > 1.0        # closed, wound outward
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    assert (np.unique(e[:, 0] * 1000 + e[:, 1], return_counts=True)[1] == 2).all()


def test_tri_closest_returns_tri_dist2_bit_for_bit():
    p, tri = soup_pairs()
    d_dist, d_closest, q = emu.tri_closest(p, tri)
    assert len(p) == 4097 + 400 * 64
    assert np.array_equal(bits(d_dist), bits(d_closest))
    assert np.isfinite(q).all()


def test_closest_point_lies_on_the_triangle_and_attains_the_distance():
    p, tri = soup_pairs()
    _, d2, q = emu.tri_closest(p, tri)
    ext = dref.extent(tri.reshape(-1, 3), p)
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    d64 = dref.point_triangle_distance(p64, tri)
    on = dref.point_triangle_distance(q64, tri)                   # distance of the returned point to its triangle
    err_on = float(on.max()) / ext
    err_att = float(np.abs(np.linalg.norm(p64 - q64, axis=1) - d64).max()) / ext
    err_d = float(np.abs(np.sqrt(d2.astype(np.float64)) - d64).max()) / ext
    print("tri_closest vs float64 oracle, of the extent: on-triangle %.3e, attains %.3e, value %.3e (tolerance %.3e)"
          % (err_on, err_att, err_d, dref.DIST_TOL))
    assert err_on <= dref.DIST_TOL and err_att <= dref.DIST_TOL and err_d <= dref.DIST_TOL


def test_mesh_closest_equals_the_distance_twin():
    import emu_meshdist
    v, f = dref.soup()
    p = dref.many_points(600)
    p[17, 1] = np.nan
    a2, af, _ = emu_meshdist.brute(p, v, f)
    for resolution in (0, 1, 5):
        d2, face, q = emu.closest(p, v, f, resolution)
        assert np.array_equal(bits(d2), bits(a2)) and np.array_equal(face, af)
    assert face[17] == -1 and np.isnan(q[17]).all() and np.isfinite(np.delete(q, 17, 0)).all()


def point_sums(p, q, w, c):
    """the point-mode sums of DESIGN.md 4h about the centre c, in numpy"""
    pc, qc = p - c, q - c
    return np.concatenate([[w.sum()], (w[:, None] * pc).sum(0), (w[:, None] * qc).sum(0),
                           (w[:, None, None] * pc[:, :, None] * qc[:, None, :]).sum(0).reshape(-1),
                           [(w * (pc * pc).sum(1)).sum()], [(w * ((p - q) ** 2).sum(1)).sum()]])


@pytest.mark.parametrize("with_scale", [False, True])
def test_solve_point_recovers_a_known_similarity(with_scale):
    rng = np.random.default_rng(3)
    p = rng.standard_normal((200, 3))
    w = rng.random(200) + 0.1
    s = 1.3 if with_scale else 1.0
    r = ref.rotation((0.3, -1.0, 0.5), 71.0)
    t = np.array([0.4, -2.0, 1.5])
    q = s * p @ r.T + t
    c = np.array([0.2, -0.1, 0.3])
    s1, r1, t1, _ = emu.solve(point_sums(p, q, w, c), emu.POINT, with_scale, c)
    assert abs(s1 - s) <= 1e-10 and np.abs(r1 - r).max() <= 1e-10 and np.abs(t1 - t).max() <= 1e-10


def test_solve_point_returns_a_proper_rotation_for_coplanar_and_mirrored_data():
    rng = np.random.default_rng(4)
    w = np.ones(100)
    c = np.zeros(3)
    flat = rng.standard_normal((100, 3)) * (1, 1, 0)
    r = ref.rotation((1, 1, 0.2), 40.0)
    _, r1, t1, _ = emu.solve(point_sums(flat, flat @ r.T + 0.5, w, c), emu.POINT, False, c)
    assert abs(np.linalg.det(r1) - 1.0) <= 1e-12 and np.abs(r1 - r).max() <= 1e-10 and np.abs(t1 - 0.5).max() <= 1e-10
    p = rng.standard_normal((100, 3))
    line = np.outer(rng.standard_normal(100), (1.0, 2.0, 0.5))
    for src, dst in ((p, p * (1, 1, -1)), (p, -p), (flat, flat * (1, -1, 1)), (line, -line), (line, line * 0)):
        for with_scale in (False, True):
            s1, r1, _, _ = emu.solve(point_sums(src, dst, w, c), emu.POINT, with_scale, c)
            assert abs(np.linalg.det(r1) - 1.0) <= 1e-12 and np.abs(r1 @ r1.T - np.eye(3)).max() <= 1e-12 and s1 > 0


def flat_square():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def test_solve_plane_leaves_an_unconstrained_direction_at_zero():
    """a flat square constrains the tilt and the height only: the spin about its normal and the two in-plane shifts stay 0"""
    v, f = flat_square()
    rng = np.random.default_rng(5)
    p0 = np.concatenate([rng.random((300, 2)) * 0.6 + 0.2, np.zeros((300, 1))], 1)
    tilt = ref.pose(4.0, axis=(1.0, 0.5, 0.0), shift=(0.0, 0.0, 0.03))
    p = ref.apply(tilt, p0 - 0.5) + 0.5
    sums, used, centre = emu.step(p.astype(np.float32), v, f, emu.PLANE)
    assert used == 300 and np.allclose(centre, (0.5, 0.5, 0.0))
    s1, r1, t1, dropped = emu.solve(sums, emu.PLANE, False)             # centre 0: the update in the centred frame
    assert dropped == 3 and s1 == 1.0
    assert t1[0] == 0.0 and t1[1] == 0.0 and t1[2] != 0.0               # tau_x, tau_y
    assert r1[1, 0] - r1[0, 1] == 0.0                                    # omega_z
    assert abs(r1[2, 1] - r1[1, 2]) > 1e-3 and abs(r1[0, 2] - r1[2, 0]) > 1e-3
    m, info = emu.fit(p.astype(np.float32), v, f)
    assert info["converged"] and info["rms"] <= 1e-7
    assert np.abs(ref.apply(m, p)[:, 2]).max() <= 1e-6


def test_compose_and_matrix_round_trip():
    a, b = ref.pose(33.0, 1.2), ref.pose(-70.0, 0.8, axis=(0, 1, 0.3), shift=(1, 2, 3))
    assert np.abs(emu.compose(a, b) - a @ b).max() <= 1e-14
    bad = a.copy()
    bad[:3, :3] = bad[:3, :3] * (1, 1, -1)
    assert np.isnan(emu.compose(bad, b)).all()                          # a mirror is not a similarity of this solver
    shear = a.copy()
    shear[0, 1] += 0.1
    assert np.isnan(emu.compose(shear, b)).all()


@pytest.mark.parametrize("deg", [10.0, 25.0])
def test_restatement_recovers_the_pose_with_the_plane_method(deg):
    m = case_points(deg)[0]
    ms = restated(deg)
    errs = [ref.pose_error(x, m) for x in ms]
    print("restatement, plane, %g deg:" % deg, ["%.2e deg %.2e" % e[:2] for e in errs])
    assert errs[-1][0] < 1e-4 and errs[-1][1] < 1e-8


def test_restatement_point_method_creeps_but_improves():
    """from 10 degrees the point method on closest points slides along the surface: it needs hundreds of iterations, so it
    gets its own cap here and only has to improve monotonically"""
    m, p, w = case_points(10.0, 1.05)
    v, f = ref.bean()
    start = ref.pose_error(np.eye(4), m)[0]
    errs = [ref.pose_error(x, m)[0] for x in ref.icp(p[::4], w[::4], v, f, "point", True, 10)]
    print("restatement, point with scale, 10 deg: start %.3f, then" % start, ["%.3f" % e for e in errs])
    assert all(b < a for a, b in zip([start] + errs, errs)) and errs[-1] < start


@pytest.mark.parametrize("name,deg,scale,method,iterations", ref.CASES)
def test_twin_fit_recovers_the_pose_and_agrees_with_the_restatement(name, deg, scale, method, iterations):
    m, p, w = case_points(deg, scale)
    v, f = ref.bean()
    got, info = emu.fit(p, v, f, mode=emu.PLANE if method == "plane" else emu.POINT, with_scale=scale is not None, weights=w,
                        max_iterations=iterations, tolerance=1e-7 if method == "plane" else 0.0)
    err = ref.pose_error(got, m)
    print("twin %s: %d updates, rms %.3e, error %.3e deg %.3e %.3e (tolerance %.1e deg %.1e %.1e, rms %.1e)"
          % ((name, info["iterations"], info["rms"]) + err + ref.FIT_TOL + (ref.RMS_TOL,)))
    assert all(e <= t for e, t in zip(err, ref.FIT_TOL)) and info["rms"] <= ref.RMS_TOL and info["used"] == len(p)
    if method == "plane":
        assert info["converged"] and info["iterations"] <= 8
        want = restated(deg)[-1]
        own = ref.pose_error(want, m)
        assert all(e <= t + o for e, t, o in zip(ref.pose_error(got, want), ref.FIT_TOL, own))


def cube_fit(p, w, v, f):
    """meshfit.align's restart rule on the twin: 4 coarse iterations from each start, the lowest rms refined"""
    import torch
    from r3g import meshfit
    inits = meshfit.cube_inits(torch.from_numpy(p), (torch.from_numpy(v), torch.from_numpy(f)), torch.from_numpy(w))
    coarse = [emu.fit(p, v, f, weights=w, init=i, max_iterations=4) for i in inits]
    best = int(np.argmin([c[1]["rms"] for c in coarse]))
    return emu.fit(p, v, f, weights=w, init=coarse[best][0]), inits


@pytest.mark.parametrize("deg,axis", [(175.0, tuple(ref.AXIS)), (95.0, (0.0, 0.0, 1.0))])
def test_restarts_recover_what_the_identity_start_misses(deg, axis):
    m, p, w = case_points(deg, None, axis)
    v, f = ref.bean()
    got, info = emu.fit(p, v, f, weights=w)
    err = ref.pose_error(got, m)
    print("identity start, %g deg: rms %.3e, %.1f deg off" % (deg, info["rms"], err[0]))
    assert 3e-2 <= info["rms"] <= 5e-2 and err[0] > 170.0              # a local minimum: the bean end for end
    (got, info), inits = cube_fit(p, w, v, f)
    err = ref.pose_error(got, m)
    print("cube_inits, %g deg: rms %.3e, error %.3e deg %.3e" % ((deg, info["rms"]) + err[:2]))
    assert all(e <= t for e, t in zip(err, ref.FIT_TOL)) and info["rms"] <= ref.RMS_TOL
    assert len(inits) == 24


def test_cube_inits_are_the_24_rotations_about_the_centroids():
    import torch
    from r3g import meshfit
    v, f = ref.bean()
    _, p, w = case_points(25.0)
    tp, tw = torch.from_numpy(p), torch.from_numpy(w)
    inits = meshfit.cube_inits(tp, (torch.from_numpy(v), torch.from_numpy(f)), tw)
    rots = np.stack([m[:3, :3] for m in inits])
    assert len(inits) == 24 and np.array_equal(rots[0], np.eye(3))
    assert len({tuple(r.reshape(-1)) for r in rots}) == 24
    assert all(abs(np.linalg.det(r) - 1) < 1e-12 and np.array_equal(np.abs(r).sum(0), np.ones(3)) for r in rots)
    cs = (p.astype(np.float64) * w[:, None]).sum(0) / w.astype(np.float64).sum()
    ct = meshfit.mesh_centroid(torch.from_numpy(v), torch.from_numpy(f))
    tri = v.astype(np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert np.abs(ct - (tri.mean(1) * area[:, None]).sum(0) / area.sum()).max() <= 1e-12
    for m in inits:
        assert np.abs(ref.apply(m, cs) - ct).max() <= 1e-6


def test_weights_max_dist_and_empty_input_in_the_twin():
    m, p, w = case_points(10.0)
    v, f = ref.bean()
    s_all, used_all, _ = emu.step(p, v, f, emu.POINT)
    s_w, used_w, _ = emu.step(p, v, f, emu.POINT, weights=w)
    assert used_all == used_w == len(p) and s_all[0] == len(p) and abs(s_w[0] - w.astype(np.float64).sum()) <= 1e-12
    d2, _, _ = emu.closest(p, v, f)
    cut = float(np.sqrt(np.median(d2.astype(np.float64))))
    s_cut, used_cut, _ = emu.step(p, v, f, emu.POINT, max_dist=cut)
    assert used_cut == int((d2 <= np.float32(cut * cut)).sum()) and 0 < used_cut < len(p) and s_cut[0] == used_cut
    init = ref.pose(12.0, 1.1)
    got, info = emu.fit(p[:0], v, f, init=init)                          # n == 0: the start comes back, nothing used
    assert np.abs(got - init).max() <= 1e-15 and info["used"] == 0 and info["iterations"] == 0 and not info["converged"]
    got, info = emu.fit(p, v, f, weights=w, init=init, max_iterations=0)
    assert np.abs(got - init).max() <= 1e-15 and info["iterations"] == 0 and info["used"] == len(p) and info["rms"] > 1e-3


def test_bad_arguments():
    import torch
    from r3g import meshfit
    m, p, w = case_points(10.0)
    v, f = ref.bean()
    for kw in (dict(mode=2), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_iterations=-1), dict(tolerance=float("nan")),
               dict(init=np.diag([1.0, 1.0, -1.0, 1.0])), dict(init=np.zeros((4, 4)))):
        with pytest.raises(ValueError):
            emu.fit(p, v, f, **kw)
    with pytest.raises(ValueError, match="error -3"):                     # fewer than 3 points within max_dist: defined
        emu.fit(p + np.float32(50.0), v, f, max_dist=0.1)
    with pytest.raises(ValueError, match="error -3"):
        emu.fit(p[:2], v, f)
    tv, tf, tp = torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(p)
    with pytest.raises(ValueError, match="method"):
        meshfit.align(tp, (tv, tf), method="icp")
    with pytest.raises(ValueError, match="not both"):
        meshfit.align(tp, (tv, tf), init=np.eye(4), inits=[np.eye(4)])
    with pytest.raises(ValueError, match="no CPU path"):                  # CPU tensors are refused, not silently handled
        meshfit.align(tp, (tv, tf))
    with pytest.raises(ValueError, match="no CPU path"):
        meshfit.align((tv, tf), (tv, tf))
    with pytest.raises(ValueError):
        meshfit.step(tp, xform=np.zeros(12))


def test_counter_is_listed_and_readable():
    import os
    from r3g import ffi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "r3g.h")).read()
    doc = hdr[hdr.index("/* Process-wide event counters"):hdr.index("int r3g_get_counter(")]
    assert '"meshfit_steps"' in doc and '"meshfit_steps"' in ffi.counter.__doc__
    assert ffi.counter("meshfit_steps") >= 0


def test_mesh_methods():
    """apply_transform is host arithmetic; closest_point and register need the device and say so without one"""
    import torch
    from r3g.mesh import Mesh
    v, f = ref.bean()
    a = Mesh(v, f)
    for name in ("apply_transform", "closest_point", "register"):
        assert callable(getattr(Mesh, name))
    m = ref.pose(25.0, 1.05)
    b = a.copy().apply_transform(m)
    assert np.abs(b.vertices - ref.apply(m, v)).max() <= 1e-12 and np.array_equal(b.faces, a.faces)

    def volume(mesh):
        t = mesh.vertices[mesh.faces]
        return np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6
    mirror = np.diag([1.0, 1.0, -1.0, 1.0])
    c = a.copy().apply_transform(mirror)
    assert np.array_equal(c.faces, a.faces[:, ::-1]) and volume(c) == pytest.approx(volume(a))      # still wound outward
    with pytest.raises(ValueError):
        a.apply_transform(np.eye(3))
    with pytest.raises(ValueError):
        Mesh().register(a)
    with pytest.raises(ValueError):
        Mesh().closest_point(v[:4])
    if torch.cuda.is_available():
        q, d, face = a.closest_point(v[:8])
        assert q.shape == (8, 3) and float(np.abs(d).max()) == 0.0
        assert a.register(b, samples=500)[0].shape == (4, 4)
    else:
        with pytest.raises(RuntimeError, match="no CPU path"):
            a.closest_point(v[:8])
        with pytest.raises(RuntimeError, match="no CPU path"):
            a.register(b)
    import importlib.util
    import os
    import r3g
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(r3g.__file__))), "compat", "trimesh", "__init__.py")
    spec = importlib.util.spec_from_file_location("r3g_compat_trimesh", path)      # under a private name: sys.modules keeps no trimesh
    trimesh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(trimesh)
    assert all(callable(getattr(trimesh.Trimesh, n)) for n in ("register", "apply_transform", "closest_point"))
