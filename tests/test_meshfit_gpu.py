"""Mesh registration on the GPU (include/r3g.h r3g_meshdist_closest / r3g_meshfit_step / r3g_meshfit, r3g/meshfit.py,
Mesh.register): closest points and the sums of one fused step bit for bit against the host twin (tests/emu_meshfit.py), and
full fits on the bean within the tolerance fixed from the twin (tests/meshfit_ref.py)."""
import ctypes

import numpy as np
import pytest

import emu_meshfit as emu
import meshdist_ref as dref
import meshfit_ref as ref

pytestmark = pytest.mark.gpu

_CACHE = {}
MOVE = np.concatenate([[1.05], ref.rotation(ref.AXIS, 25.0).reshape(-1), ref.SHIFT + 0.2])      # a non-identity xform
CUT = 0.3                                                                                       # a max_dist that excludes some


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def soup():
    """the soup, 4097 points with weights, and the twin's closest points (computed once)"""
    if "soup" not in _CACHE:
        v, f = dref.soup()
        p = dref.many_points(4097)
        w = (np.random.default_rng(9).random(4097) * 2).astype(np.float32)
        out = (v, f, p, w) + emu.closest(p, v, f)
        for a in out:
            a.setflags(write=False)
        _CACHE["soup"] = out
    return _CACHE["soup"]


def bean_case(deg, scale=None, axis=ref.AXIS):
    key = (deg, scale, tuple(axis))
    if key not in _CACHE:
        m = ref.pose(deg, scale, axis)
        _CACHE[key] = (m,) + ref.source_points(m, 1000)
    return _CACHE[key]


def bean_dev():
    if "bean" not in _CACHE:
        v, f = ref.bean()
        _CACHE["bean"] = (dev(v), dev(f, np.int32))
    return _CACHE["bean"]


def gpu_step(p, w, v, f, method, xform=None, max_dist=None, resolution=None):
    from r3g import ffi, meshdist, meshfit
    with ffi.device_lock(0):
        meshdist.build(dev(v), dev(f, np.int32), resolution)
        return meshfit.step(dev(p), xform, None if w is None else dev(w), method, max_dist)


@pytest.mark.parametrize("resolution", [1, 3, 16, None])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_closest_point_equals_the_twin_bit_for_bit(n, resolution):
    from r3g import ffi, meshdist
    v, f, p, _, a2, af, aq = soup()
    with ffi.device_lock(0):
        meshdist.build(dev(v), dev(f, np.int32), resolution)
        d2, face, q = meshdist.closest(dev(p[:n]))
        e2, eface = meshdist.query(dev(p[:n]))
    assert q.dtype == __import__("torch").float32 and tuple(q.shape) == (n, 3)
    assert np.array_equal(bits(d2.cpu().numpy()), bits(a2[:n])) and np.array_equal(face.cpu().numpy(), af[:n])
    assert np.array_equal(bits(q.cpu().numpy()), bits(aq[:n]))
    assert np.array_equal(bits(d2.cpu().numpy()), bits(e2.cpu().numpy())) and np.array_equal(face.cpu().numpy(), eface.cpu().numpy())


def test_closest_point_surface_and_non_finite_points():
    import torch
    from r3g import meshdist
    v, f, p, _, a2, af, aq = soup()
    q = p[:300].copy()
    q[5, 1] = np.nan
    q[64, 0] = -np.inf
    cp, d, face = meshdist.closest_point(dev(q), dev(v), dev(f, np.int32))
    cp, d, face = cp.cpu().numpy(), d.cpu().numpy(), face.cpu().numpy()
    bad = [5, 64]
    assert np.isnan(cp[bad]).all() and np.isnan(d[bad]).all() and (face[bad] == -1).all()
    keep = np.delete(np.arange(300), bad)
    assert np.array_equal(bits(cp[keep]), bits(aq[keep])) and np.array_equal(face[keep], af[keep])
    np.testing.assert_allclose(d[keep], np.sqrt(a2[keep]), rtol=2e-7, atol=0)
    cp, d, face = meshdist.closest_point(torch.zeros((0, 3), device="cuda"), dev(v), dev(f, np.int32))      # N == 0: a no-op
    assert cp.shape == (0, 3) and d.shape == (0,) and face.shape == (0,)
    with pytest.raises(ValueError):
        meshdist.closest_point(torch.from_numpy(q), dev(v), dev(f, np.int32))


@pytest.mark.parametrize("method", ["point", "plane"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_step_sums_equal_the_twin_bit_for_bit(n, method):
    """with and without weights, with and without a max_dist that excludes points, under the identity and a similarity"""
    v, f, p, w = soup()[:4]
    mode = emu.POINT if method == "point" else emu.PLANE
    for weights in (None, w[:n]):
        for max_dist in (None, CUT):
            for xform in (None, MOVE):
                want, used, _ = emu.step(p[:n], v, f, mode, xform, weights, float("inf") if max_dist is None else max_dist)
                got, gused = gpu_step(p[:n], weights, v, f, method, xform, max_dist)
                assert gused == used, (weights is not None, max_dist, xform is not None)
                assert np.array_equal(bits64(got), bits64(want)), (weights is not None, max_dist, xform is not None)
                assert got.shape == (emu.TERMS[mode],)
    if n == 4097:
        full = emu.step(p, v, f, mode, MOVE, w)[1]
        cut = emu.step(p, v, f, mode, MOVE, w, CUT)[1]
        assert 0 < cut < full <= n                                     # the cut did exclude some, and not all


@pytest.mark.parametrize("method", ["point", "plane"])
def test_step_with_more_than_256_block_partials(method):
    """70 001 points: 274 blocks, so the last kernel's lanes 0..17 add two records each before the tree"""
    v, f = soup()[:2]
    p = dref.many_points(70001, seed=6)
    w = (np.random.default_rng(10).random(70001) + 0.5).astype(np.float32)
    mode = emu.POINT if method == "point" else emu.PLANE
    want, used, _ = emu.step(p, v, f, mode, MOVE, w, 2.0)
    got, gused = gpu_step(p, w, v, f, method, MOVE, 2.0)
    assert gused == used and 0 < used < 70001
    assert np.array_equal(bits64(got), bits64(want))


def test_two_runs_are_identical_and_the_resolution_does_not_matter():
    v, f, p, w = soup()[:4]
    for method in ("point", "plane"):
        first = gpu_step(p, w, v, f, method, MOVE, CUT)
        for resolution in (None, 1, 3, 16):
            got = gpu_step(p, w, v, f, method, MOVE, CUT, resolution)
            assert got[1] == first[1] and np.array_equal(bits64(got[0]), bits64(first[0])), (method, resolution)


@pytest.mark.parametrize("name,deg,scale,method,iterations", ref.CASES[1:])
def test_full_fit_recovers_the_pose(name, deg, scale, method, iterations):
    from r3g import meshfit
    m, p, w = bean_case(deg, scale)
    got, info = meshfit.align(dev(p), bean_dev(), method=method, with_scale=scale is not None, weights=dev(w),
                              max_iterations=iterations, tolerance=1e-7 if method == "plane" else 0.0)
    err = ref.pose_error(got, m)
    print("device %s: %d updates, rms %.3e, error %.3e deg %.3e %.3e (tolerance %.1e deg %.1e %.1e, rms %.1e)"
          % ((name, info["iterations"], info["rms"]) + err + ref.FIT_TOL + (ref.RMS_TOL,)))
    assert got.shape == (4, 4) and got.dtype == np.float64 and info["used"] == len(p)
    assert all(e <= t for e, t in zip(err, ref.FIT_TOL)) and info["rms"] <= ref.RMS_TOL
    assert abs(info["scale"] - (scale or 1.0)) <= ref.FIT_TOL[2] * (scale or 1.0) + 1e-15


def test_cube_inits_recover_175_degrees():
    from r3g import meshfit
    m, p, w = bean_case(175.0)
    tp, tw = dev(p), dev(w)
    got, info = meshfit.align(tp, bean_dev(), weights=tw)
    err = ref.pose_error(got, m)
    print("identity start, 175 deg: rms %.3e, %.1f deg off" % (info["rms"], err[0]))
    assert 3e-2 <= info["rms"] <= 5e-2 and err[0] > 170.0
    inits = meshfit.cube_inits(tp, bean_dev(), tw)
    got, info = meshfit.align(tp, bean_dev(), weights=tw, inits=inits)
    err = ref.pose_error(got, m)
    print("cube_inits, 175 deg: start %d, rms %.3e, error %.3e deg %.3e" % ((info["chosen"], info["rms"]) + err[:2]))
    assert all(e <= t for e, t in zip(err, ref.FIT_TOL)) and info["rms"] <= ref.RMS_TOL
    assert len(info["candidate_rms"]) == 24 and info["candidate_rms"][info["chosen"]] == min(info["candidate_rms"])


def test_compare_aligned_keeps_the_radial_gap_of_concentric_spheres():
    """alignment must not explain away a difference in shape: the 400 and 441 spheres stay one voxel apart"""
    from r3g import mc, meshfit
    a, b = (mc.marching_cubes(dev(dref.sphere_volume(c)), 0.5) for c in (400, 441))
    s = meshfit.compare_aligned(a, b, samples=50000, taus=(0.9, 1.05), fit_samples=20000)
    print("compare_aligned, concentric spheres:", s["ab"]["mean"], s["ba"]["mean"], s["hausdorff"], s["fit"])
    assert 0.99 <= s["ab"]["mean"] <= 1.01 and 0.99 <= s["ba"]["mean"] <= 1.01
    assert s["fscore"][0.9] == 0 and s["fscore"][1.05] == 1 and s["hausdorff"] <= 1.03
    assert s["matrix"].shape == (4, 4) and 0.99 <= s["fit"]["rms"] <= 1.01


def test_mesh_register_and_apply_transform():
    from r3g.mesh import Mesh
    v, f = ref.bean()
    m = ref.pose(25.0)
    target = Mesh(v, f)
    moved = Mesh(ref.apply(np.linalg.inv(m), v), f)
    before = moved.distance_to(target, samples=5000)
    matrix, cost = moved.register(target, samples=1000)
    print("Mesh.register: cost %.3e (tolerance %.1e), error %.3e deg %.3e" % ((cost, ref.RMS_TOL) + ref.pose_error(matrix, m)[:2]))
    assert cost <= ref.RMS_TOL
    after = moved.apply_transform(matrix).distance_to(target, samples=5000)
    print("distance_to: chamfer_l1 %.3e -> %.3e, hausdorff %.3e -> %.3e"
          % (before["chamfer_l1"], after["chamfer_l1"], before["hausdorff"], after["hausdorff"]))
    # what is left is float32 rounding of coordinates of size <= 1.3 (ulp 1.2e-7), three times over
    assert before["ab"]["mean"] > 1e-2 and after["hausdorff"] <= 1e-6 and after["chamfer_l1"] <= 1e-6
    dmesh = Mesh.from_device(*bean_dev()).copy().apply_transform(np.diag([1.0, 1.0, -1.0, 1.0]))      # device-born: stays there
    assert dmesh._v is None and np.array_equal(dmesh.faces, f[:, [0, 2, 1]])
    q, d, face = target.closest_point(v[:50] * 1.5)
    aq = emu.closest((v[:50] * 1.5).astype(np.float32), v, f)
    assert isinstance(q, np.ndarray) and np.array_equal(bits(q), bits(aq[2])) and np.array_equal(face, aq[1])


def test_the_counter_advances_by_the_number_of_launches():
    from r3g import ffi, meshdist, meshfit
    m, p, w = bean_case(25.0)
    with ffi.device_lock(0):
        meshdist.build(*bean_dev())
        n0 = ffi.counter("meshfit_steps")
        meshfit.step(dev(p), method="plane")
        meshfit.step(dev(p), method="point")
        assert ffi.counter("meshfit_steps") == n0 + 2
        _, info = meshfit.fit(dev(p), dev(w))                           # one accumulation per update, and the one that stops
        n1 = n0 + 2 + info["iterations"] + 1
        assert info["converged"] and ffi.counter("meshfit_steps") == n1
        _, info = meshfit.fit(dev(p), dev(w), max_iterations=2)
        assert not info["converged"] and info["iterations"] == 2 and ffi.counter("meshfit_steps") == n1 + 3


def test_error_paths():
    import torch
    from r3g import ffi, meshdist, meshfit
    L = ffi.lib()
    m, p, w = bean_case(25.0)
    tp = dev(p)
    ctx = ffi.new_context(0)                                           # no grid on this context
    try:
        sums, used, mat, info = np.zeros(37), ctypes.c_int64(0), np.zeros(16), np.zeros(5)
        x = np.ascontiguousarray(emu.IDENTITY)
        out = torch.empty((len(p), 5), device="cuda")
        assert L.r3g_meshdist_closest(ctx, ctypes.c_void_p(tp.data_ptr()), len(p), ctypes.c_void_p(out.data_ptr()),
                                      ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr()), None) == -4
        assert L.r3g_meshfit_step(ctx, ctypes.c_void_p(tp.data_ptr()), len(p), None, x.ctypes.data, 1, float("inf"), sums.ctypes.data,
                                  ctypes.byref(used), None) == -4
        assert L.r3g_meshfit(ctx, ctypes.c_void_p(tp.data_ptr()), len(p), None, None, 1, 0, 5, 1e-7, float("inf"), mat.ctypes.data,
                             info.ctypes.data, None) == -4 and b"r3g_meshdist_build" in L.r3g_last_error()
    finally:
        L.r3g_destroy(ctx)
    with ffi.device_lock(0):
        meshdist.build(*bean_dev())
        for kw in (dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(max_iterations=-1), dict(tolerance=float("nan")),
                   dict(init=np.diag([1.0, 1.0, -1.0, 1.0]))):
            with pytest.raises(ffi.R3GError) as e:
                meshfit.fit(tp, **kw)
            assert e.value.code == -1, kw
        ctx0 = ffi.context(0)
        assert L.r3g_meshfit(ctx0, ctypes.c_void_p(tp.data_ptr()), len(p), None, None, 2, 0, 5, 1e-7, float("inf"), mat.ctypes.data,
                             info.ctypes.data, None) == -1
        with pytest.raises(ffi.R3GError) as e:                          # fewer than 3 points in reach: a defined error
            meshfit.fit(tp + 50.0, max_dist=0.1)
        assert e.value.code == -1 and "too few points" in str(e.value)
        with pytest.raises(ffi.R3GError) as e:
            meshfit.fit(tp[:2])
        assert "too few points" in str(e.value)
        init = ref.pose(12.0, 1.1)
        got, info = meshfit.fit(tp[:0], init=init)                      # n == 0: the start comes back, nothing used
        assert np.abs(got - init).max() <= 1e-15 and info["used"] == 0 and info["iterations"] == 0
        got, info = meshfit.fit(tp, dev(w))                             # and the context still works
        assert all(e <= t for e, t in zip(ref.pose_error(got, m), ref.FIT_TOL))
