"""Mesh distance on the GPU (include/r3g.h r3g_meshdist_build / r3g_meshdist_query, r3g/meshdist.py, Mesh.distance_to):
bit for bit against the host twin of csrc/meshdist_core.h (tests/emu_meshdist.py), within meshdist_ref.DIST_TOL of the
float64 oracle (tests/meshdist_ref.py), and the scores of two concentric spheres whose true distance is known."""
import ctypes

import numpy as np
import pytest

import emu_meshdist as emu
import meshdist_ref as ref

pytestmark = pytest.mark.gpu

_CACHE = {}


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_dist2(points, verts, faces, resolution=None):
    """(dist2, face, info) through build + query (nearest() returns the square root)"""
    from r3g import ffi, meshdist
    with ffi.device_lock(0):
        info = meshdist.build(dev(verts), dev(faces, np.int32), resolution)
        d2, face = meshdist.query(dev(points))
    return d2.cpu().numpy(), face.cpu().numpy(), info


def soup_twin():
    """the soup, 4097 points and the twin's brute force over them (computed once)"""
    if "soup" not in _CACHE:
        v, f = ref.soup()
        p = ref.many_points(4097)
        a2, af, _ = emu.brute(p, v, f)
        a2.setflags(write=False)
        af.setflags(write=False)
        _CACHE["soup"] = (v, f, p, a2, af)
    return _CACHE["soup"]


def spheres():
    """the 400 (golden A) and 441 spheres at 65^3 by the product's marching cubes, index units, on the device"""
    if "spheres" not in _CACHE:
        from r3g import mc
        _CACHE["spheres"] = tuple(mc.marching_cubes(dev(ref.sphere_volume(c)), 0.5) for c in (400, 441))
    return _CACHE["spheres"]


@pytest.mark.parametrize("resolution", [1, 3, 16, None])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_device_equals_the_twin_bit_for_bit(n, resolution):
    v, f, p, a2, af = soup_twin()
    d2, face, info = gpu_dist2(p[:n], v, f, resolution)
    assert d2.dtype == np.float32 and face.dtype == np.int32
    assert np.array_equal(bits(d2), bits(a2[:n])) and np.array_equal(face, af[:n])
    assert info["skipped"] == 0 and info["resolution"] == (resolution or emu.grid(p[:1], v, f, 0)[2]["resolution"])
    assert info["pairs"] == emu.grid(p[:1], v, f, info["resolution"])[2]["pairs"]


@pytest.mark.parametrize("resolution", [127, 128])
def test_forced_resolutions_on_either_side_of_the_scan_switch(resolution):
    """127^3 + 1 cells are 1001 scan tiles, 128^3 + 1 are 1025: one block scans the tile sums 4 or 40 to a thread"""
    v, f, p, a2, af = soup_twin()
    d2, face, info = gpu_dist2(p[:65], v, f, resolution)
    assert np.array_equal(bits(d2), bits(a2[:65])) and np.array_equal(face, af[:65])
    assert info["resolution"] == resolution and info["pairs"] == emu.grid(p[:1], v, f, resolution)[2]["pairs"]


def test_two_runs_are_identical_and_the_resolution_does_not_matter():
    import torch
    from r3g import meshdist
    v, f, p, a2, af = soup_twin()
    tv, tf, tp = dev(v), dev(f, np.int32), dev(p)
    first = meshdist.nearest(tp, tv, tf)
    for resolution in (None, 2, 7, 32):
        d, face = meshdist.nearest(tp, tv, tf, resolution)
        assert torch.equal(d.view(torch.int32), first[0].view(torch.int32)) and torch.equal(face, first[1])
    np.testing.assert_allclose(first[0].cpu().numpy(), np.sqrt(a2), rtol=2e-7, atol=0)


def test_mesh_buffers_may_be_freed_between_build_and_query():
    import torch
    from r3g import ffi, meshdist
    v, f, p, a2, af = soup_twin()
    with ffi.device_lock(0):
        tv, tf = dev(v), dev(f, np.int32)
        meshdist.build(tv, tf)
        tv.fill_(float("nan"))
        tf.fill_(-5)
        del tv, tf
        torch.cuda.empty_cache()
        d2, face = meshdist.query(dev(p[:500]))
    assert np.array_equal(bits(d2.cpu().numpy()), bits(a2[:500])) and np.array_equal(face.cpu().numpy(), af[:500])


def test_sphere_against_the_float64_oracle():
    from r3g import meshdist
    a, b = spheres()
    v, f = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert v.shape == (7470, 3) and f.shape == (14936, 3)
    p = ref.sphere_points(b[0].cpu().numpy(), b[1].cpu().numpy(), 1000, 1000)
    d, face = meshdist.nearest(dev(p), a[0], a[1])
    d, face = d.cpu().numpy().astype(np.float64), face.cpu().numpy()
    d64, _ = ref.oracle(p, v, f)
    err = float(np.abs(d - d64).max()) / ref.extent(v, p)
    print("meshdist device vs float64 oracle, sphere: %.3e of the extent (tolerance %.3e)" % (err, ref.DIST_TOL))
    assert err <= ref.DIST_TOL
    own = ref.point_triangle_distance(p.astype(np.float64), v.astype(np.float64)[f[face]])      # the face returned holds the distance
    assert float(np.abs(own - d64).max()) / ref.extent(v, p) <= ref.DIST_TOL


def test_concentric_spheres_through_compare():
    import torch
    from r3g import meshdist
    a, b = spheres()
    for (v, f), (r0, r1) in zip((a, b), ((19.97, 19.99), (20.97, 20.99))):
        r = (v.double() - 32).norm(dim=1)
        assert r0 < float(r.min()) and float(r.max()) < r1 + 0.01
    s = meshdist.compare(a, b, samples=50000, taus=(0.9, 1.05))
    print("concentric spheres:", {k: s[k] for k in ("chamfer_l1", "hausdorff", "samples", "resolution", "query_ms")},
          s["ab"]["mean"], s["ba"]["mean"])
    assert 0.99 <= s["ab"]["mean"] <= 1.01 and 0.99 <= s["ba"]["mean"] <= 1.01
    assert s["fscore"][0.9] == 0 and s["fscore"][1.05] == 1
    assert s["hausdorff"] <= 1.03
    assert s["chamfer_l1"] == s["ab"]["mean"] + s["ba"]["mean"] and s["skipped"] == (0, 0)
    assert s["samples"][0] >= 50000 + a[0].shape[0] and s["samples"][1] >= 50000 + b[0].shape[0] and s["query_ms"] > 0
    for src, dst in ((a, b), (b, a)):                        # every distance, not only the summary
        pts = torch.cat([meshdist.sample_surface(src[0], src[1], 50000)[0], src[0]])
        d, _ = meshdist.nearest(pts, dst[0], dst[1])
        assert 0.97 <= float(d.min()) and float(d.max()) <= 1.03


def test_compare_a_mesh_with_itself():
    from r3g import meshdist
    a, _ = spheres()
    d, face = meshdist.nearest(a[0], a[0], a[1])
    assert float(d.max()) == 0.0                              # the vertex part: exactly zero
    f = a[1].long()
    assert bool(((f[face.long()] == __import__("torch").arange(a[0].shape[0], device=f.device)[:, None]).any(1)).all())
    tol = ref.DIST_TOL * ref.extent(a[0].cpu().numpy())
    s = meshdist.compare(a, a, samples=50000, taus=(tol,))
    print("compare(a, a): hausdorff %.3e, tolerance %.3e" % (s["hausdorff"], tol))
    assert s["hausdorff"] <= tol and s["chamfer_l1"] <= 2 * tol and s["fscore"][tol] == 1


def test_error_paths_leave_the_context_usable():
    import torch
    from r3g import ffi, meshdist
    v, f, p, a2, af = soup_twin()
    tv, tp = dev(v), dev(p[:100])
    for bad_value in (len(v), -1, 2 ** 31 - 1):
        bad = f.copy()
        bad[123, 1] = bad_value
        with pytest.raises(ffi.R3GError) as e:
            meshdist.build(tv, dev(bad, np.int32))
        assert e.value.code == -2 and "face index" in str(e.value)
        with pytest.raises(ffi.R3GError) as e:                # a failed build leaves no grid behind
            meshdist.query(tp)
        assert e.value.code == -4
    d2, face, _ = gpu_dist2(p[:100], v, f)                    # and the context still works
    assert np.array_equal(bits(d2), bits(a2[:100])) and np.array_equal(face, af[:100])
    with pytest.raises(ffi.R3GError) as e:
        meshdist.build(tv, torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert e.value.code == -1
    with pytest.raises(ffi.R3GError) as e:
        meshdist.build(torch.full_like(tv, float("inf")), dev(f, np.int32))
    assert e.value.code == -1 and "non-finite" in str(e.value)
    with pytest.raises(ffi.R3GError):
        meshdist.build(tv, dev(f, np.int32), resolution=257)
    with pytest.raises(ValueError):
        meshdist.nearest(torch.from_numpy(p[:4]), tv, dev(f, np.int32))          # CPU tensors are refused
    with pytest.raises(ValueError):
        meshdist.nearest(tp, torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(ValueError):
        meshdist.sample_surface(tv, torch.zeros((0, 3), dtype=torch.int32, device="cuda"), 10)


def test_query_before_any_build_is_an_error():
    import torch
    from r3g import ffi
    ctx = ffi.new_context(0)
    try:
        p = torch.zeros((8, 3), device="cuda")
        d2 = torch.empty(8, device="cuda")
        face = torch.empty(8, dtype=torch.int32, device="cuda")
        rc = ffi.lib().r3g_meshdist_query(ctx, ctypes.c_void_p(p.data_ptr()), 8, ctypes.c_void_p(d2.data_ptr()),
                                          ctypes.c_void_p(face.data_ptr()), None)
        assert rc == -4 and b"r3g_meshdist_build" in ffi.lib().r3g_last_error()
    finally:
        ffi.lib().r3g_destroy(ctx)


def test_non_finite_points_and_vertices():
    import torch
    from r3g import meshdist
    v, f, p, _, _ = soup_twin()
    v = v.copy()
    v[3 * 7] = np.nan
    v[3 * 9 + 1, 2] = np.inf
    q = p[:300].copy()
    q[5, 1] = np.nan
    q[64, 0] = -np.inf
    q[299] = np.nan
    a2, af, skipped = emu.brute(q, v, f)
    for resolution in (None, 1, 9):
        d2, face, info = gpu_dist2(q, v, f, resolution)
        assert info["skipped"] == skipped == 2
        assert np.array_equal(bits(d2), bits(a2)) and np.array_equal(face, af)
    assert np.isnan(d2[[5, 64, 299]]).all() and (face[[5, 64, 299]] == -1).all() and np.isfinite(np.delete(d2, [5, 64, 299])).all()
    d, face = meshdist.nearest(torch.zeros((0, 3), device="cuda"), dev(v), dev(f, np.int32))        # N == 0: a no-op
    assert d.shape == (0,) and face.shape == (0,)


def test_mesh_distance_to():
    from r3g import meshdist
    from r3g.mesh import Mesh
    a, b = spheres()
    s = Mesh.from_device(*a).distance_to(Mesh.from_device(*b), samples=20000, taus=(0.9, 1.05))
    assert 0.99 <= s["ab"]["mean"] <= 1.01 and 0.99 <= s["ba"]["mean"] <= 1.01 and s["hausdorff"] <= 1.03
    assert s["fscore"][0.9] == 0 and s["fscore"][1.05] == 1
    host = Mesh(a[0].cpu().numpy(), a[1].cpu().numpy())               # host arrays are uploaded on demand
    assert host.distance_to(Mesh.from_device(*a), samples=5000)["ab"]["max"] <= ref.DIST_TOL * ref.extent(a[0].cpu().numpy())
    with pytest.raises(ValueError):
        Mesh().distance_to(host)
    assert meshdist.voxel_size(1.01, 64) == pytest.approx(2.02 / 65)
