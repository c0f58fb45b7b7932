"""Point in mesh on the GPU (include/r3g.h r3g_meshinside_build / r3g_meshinside_query, r3g/meshinside.py, Mesh.contains):
every count equal to the host twin of csrc/meshinside_core.h (tests/emu_meshinside.py), the scores on top of it against the
numpy restatement (tests/meshinside_ref.py) and against two concentric spheres whose answers are known."""
import ctypes

import numpy as np
import pytest

import emu_meshinside as emu
import meshdist_ref as mref
import meshinside_ref as ref

pytestmark = pytest.mark.gpu

_CACHE = {}
RHO = float(np.sqrt(399.5))


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def gpu_counts(points, verts, faces, axis, resolution=None):
    """(count, info) through build + query"""
    from r3g import ffi, meshinside
    with ffi.device_lock(0):
        info = meshinside.build(dev(verts), dev(faces, np.int32), axis, resolution)
        count = meshinside.query(dev(points))
    return count.cpu().numpy(), info


def soup_twin(axis):
    """the soup, 4097 points and the twin's brute force over them (computed once per axis, read-only)"""
    if ("soup", axis) not in _CACHE:
        v, f = mref.soup()
        p = mref.many_points(4097)
        c = emu.brute(p, v, f, axis)[0]
        c.setflags(write=False)
        _CACHE["soup", axis] = (v, f, p, c)
    return _CACHE["soup", axis]


def spheres():
    """the 400 (golden A) and 441 spheres at 65^3 by the product's marching cubes, index units, on the device"""
    if "spheres" not in _CACHE:
        from r3g import mc
        _CACHE["spheres"] = tuple(mc.marching_cubes(dev(mref.sphere_volume(c)), 0.5) for c in (400, 441))
    return _CACHE["spheres"]


def host(mesh):
    return mesh[0].cpu().numpy(), mesh[1].cpu().numpy()


def sphere_iou_restated():
    """the restatement's volume_iou of the two spheres at n = 32 (computed once)"""
    if "iou" not in _CACHE:
        a, b = spheres()
        _CACHE["iou"] = ref.volume_iou(host(a), host(b), 32)
    return _CACHE["iou"]


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_device_equals_the_twin(n, axis):
    v, f, p, want = soup_twin(axis)
    first = None
    for resolution in (1, 3, 16, None):
        got, info = gpu_counts(p[:n], v, f, axis, resolution)
        assert got.dtype == np.int32 and np.array_equal(got, want[:n]), resolution
        twin = emu.grid(p[:1], v, f, axis, resolution or 0)[1]
        assert info["skipped"] == 0 and info["resolution"] == twin["resolution"] and info["pairs"] == twin["pairs"]
        first = got if first is None else first
        assert np.array_equal(got, first)                         # the result does not depend on the resolution


def test_the_highest_resolution():
    """1024^2 + 1 columns: 513 scan tiles, the most the columns can ask of the scan"""
    v, f, p, want = soup_twin(2)
    got, info = gpu_counts(p[:65], v, f, 2, 1024)
    assert np.array_equal(got, want[:65])
    assert info["resolution"] == 1024 and info["pairs"] == emu.grid(p[:1], v, f, 2, 1024)[1]["pairs"]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cube_literals_and_the_sphere_lattice(axis):
    v, f = ref.cube()
    got, _ = gpu_counts(ref.cube_literal_points(axis), v, f, axis)
    for c, (_, want) in zip(got, ref.CUBE_LITERALS):
        assert (c % 2 == 0 and c >= 0) if want == "even" else c == want, (axis, got)
    sv, sf = host(spheres()[0])
    assert sv.shape == (7470, 3) and sf.shape == (14936, 3)
    p = ref.sphere_lattice()
    got, info = gpu_counts(p, sv, sf, axis)
    assert np.array_equal(got, emu.brute(p, sv, sf, axis)[0]) and info["resolution"] == 61
    rho = np.linalg.norm(p.astype(np.float64) - 32, axis=1)
    far = np.abs(rho - RHO) > 1.0
    assert got.max() <= 2 and np.array_equal((got % 2 == 1)[far], rho[far] < RHO)


def test_mesh_buffers_may_be_freed_and_both_grids_are_held_at_once():
    import torch
    from r3g import ffi, meshdist, meshinside
    v, f, p, want = soup_twin(2)
    with ffi.device_lock(0):
        tv, tf = dev(v), dev(f, np.int32)
        meshinside.build(tv, tf, 2)
        meshdist.build(tv, tf)
        tv.fill_(float("nan"))
        tf.fill_(-5)
        del tv, tf
        torch.cuda.empty_cache()
        d2, _ = meshdist.query(dev(p[:500]))
        count = meshinside.query(dev(p[:500]))
    assert np.array_equal(count.cpu().numpy(), want[:500]) and bool(torch.isfinite(d2).all())


def test_non_finite_points_and_vertices():
    import torch
    from r3g import meshinside
    v, f, p, _ = soup_twin(2)
    v = v.copy()
    v[3 * 7] = np.nan
    v[3 * 9 + 1, 2] = np.inf
    q = p[:300].copy()
    q[5, 1] = np.nan
    q[64, 0] = -np.inf
    q[299] = np.nan
    for axis in range(3):
        want, skipped = emu.brute(q, v, f, axis)
        for resolution in (None, 1, 9):
            got, info = gpu_counts(q, v, f, axis, resolution)
            assert info["skipped"] == skipped == 2 and np.array_equal(got, want)
        assert (got[[5, 64, 299]] == -1).all() and (np.delete(got, [5, 64, 299]) >= 0).all()
    inside = meshinside.contains(dev(q), dev(v), dev(f, np.int32))
    assert inside.dtype == torch.bool and not bool(inside[[5, 64, 299]].any())
    c = meshinside.crossings(torch.zeros((0, 3), device="cuda"), dev(v), dev(f, np.int32))        # N == 0: a no-op
    assert c.shape == (0,) and c.dtype == torch.int32


def test_error_paths_leave_the_context_usable():
    import torch
    from r3g import ffi, meshinside
    v, f, p, want = soup_twin(2)
    tv, tp = dev(v), dev(p[:100])
    for bad_value in (len(v), -1, 2 ** 31 - 1):
        bad = f.copy()
        bad[123, 1] = bad_value
        with pytest.raises(ffi.R3GError) as e:
            meshinside.build(tv, dev(bad, np.int32))
        assert e.value.code == -2 and "face index" in str(e.value)
        with pytest.raises(ffi.R3GError) as e:                # a failed build leaves no grid behind
            meshinside.query(tp)
        assert e.value.code == -4
    got, _ = gpu_counts(p[:100], v, f, 2)                     # and the context still works
    assert np.array_equal(got, want[:100])
    with pytest.raises(ffi.R3GError) as e:
        meshinside.build(tv, torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert e.value.code == -1
    with pytest.raises(ffi.R3GError) as e:
        meshinside.build(torch.full_like(tv, float("inf")), dev(f, np.int32))
    assert e.value.code == -1 and "non-finite" in str(e.value)
    for kw in ({"resolution": 1025}, {"axis": 3}, {"axis": -1}):
        with pytest.raises(ffi.R3GError) as e:
            meshinside.build(tv, dev(f, np.int32), **kw)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        meshinside.crossings(torch.from_numpy(p[:4]), tv, dev(f, np.int32))          # CPU tensors are refused
    with pytest.raises(ValueError):
        meshinside.crossings(tp, torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(ValueError):
        meshinside.contains(tp, tv, dev(f, np.int32), axes=(0, 1))


def test_query_before_any_build_is_an_error():
    import torch
    from r3g import ffi
    ctx = ffi.new_context(0)
    try:
        p = torch.zeros((8, 3), device="cuda")
        count = torch.empty(8, dtype=torch.int32, device="cuda")
        rc = ffi.lib().r3g_meshinside_query(ctx, ctypes.c_void_p(p.data_ptr()), 8, ctypes.c_void_p(count.data_ptr()), None)
        assert rc == -4 and b"r3g_meshinside_build" in ffi.lib().r3g_last_error()
    finally:
        ffi.lib().r3g_destroy(ctx)


def test_signed_distance():
    import torch
    from r3g import meshdist, meshinside
    a, _ = spheres()
    sv, sf = host(a)
    p = ref.sphere_lattice()
    tp = dev(p)
    sd, face = meshinside.signed_distance(tp, *a)
    d, face_n = meshdist.nearest(tp, *a)
    assert sd.dtype == torch.float32 and torch.equal(sd.abs().view(torch.int32), d.view(torch.int32)) and torch.equal(face, face_n)
    sd = sd.cpu().numpy()
    parity = emu.brute(p, sv, sf, 2)[0] % 2 == 1
    on = d.cpu().numpy() == 0                                    # -0.0 and 0.0 have no sign to compare
    assert np.array_equal((sd < 0)[~on], parity[~on])
    rho = np.linalg.norm(p.astype(np.float64) - 32, axis=1)
    assert (rho <= 18).sum() > 500 and (rho >= 22).sum() > 1000
    assert (sd[rho <= 18] < 0).all() and (sd[rho >= 22] > 0).all()
    sd3, _ = meshinside.signed_distance(tp, *a, axes=(0, 1, 2))  # a closed surface: three axes change nothing
    assert np.array_equal(sd3.cpu().numpy().view(np.uint32), sd.view(np.uint32))


def test_contains_with_three_axes_reports_agreement():
    from r3g import meshinside
    a, _ = spheres()
    sv, sf = host(a)
    p = ref.sphere_lattice()
    inside, agreement = meshinside.contains(dev(p), *a, axes=(0, 1, 2))
    assert agreement == 1.0 and np.array_equal(inside.cpu().numpy(), emu.brute(p, sv, sf, 2)[0] % 2 == 1)
    hemi = sf[(sv[sf][:, :, 2] > 32).all(1)]
    inside, agreement = meshinside.contains(dev(p), a[0], dev(hemi, np.int32), axes=(0, 1, 2))       # open: raises nothing
    want, want_agreement = emu.contains(p, sv, hemi, (0, 1, 2))
    assert agreement < 1.0 and agreement == pytest.approx(want_agreement, abs=1e-12)
    assert np.array_equal(inside.cpu().numpy(), want)


def test_volume_iou_of_the_spheres():
    import mesh_metrics
    from r3g import meshinside
    a, b = spheres()
    s = meshinside.volume_iou(a, b, n=32)
    want = sphere_iou_restated()
    print("volume_iou, spheres 400 / 441, n = 32:", s)
    for k in ("inter", "union", "in_a", "in_b"):
        assert isinstance(s[k], int) and s[k] == want[k], k
    ratio = abs(mesh_metrics.signed_volume(*host(a))) / abs(mesh_metrics.signed_volume(*host(b)))
    print("iou %.6f, volume ratio %.6f, tolerance %.4e" % (s["iou"], ratio, ref.IOU_TOL))
    assert s["iou"] == s["inter"] / s["union"] and abs(s["iou"] - ratio) <= ref.IOU_TOL
    assert s["volume_a"] == pytest.approx(want["volume_a"], rel=1e-12) and s["volume_b"] == pytest.approx(want["volume_b"], rel=1e-12)
    assert s["n"] == 32 and s["query_ms"] > 0
    s3 = meshinside.volume_iou(a, b, n=32, axes=(0, 1, 2))
    assert all(s3[k] == s[k] for k in ("inter", "union", "in_a", "in_b"))
    boxes = [tuple(dev(x, t) for x, t in zip(ref.box_mesh(lo, hi), (np.float32, np.int32))) for lo, hi in
             (((0, 0, 0), (4, 4, 4)), ((1, 1, 1), (3, 3, 3)), ((10, 10, 10), (11, 11, 11)))]
    s = meshinside.volume_iou(boxes[0], boxes[1], n=8)
    assert (s["in_a"], s["in_b"], s["inter"], s["union"], s["iou"], s["volume_a"], s["volume_b"]) == (512, 64, 64, 512, 0.125, 64.0, 8.0)
    s = meshinside.volume_iou(boxes[1], boxes[2], n=2)
    assert s["union"] == 0 and s["iou"] == 0.0


def test_normal_consistency_of_the_spheres():
    from r3g import meshinside
    a, b = spheres()
    s = meshinside.normal_consistency(a, b, samples=20000)
    print("normal consistency, concentric spheres:", s)
    for k in ("ab", "ba"):
        assert s[k]["abs"] == pytest.approx(s[k]["signed"], abs=1e-12) and s[k]["abs"] >= ref.NC_MIN
    assert s["abs"] == 0.5 * (s["ab"]["abs"] + s["ba"]["abs"]) and s["signed"] == 0.5 * (s["ab"]["signed"] + s["ba"]["signed"])
    flipped = (b[0], b[1].flip(1).contiguous())
    s = meshinside.normal_consistency(a, flipped, samples=20000)
    assert s["abs"] >= ref.NC_MIN and s["signed"] <= -ref.NC_MIN


def test_mesh_contains_through_compat_trimesh():
    import importlib.util
    import os
    import r3g
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(r3g.__file__))), "compat", "trimesh", "__init__.py")
    spec = importlib.util.spec_from_file_location("r3g_compat_trimesh", path)      # under a private name: sys.modules keeps no trimesh
    trimesh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(trimesh)
    assert trimesh.__r3g_compat__
    a, b = spheres()
    sv, sf = host(a)
    m = trimesh.Trimesh(sv, sf, process=False)
    p = ref.sphere_lattice()[:1000]
    inside = m.contains(p)
    assert isinstance(inside, np.ndarray) and inside.dtype == bool and inside.shape == (1000,)
    assert np.array_equal(inside, emu.brute(p, sv, sf, 2)[0] % 2 == 1)
    assert np.array_equal(m.contains(p.astype(np.float64).tolist()), inside)
    sd = m.signed_distance(p)
    assert isinstance(sd, np.ndarray) and sd.dtype == np.float32 and np.array_equal((sd < 0)[sd != 0], inside[sd != 0])
    from r3g.mesh import Mesh
    s = m.volume_iou(Mesh.from_device(*b), n=32)
    want = sphere_iou_restated()
    assert s["inter"] == want["inter"] and s["union"] == want["union"]
    with pytest.raises(ValueError):
        Mesh().contains(p)


def test_counter_advances():
    from r3g import ffi
    v, f, p, _ = soup_twin(2)
    n0 = ffi.counter("meshinside_tests")
    _, info = gpu_counts(p[:1000], v, f, 2, 4)
    n1 = ffi.counter("meshinside_tests")
    assert n1 - n0 == emu.grid(p[:1000], v, f, 2, 4)[1]["tests"] > 0
