"""The plane fit on the GPU (include/r3g.h r3g_plane_ransac / r3g_plane_moments, r3g/plane.py): counts, winner, mask, report and
every double bit for bit against the host twin of csrc/plane_core.h (tests/emu_plane.py) on the named clouds of tests/plane_ref.py,
the sizes around a wave, a block and the count pass's rows per block, the contract's edges and refusals, and the reference's
recorded fits and yaw search (goldens of tools/make_plane_goldens.py; nothing here reads the reference)."""
import ctypes
import json
import os

import numpy as np
import pytest

import emu_plane as E
import plane_ref as R

pytestmark = pytest.mark.gpu

NAMES = tuple(R.clouds())
_TWIN = {}
THR = 0.05


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def twin(name):
    """the twin's plain loops, computed once and left unchanged"""
    if name not in _TWIN:
        t = E.brute(*R.clouds()[name])
        for k in ("counts", "mask", "plane"):
            t[k].setflags(write=False)
        _TWIN[name] = t
    return _TWIN[name]


def device(p, t, thr, **kw):
    from r3g import plane
    r = plane.ransac(dev(np.asarray(p, np.float32).reshape(-1, 3)), np.asarray(t, np.int32).reshape(-1, 3), thr, **kw)
    return {"counts": None if r["counts"] is None else r["counts"].cpu().numpy().astype(np.uint32),
            "mask": None if r["mask"] is None else r["mask"].cpu().numpy(), "report": r["report"], "plane": r["plane"]}


def assert_same(d, t, what):
    assert np.array_equal(d["counts"], t["counts"]), what
    assert np.array_equal(d["mask"], t["mask"]), what
    assert d["report"] == t["report"], (what, d["report"], t["report"])
    assert d["plane"].tobytes() == t["plane"].tobytes(), (what, d["plane"], t["plane"])


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "plane_expect.json")) as f:
        expect = json.load(f)
    return expect, np.load(os.path.join(golden_dir, "plane_clouds.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_twin_bit_for_bit(name):
    from r3g import plane
    p, t, thr = R.clouds()[name]
    assert_same(device(p, t, thr), twin(name), name)
    for mask in (None, twin(name)["mask"]):
        m = plane.moments(dev(p), None if mask is None else dev(mask, np.uint8))
        e = E.moments(p, mask)
        assert m["out"].tobytes() == e["out"].tobytes(), (name, m["out"], e["out"])
        assert {k: m[k] for k in E.MOMENTS_REPORT} == e["report"], name


@pytest.mark.parametrize("n", (0, 1, 2, 3, 63, 64, 65, 4097, E.count_points() - 1, E.count_points() + 1))
def test_sizes_around_a_wave_a_block_and_the_count_tile(n):
    from r3g import plane
    p = R.uniform(21, 4097)[:n]
    t = R.random_triples(22, n, 33) if n >= 3 else np.array([[0, 1, 2], [0, 0, 0]], np.int32)
    assert_same(device(p, t, 0.2), E.brute(p, t, 0.2), n)
    assert plane.moments(dev(p))["out"].tobytes() == E.moments(p)["out"].tobytes()


@pytest.mark.parametrize("h", (0, 1, 2, 63, 65, 2000))
def test_table_sizes(h):
    p = R.uniform(23, 1500)
    t = R.random_triples(24, len(p), h) if h else np.zeros((0, 3), np.int32)
    d, e = device(p, t, 0.1), E.brute(p, t, 0.1)
    assert_same(d, e, h)
    if h == 0:
        assert d["report"] == {"n_usable": 1500, "n_valid": 0, "best": -1, "best_count": 0, "few": 1} and not d["mask"].any()


def test_tie_invalid_tables_odd_indices_and_nan_rows():
    tie = device(*R.clouds()["planes_tie"])
    assert tie["report"]["best"] == 0 and len(set(tie["counts"].tolist())) == 1      # four equal counts: the lowest h
    none = device(*R.clouds()["collinear"])
    assert none["report"]["n_valid"] == 0 and none["report"]["best"] == -1 and not none["mask"].any() and not none["counts"].any()
    assert none["plane"][:9].tolist() == [0.0] * 9 and none["plane"][9:12].tolist() == [0.0, 1.0, 0.0] and none["report"]["few"] == 1
    odd = device(*R.clouds()["duplicates"])
    assert odd["counts"][:4].tolist() == [0, 0, 0, 0]          # coincident rows, a repeated index, an index past the end, a negative one
    p, t, thr = R.clouds()["nonfinite"]
    nan = device(p, t, thr)
    assert nan["report"]["n_usable"] == len(p) - 4 and not nan["mask"][[5, 17, 200, 299]].any()
    assert nan["counts"][[3, 9, 11]].tolist() == [0, 0, 0]      # triples that touch a non-finite row


def test_optional_outputs_may_be_null():
    p, t, thr = R.clouds()["slab_outliers"]
    e = twin("slab_outliers")
    for kw in ({"counts": False}, {"mask": False}, {"counts": False, "mask": False}):
        d = device(p, t, thr, **kw)
        assert d["report"] == e["report"] and d["plane"].tobytes() == e["plane"].tobytes(), kw
        assert d["counts"] is None or np.array_equal(d["counts"], e["counts"])
        assert d["mask"] is None or np.array_equal(d["mask"], e["mask"])


def test_refusals():
    from r3g import ffi, plane
    p, t = dev(R.uniform(1, 16)), np.array([[0, 1, 2]], np.int32)
    for thr in (0.0, -0.05, float("nan"), float("inf")):
        with pytest.raises(ffi.R3GError) as err:
            plane.ransac(p, t, thr)
        assert err.value.code == -1 and "threshold" in str(err.value)
    with pytest.raises(ffi.R3GError) as err:
        plane.ransac(p, np.zeros((65537, 3), np.int32), THR)
    assert err.value.code == -1 and "n_hyp" in str(err.value)
    L, ctx = ffi.lib(), ffi.context(0)
    rep, out = (ctypes.c_int64 * 8)(), (ctypes.c_double * 16)()
    with ffi.device_lock(0):
        assert L.r3g_plane_ransac(ctx, None, 16, None, 0, THR, None, None, rep, out, None) == -1
        assert L.r3g_plane_ransac(ctx, ctypes.c_void_p(p.data_ptr()), 16, None, 1, THR, None, None, rep, out, None) == -1
        assert L.r3g_plane_ransac(ctx, ctypes.c_void_p(p.data_ptr()), 16, None, 0, THR, None, None, None, out, None) == -1
        assert L.r3g_plane_ransac(ctx, ctypes.c_void_p(p.data_ptr()), -1, None, 0, THR, None, None, rep, out, None) == -1
        assert L.r3g_plane_moments(ctx, None, 16, None, out, rep, None) == -1
    with pytest.raises(ValueError):
        plane.fit_plane_ransac_refined(dev(R.clouds()["collinear"][0]), 64)
    with pytest.raises(ValueError):
        plane.ransac(p.cpu(), t, THR)


def test_streams_and_contexts_give_the_same_bits():
    import torch
    from r3g import ffi, plane
    p, t, thr = R.clouds()["tilted"]
    e = twin("tilted")
    for _ in range(2):
        with torch.cuda.stream(torch.cuda.Stream()):
            assert_same(device(p, t, thr), e, "stream")
    L, own = ffi.lib(), ctypes.c_void_p()
    ffi.check(L.r3g_create(0, ctypes.byref(own)))
    try:
        dp, dt = dev(p), dev(t, np.int32)
        cnt, msk = torch.zeros(len(t), dtype=torch.int32, device="cuda"), torch.zeros(len(p), dtype=torch.uint8, device="cuda")
        rep, out = (ctypes.c_int64 * 8)(), (ctypes.c_double * 16)()
        torch.cuda.synchronize()
        ffi.check(L.r3g_plane_ransac(own, ctypes.c_void_p(dp.data_ptr()), len(p), ctypes.c_void_p(dt.data_ptr()), len(t), thr,
                                     ctypes.c_void_p(cnt.data_ptr()), ctypes.c_void_p(msk.data_ptr()), rep, out, ffi.stream_ptr()))
        d = {"counts": cnt.cpu().numpy().astype(np.uint32), "mask": msk.cpu().numpy(),
             "report": dict(zip(plane.RANSAC_REPORT, (int(v) for v in rep))), "plane": np.array(list(out))}
        assert_same(d, e, "context")
        ms = (ctypes.c_double * 4)()
        ffi.check(L.r3g_plane_times(own, ms))
        assert all(v >= 0.0 for v in ms)
    finally:
        L.r3g_destroy(own)


def test_reference_sampler_reproduces_the_recorded_fit(golden):
    import torch
    from r3g import plane
    expect, clouds = golden
    for name, e in expect["ransac"].items():
        p = clouds[name]
        torch.manual_seed(e["seed"])
        assert plane.draw_triples(len(p), expect["h"], sampler="reference").tolist() == e["triples"], name
        torch.manual_seed(e["seed"])
        normal, point, mask = plane.fit_plane_ransac_refined(dev(p), expect["h"], expect["threshold"], sampler="reference")
        assert torch.nonzero(mask).flatten().tolist() == e["mask_rows"] and int(mask.sum()) == e["count"], name
        assert tuple(normal.shape) == (3,) and tuple(point.shape) == (1, 3) and mask.dtype == torch.bool
        assert np.abs(point.cpu().numpy()[0] - np.array(e["centroid"])).max() <= len(p) * 2.0 ** -24 * np.abs(p).max(), name
        counts, rep = plane.ransac_counts(dev(p), e["triples"], expect["threshold"])
        assert rep["best_count"] == e["count"] == int(counts[rep["best"]]), name
    p = clouds["mirror_slab"]
    val = E.moments(p)["out"][10:13]
    bound = 4 * len(p) * 2.0 ** -24 * val[2] / (val[1] - val[0])
    normal, centroid = plane.fit_plane_svd(dev(p))
    ref = np.array(expect["svd"]["mirror_slab"]["svd_normal"])
    angle = float(np.arccos(min(1.0, abs(float(np.dot(normal.cpu().numpy().astype(np.float64), ref))) / np.linalg.norm(ref))))
    assert bound < 1e-2 and angle <= bound and tuple(centroid.shape) == (1, 3)


def test_fast_sampler_is_seeded_and_fits_the_floor():
    import torch
    from r3g import plane
    p = dev(R.slab(31, 3000, tilt_deg=4.0, outliers=0.3))
    a = plane.fit_plane_ransac_refined(p, 256, THR, generator=torch.Generator().manual_seed(5))
    b = plane.fit_plane_ransac_refined(p, 256, THR, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    t = plane.draw_triples(3000, 256, torch.Generator().manual_seed(5))
    assert tuple(t.shape) == (256, 3) and all(len(set(r)) == 3 for r in t.tolist())
    up = np.array([0.0, np.cos(np.deg2rad(4.0)), np.sin(np.deg2rad(4.0))])
    assert abs(float(np.dot(a[0].cpu().numpy(), up))) > 0.9995 and float(a[2].float().mean()) > 0.65


def test_best_initial_yaw_reproduces_the_recorded_search(golden):
    from r3g import plane
    expect, clouds = golden
    for name, e in expect["yaw"].items():
        r, losses, index = plane.best_initial_yaw(dev(clouds[name + "_verts"]), dev(clouds[name + "_target"]), 18, "bbox")
        assert index == e["argmin"], name
        got, rec = losses.cpu().numpy().astype(np.float64), np.array(e["losses"])
        print(name, "largest per-loss relative difference %.3e" % (np.abs(got - rec) / rec).max())
        assert rec.min() > 0 and np.all(np.abs(got - rec) <= 1e-4 * rec), name      # every loss against itself
        assert np.allclose(r.cpu().numpy(), np.array(e["rotation"]), atol=1e-6), name


def test_fit_floor_takes_each_branch():
    from r3g import cloud, plane
    import torch
    flat = R.slab(41, 2000, noise=0.0005)
    rough = R.slab(42, 2000, noise=0.025)
    dirty = R.slab(43, 2000, noise=0.03, outliers=0.4)
    for p, method in ((flat, "pca"), (dirty, "ransac"), (rough, "svd")):
        fit = plane.fit_floor(dev(p), 200, THR, generator=torch.Generator().manual_seed(1))
        assert fit["method"] == method, (method, fit["planarity"], fit["inlier_ratio"])
        assert (fit["planarity"] < 1e-3) == (method == "pca") and (method != "ransac" or fit["inlier_ratio"] < 0.85)
        assert abs(float(fit["normal"][1])) > 0.99 and tuple(fit["point"].shape) == (1, 3) and fit["mask"].dtype == torch.bool
        assert fit["ransac_rmse"] > 0 and fit["svd_rmse"] > 0
    # no triple spans a plane: the planarity test still decides a flat cloud; any other cloud has no answer
    line = plane.fit_floor(dev(R.clouds()["collinear"][0]), 64, THR, generator=torch.Generator().manual_seed(1))
    assert line["method"] == "pca" and line["ransac_rmse"] is None and line["inlier_ratio"] is None and bool(line["mask"].all())
    with pytest.raises(ValueError):
        plane.fit_floor(dev(dirty), threshold=THR, triples=np.array([[0, 0, 1], [2, 2, 2]]))
    with pytest.raises(ValueError):
        plane.best_initial_yaw(dev(flat[:50]), dev(rough[:50]), 18, "centre_of_mass")
    via = cloud.PointCloud(dirty.astype(np.float64)).fit_plane(200, THR, generator=torch.Generator().manual_seed(1))
    assert via["method"] == "ransac" and via["normal"].shape == (3,) and via["mask"].shape == (2000,)


def test_obb_frame_and_times():
    from r3g import plane
    rng = np.random.default_rng(1)
    pts = (rng.uniform(-1, 1, (4000, 3)) * [2.0, 0.3, 0.5]) @ R.yaw_rotation(0.6).T + [1.0, 2.0, 3.0]
    c, rot, ext = plane.yaw_obb(dev(pts))
    c0, rot0, ext0 = R.yaw_obb(pts.astype(np.float32))
    assert np.allclose(c, c0, atol=1e-6) and np.allclose(rot, rot0, atol=1e-6) and np.allclose(ext, ext0, atol=1e-5)
    m, inv = plane.plane_frame(dev(np.array([0.1, 0.9, -0.2])), dev(np.array([[1.0, 2.0, 3.0]])))
    m0, inv0 = R.plane_frame([0.1, 0.9, -0.2], [1.0, 2.0, 3.0])
    assert np.allclose(m, m0, atol=1e-7) and np.allclose(inv, inv0, atol=1e-7)
    device(*R.clouds()["slab_outliers"])
    ms = plane.times(0)
    assert tuple(ms) == plane.PASSES and all(v >= 0.0 for v in ms.values())
