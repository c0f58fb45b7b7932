"""DBSCAN on the GPU (include/r3g.h r3g_cloud_dbscan, r3g/cloud.py): labels, counts and report bit for bit against the host
twin of csrc/dbscan_core.h (tests/emu_dbscan.py) on the clouds of tests/test_dbscan_cpu.py, the contract's edges and refusals,
and the reference's two filters against the rows it kept (goldens recorded by tools/make_dbscan_goldens.py)."""
import ctypes

import numpy as np
import pytest

import dbscan_ref as R
import emu_dbscan as emu

pytestmark = pytest.mark.gpu

RESOLUTIONS = (1, 3, 16, None)
ERR_STATE = -4      # R3G_ERR_STATE of include/r3g.h
NAMES = tuple(R.RANDOM) + tuple(R.fixed_clouds())
_TWIN = {}


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def twin(name):
    """the twin's brute force, computed once and left unchanged"""
    if name not in _TWIN:
        t = emu.brute(*R.clouds()[name])
        for k in ("labels", "counts", "core"):
            t[k].setflags(write=False)
        _TWIN[name] = t
    return _TWIN[name]


def report_of(rep):
    return {k: rep[k] for k in R.REPORT}


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_twin_bit_for_bit(name):
    """with d_count the whole count, without it a count that may stop at min_samples: the labels and the report are the same"""
    from r3g import cloud
    p, eps, ms = R.clouds()[name]
    t = twin(name)
    dp = dev(p)
    for res in RESOLUTIONS:
        labels, counts, rep = cloud.dbscan(dp, eps, ms, res, counts=True)
        assert labels.dtype.is_signed and tuple(labels.shape) == (len(p),) and tuple(counts.shape) == (len(p),)
        assert np.array_equal(labels.cpu().numpy(), t["labels"]), (name, res)
        assert np.array_equal(counts.cpu().numpy().astype(np.uint32), t["counts"]), (name, res)
        assert report_of(rep) == t["report"], (name, res)
        if t["report"]["n_usable"]:
            assert rep["resolution"] == (res if res else emu.grid(p, eps, ms)["resolution"])
        quick, rep2 = cloud.dbscan(dp, eps, ms, res)
        assert np.array_equal(quick.cpu().numpy(), t["labels"]) and report_of(rep2) == t["report"], (name, res)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sizes_around_a_wave_and_past_a_block(n):
    from r3g import cloud
    p = R.uniform(21, 4097)[:n]
    eps, ms = 0.06, 4
    t = emu.brute(p, eps, ms)
    for res in RESOLUTIONS:
        labels, counts, rep = cloud.dbscan(dev(p), eps, ms, res, counts=True)
        assert np.array_equal(labels.cpu().numpy(), t["labels"]) and np.array_equal(counts.cpu().numpy().astype(np.uint32), t["counts"])
        assert report_of(rep) == t["report"]


def test_launches_do_not_depend_on_the_data():
    """a chain of 4 097 core points is one cluster after the same number of launches as the uniform cloud: no pass is repeated
    until it converges"""
    from r3g import cloud, ffi
    per_call = []
    with ffi.device_lock(0):
        for name in ("chain", "uniform", "blobs"):
            p, eps, ms = R.clouds()[name]
            n0 = ffi.counter("dbscan_launches")
            _, rep = cloud.dbscan(dev(p), eps, ms)
            per_call.append(ffi.counter("dbscan_launches") - n0)
            assert report_of(rep) == twin(name)["report"]
    assert per_call[0] == per_call[1] == per_call[2] and 0 < per_call[0] <= 32, per_call
    assert twin("chain")["report"]["n_clusters"] == 1 and twin("chain")["report"]["n_core"] == 4097


def test_predicate_evaluations_are_counted_and_match_the_twin():
    from r3g import cloud, ffi
    p, eps, ms = R.clouds()["shell"]
    with ffi.device_lock(0):
        n0 = ffi.counter("dbscan_tests")
        cloud.dbscan(dev(p), eps, ms, 16, counts=True)
        tests = ffi.counter("dbscan_tests") - n0
    assert tests == emu.grid(p, eps, ms, 16)["tests"]


def test_two_runs_are_identical():
    from r3g import cloud
    p, eps, ms = R.clouds()["blobs"]
    a = cloud.dbscan(dev(p), eps, ms, counts=True)
    b = cloud.dbscan(dev(p), eps, ms, counts=True)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy()) and np.array_equal(a[1].cpu().numpy(), b[1].cpu().numpy()) and a[2] == b[2]


def test_the_callers_buffer_may_go_and_the_cloud_is_replaced():
    """the call synchronises and the context keeps its own packed copy of the usable points: k-NN afterwards runs against them"""
    import torch
    import emu_cloud
    from r3g import cloud, ffi
    p, eps, ms = R.clouds()["nonfinite"]
    with ffi.device_lock(0):
        dp = dev(p)
        labels, rep = cloud.dbscan(dp, eps, ms)
        dp.fill_(float("nan"))
        del dp
        torch.cuda.empty_cache()
        junk = torch.full((len(p), 3), 7.0, device="cuda")
        q = p[np.isfinite(p).all(1)][:200]
        d2, ix = cloud.knn(dev(q), 3)
        del junk
    td, ti, _ = emu_cloud.brute(q, p, 3)
    assert np.array_equal(ix.cpu().numpy(), ti) and np.array_equal(d2.cpu().numpy().view(np.uint32), td.view(np.uint32))
    assert np.array_equal(labels.cpu().numpy(), twin("nonfinite")["labels"])


def test_empty_and_unusable_inputs_succeed():
    import torch
    from r3g import cloud, ffi
    zero = dict(zip(R.REPORT, (0, 0, 0, 0, 0, -1, 0)))
    labels, counts, rep = cloud.dbscan(torch.zeros((0, 3), device="cuda"), 0.1, 3, counts=True)
    assert labels.numel() == 0 and counts.numel() == 0 and report_of(rep) == zero
    labels, counts, rep = cloud.dbscan(dev(np.full((70, 3), np.nan)), 0.1, 1, counts=True)
    assert (labels.cpu().numpy() == -1).all() and (counts.cpu().numpy() == 0).all() and report_of(rep) == zero
    with ffi.device_lock(0), pytest.raises(ffi.R3GError):     # such a call leaves the context without a cloud
        cloud.knn(dev(np.zeros((1, 3))), 1)


def test_times_belong_to_the_last_complete_run():
    """r3g_cloud_dbscan_times on a context of its own: R3G_ERR_STATE before any run, five finite non-negative intervals after one
    (inside the call, so their sum is at most its wall time between two synchronisations), and R3G_ERR_STATE again after a call
    that clustered nothing (no point, or no usable one: both succeed)"""
    import time
    import torch
    from r3g import cloud, ffi
    L = ffi.lib()
    rng = np.random.default_rng(5)
    blobs = np.concatenate([rng.normal(c, 0.02, (200, 3)) for c in (0.0, 5.0)])      # two blobs of 200 points, 8.7 apart
    p, nan = dev(blobs), dev(np.full((70, 3), np.nan))
    lab = torch.zeros(len(blobs), dtype=torch.int32, device="cuda")
    rep, ms = (ctypes.c_int64 * 8)(), (ctypes.c_double * len(cloud.DBSCAN_PASSES))()
    ctx = ffi.new_context(0)

    def run(pts, n):
        return L.r3g_cloud_dbscan(ctx, ctypes.c_void_p(pts.data_ptr()), n, 0.2, 4, 0, ctypes.c_void_p(lab.data_ptr()), None, rep, ffi.stream_ptr())

    try:
        assert L.r3g_cloud_dbscan_times(ctx, ms) == ERR_STATE
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ffi.check(run(p, len(blobs)))
        torch.cuda.synchronize()
        wall_ms = 1e3 * (time.perf_counter() - t0)
        assert dict(zip(R.REPORT, rep))["n_clusters"] == 2 and sorted(np.bincount(lab.cpu().numpy()).tolist()) == [200, 200]
        ffi.check(L.r3g_cloud_dbscan_times(ctx, ms))
        print("dbscan passes (ms):", list(ms), "wall (ms):", wall_ms)
        assert len(ms) == 5 and all(np.isfinite(v) and v >= 0.0 for v in ms) and sum(ms) <= wall_ms
        ffi.check(run(p, 0))
        assert L.r3g_cloud_dbscan_times(ctx, ms) == ERR_STATE
        ffi.check(run(p, len(blobs)))
        ffi.check(L.r3g_cloud_dbscan_times(ctx, ms))
        ffi.check(run(nan, 70))
        assert L.r3g_cloud_dbscan_times(ctx, ms) == ERR_STATE
        assert L.r3g_cloud_dbscan_times(ctx, None) == -1 and L.r3g_cloud_dbscan_times(None, ms) == -1
    finally:
        torch.cuda.synchronize()
        L.r3g_destroy(ctx)


def test_refusals():
    import torch
    from r3g import cloud, ffi
    p = dev(R.clouds()["n63"][0])
    for kw in (dict(eps=0.0), dict(eps=-0.1), dict(eps=float("nan")), dict(eps=float("inf")), dict(min_samples=0), dict(min_samples=-3),
               dict(resolution=257), dict(resolution=-1)):
        args = dict(eps=0.2, min_samples=3, resolution=None)
        args.update(kw)
        with pytest.raises(ffi.R3GError):
            cloud.dbscan(p, **args)
    lib, ctx = ffi.lib(), ffi.context(0)
    lab = torch.zeros(63, dtype=torch.int32, device="cuda")
    rep = (ctypes.c_int64 * 8)()
    with ffi.device_lock(0):
        n0 = ffi.counter("dbscan_launches")
        for n in (-1, 2 ** 31):
            assert lib.r3g_cloud_dbscan(ctx, ctypes.c_void_p(p.data_ptr()), n, 0.2, 3, 0, ctypes.c_void_p(lab.data_ptr()), None, rep, None) != 0
        assert lib.r3g_cloud_dbscan(ctx, None, 63, 0.2, 3, 0, ctypes.c_void_p(lab.data_ptr()), None, rep, None) != 0
        assert lib.r3g_cloud_dbscan(ctx, ctypes.c_void_p(p.data_ptr()), 63, 0.2, 3, 0, None, None, rep, None) != 0
        assert ffi.counter("dbscan_launches") == n0           # refused before any launch
    with pytest.raises(ValueError):
        cloud.dbscan(torch.zeros((4, 3)), 0.1, 3)             # there is no CPU path


def test_filters_equal_the_reference_on_the_goldens():
    import torch
    from r3g import cloud
    pts, expect = R.golden()
    for name, (_, eps, ms, _) in R.RANDOM.items():
        e = expect["clouds"][name]
        dp = dev(pts[name])
        kept = cloud.filter_dbscan(dp, eps, ms)
        assert np.array_equal(kept.cpu().numpy(), pts[name][e["dbscan_keep"]]), name
        if e["quantile_keep"] is not None:
            kept = cloud.filter_points_by_quantile(dp, e["q"])
            assert np.array_equal(kept.cpu().numpy(), pts[name][e["quantile_keep"]]), name
    lone = dev(R.clouds()["isolated"][0])
    assert cloud.filter_dbscan(lone, 0.25, 2) is lone                        # no cluster: the input itself
    empty = torch.zeros((0, 3), device="cuda")
    assert cloud.filter_dbscan(empty) is empty and cloud.filter_points_by_quantile(empty) is empty


def test_pointcloud_stand_in():
    from r3g import cloud
    p, eps, ms = R.clouds()["blobs"]
    colours = np.random.default_rng(3).integers(0, 256, (len(p), 3)).astype(np.uint8)
    pc = cloud.PointCloud(p, colours)
    labels, rep = pc.dbscan(eps, ms)
    assert np.array_equal(labels, twin("blobs")["labels"]) and report_of(rep) == twin("blobs")["report"]
    big = pc.largest_cluster(eps, ms)
    rows = R.largest_cluster_rows(twin("blobs")["labels"])
    assert np.array_equal(big.vertices, pc.vertices[rows]) and np.array_equal(big.colors, colours[rows]) and big.normals is None
