"""Normal orientation on the GPU (include/r3g.h r3g_cloud_orient, r3g.cloud.orient_normals): sign, tree and report equal the host
twin of csrc/orient_core.h (tests/emu_orient.py) exactly, on the clouds of tests/test_orient_cpu.py and across block and wave
boundaries; the refusals of include/r3g.h; the result does not depend on the resolution of the cloud the rows come from."""
import ctypes

import numpy as np
import pytest

import emu_orient as emu
import orient_ref as R

pytestmark = pytest.mark.gpu

CLOUDS = R.clouds()
_UNIFORM = {}


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _device(p, nr, k):
    from r3g import cloud, ffi
    with ffi.device_lock(0):
        out, info = cloud.orient_normals(dev(p), dev(nr), k)
    rep = {f: int(info[f]) for f in emu.REPORT_FIELDS}
    return out.cpu().numpy(), info["sign"].cpu().numpy(), info["tree"].cpu().numpy(), rep


def _uniform(n):
    if n not in _UNIFORM:
        _UNIFORM[n] = R.random_cloud(n, 100 + n)
    return _UNIFORM[n]


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_device_equals_the_twin_exactly(name):
    p, nr, k = CLOUDS[name]
    out, sign, tree, rep = _device(p, nr, k)
    s, t, r = emu.orient(p, nr, k)
    assert np.array_equal(sign, s) and np.array_equal(tree, t) and rep == r
    want = np.where((s < 0)[:, None], -nr, nr)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))           # a point that is not usable keeps its normal's bits


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 4097))
@pytest.mark.parametrize("k", (1, 8, 31))
def test_sizes_across_wave_and_block_boundaries(n, k):
    p, nr = _uniform(n)
    _, sign, tree, rep = _device(p, nr, k)
    s, t, r = emu.orient(p, nr, k)
    assert np.array_equal(sign, s) and np.array_equal(tree, t) and rep == r


def test_coin_flipped_sphere_ends_outward():
    from r3g import ffi
    p, nr = R.fibonacci_sphere(4096)
    flipped = R.coin_flipped(nr, 7)
    r0 = ffi.counter("orient_rounds")
    out, sign, tree, rep = _device(p, flipped, 8)
    assert ((out.astype(np.float64) * p.astype(np.float64)).sum(1) > 0).all()
    assert rep["frustrated"] == 0 and rep["trees"] == 1 and (tree == 0).all()
    assert ffi.counter("orient_rounds") - r0 == rep["rounds"]


def test_refusals():
    import torch
    from r3g import ffi
    p, nr = _uniform(65)
    dp, dn = dev(p), dev(nr)
    sign = torch.zeros(65, dtype=torch.int8, device="cuda")
    tree = torch.zeros(65, dtype=torch.int32, device="cuda")
    L, ctx = ffi.lib(), ffi.context(0)

    def call(points, normals, n, k, s=sign, t=tree, res=0):
        return L.r3g_cloud_orient(ctx, points, normals, n, k, res, ctypes.c_void_p(s.data_ptr()) if s is not None else None,
                                  ctypes.c_void_p(t.data_ptr()) if t is not None else None, None, ffi.stream_ptr())

    P, N = ctypes.c_void_p(dp.data_ptr()), ctypes.c_void_p(dn.data_ptr())
    with ffi.device_lock(0):
        for k in (0, 32, -3):
            assert call(P, N, 65, k) == -1 and b"k outside" in L.r3g_last_error()
        assert call(P, N, 65, 8, res=-1) == -1 and call(P, N, 65, 8, res=257) == -1
        assert call(P, N, 0, 8) == -1 and call(P, N, -5, 8) == -1 and call(P, N, 2 ** 31, 8) == -1
        assert call(None, N, 65, 8) == -1 and call(P, None, 65, 8) == -1
        assert call(P, N, 65, 8, s=None) == -1 and call(P, N, 65, 8, t=None) == -1
        assert call(P, N, 65, 8) == 0
        # no usable point: success, every sign 0 and every tree -1
        nan = torch.full((65, 3), float("nan"), device="cuda")
        assert call(ctypes.c_void_p(nan.data_ptr()), N, 65, 8) == 0
    assert not sign.any() and (tree == -1).all()


def test_top_level_clamps_k_to_31():
    from r3g import cloud, ffi
    p, nr = _uniform(65)
    with ffi.device_lock(0):
        _, info = cloud.orient_normals(dev(p), dev(nr), 100)
    assert info["k"] == 31
    s, t, r = emu.orient(p, nr, 31)
    assert np.array_equal(info["sign"].cpu().numpy(), s)


@pytest.mark.parametrize("name", ("random500", "tripled", "nonfinite"))
def test_result_does_not_depend_on_the_clouds_resolution(name):
    """the rows are r3g_cloud_knn's, which the grid only prunes"""
    from r3g import cloud, ffi
    p, nr, k = CLOUDS[name]
    s, t, r = emu.orient(p, nr, k)
    for res in (1, 3, 16, None):
        with ffi.device_lock(0):
            _, info = cloud.orient_normals(dev(p), dev(nr), k, resolution=res)
        assert np.array_equal(info["sign"].cpu().numpy(), s) and np.array_equal(info["tree"].cpu().numpy(), t), res
        assert {f: int(info[f]) for f in emu.REPORT_FIELDS} == r, res
