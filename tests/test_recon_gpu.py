"""Poisson surface on the GPU (include/r3g.h r3g_recon_splat / _solve / _sample, r3g/recon.py): channels, divergence, chi, level
and sampled densities equal the host twin of csrc/recon_core.h (tests/emu_recon.py) bit for bit; the mesh of `reconstruct`
equals marching cubes of the twin's chi; writes stay inside their buffers; the refusals of include/r3g.h; and the reference's
`mesh_pointcloud` end to end on a sphere."""
import ctypes

import numpy as np
import pytest

import emu_mc
import emu_recon as emu
import orient_ref
import recon_ref as R

pytestmark = pytest.mark.gpu

DEPTHS = (2, 3, 4, 5)
_CACHE = {}


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _case(depth):
    """depth -> the cloud, its box and everything the twin makes of it, computed once and left unchanged"""
    if depth not in _CACHE:
        p, nr = R.fibonacci_sphere(4097 if depth == 5 else 600)
        p = (p * np.array([1.0, 0.8, 0.6], np.float32) + np.array([0.3, -0.2, 0.1], np.float32)).astype(np.float32)
        p[7, 0], nr[11], nr[13, 2] = np.nan, 0.0, np.inf
        centre, side, h = R.box(p, nr, depth)
        ch, used = emu.splat(p, nr, depth, centre, side)
        b = emu.rhs(ch, depth, centre, side)
        chi = {c: emu.vcycles(b, depth, side, c) for c in (1, 10)}
        _, total, count = emu.sample(chi[10], depth, centre, side, p, nr)
        case = dict(p=p, nr=nr, centre=centre, side=side, h=h, ch=ch, used=used, b=b, chi=chi, total=total, count=count)
        for a in (ch, b, chi[1], chi[10]):
            a.setflags(write=False)
        _CACHE[depth] = case
    return _CACHE[depth]


@pytest.mark.parametrize("depth", DEPTHS)
def test_b_chi_and_level_equal_the_twin_bit_for_bit(depth):
    from r3g import ffi, recon
    c = _case(depth)
    with ffi.device_lock(0):
        centre, side, h = recon.box(dev(c["p"]), dev(c["nr"]), depth)
        assert np.array_equal(centre, c["centre"]) and side == c["side"] and h == c["h"]
        used, ch = recon.splat(dev(c["p"]), dev(c["nr"]), depth, centre, side, want_channels=True)
        assert used == c["used"] == len(c["p"]) - 3
        assert np.array_equal(ch.cpu().numpy(), c["ch"])                     # the four int64 channels
        for cycles in (1, 10):
            s0, c0 = ffi.counter("recon_solves"), ffi.counter("recon_cycles")
            chi, b = recon.solve(depth, "cuda:0", cycles, want_b=True)
            assert (ffi.counter("recon_solves") - s0, ffi.counter("recon_cycles") - c0) == (1, cycles)
            assert np.array_equal(R.bits(b.cpu().numpy()), R.bits(c["b"]))
            assert np.array_equal(R.bits(chi.cpu().numpy()), R.bits(c["chi"][cycles])), cycles
        _, total, count = recon.sample(1, dev(c["p"]), dev(c["nr"]))
    assert (total, count) == (c["total"], c["count"])
    assert recon.level_from_sum(total, count) == (c["total"] / 2.0 ** 30) / c["count"]


@pytest.mark.parametrize("depth", DEPTHS)
def test_density_sampled_at_every_node(depth):
    """the density channel read back through r3g_recon_sample at (about) every node of the lattice"""
    from r3g import ffi, recon
    c = _case(depth)
    n = R.nodes(depth)
    lo = c["centre"] - 0.5 * c["side"]
    idx = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    with ffi.device_lock(0):
        recon.splat(dev(c["p"]), dev(c["nr"]), depth, c["centre"], c["side"])
        pts = (lo + idx * c["h"]).astype(np.float32)
        v, total, count = recon.sample(0, dev(pts))
    v_twin, total_twin, count_twin = emu.sample(c["ch"][0], depth, c["centre"], c["side"], pts)
    assert np.array_equal(R.bits(v.cpu().numpy()), R.bits(v_twin)) and (total, count) == (total_twin, count_twin)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_sampled_densities_equal_the_twin(n):
    from r3g import ffi, recon
    c = _case(5)
    rng = np.random.default_rng(n)
    q = (c["centre"] + (rng.random((n, 3)) - 0.5) * c["side"] * 1.05).astype(np.float32)       # a few fall outside the box: clamped
    if n > 1:
        q[1, 1] = np.nan
    with ffi.device_lock(0):
        recon.splat(dev(c["p"]), dev(c["nr"]), 5, c["centre"], c["side"])
        recon.solve(5, "cuda:0", 10)
        for field, data in ((0, c["ch"][0]), (1, c["chi"][10])):
            v, total, count = recon.sample(field, dev(q))
            v_twin, total_twin, count_twin = emu.sample(data, 5, c["centre"], c["side"], q)
            assert np.array_equal(R.bits(v.cpu().numpy()), R.bits(v_twin)), (n, field)
            assert (total, count) == (total_twin, count_twin) and count == n - (n > 1)


def test_reconstruct_equals_marching_cubes_of_the_twins_chi():
    from r3g import ffi, recon
    c = _case(5)
    mesh, dens, info = recon.reconstruct(dev(c["p"]), dev(c["nr"]), depth=5)
    level = (c["total"] / 2.0 ** 30) / c["count"]
    assert info["level"] == level and info["usable"] == c["used"] and info["n"] == 33 and 0 <= info["residual"] < 1e-3
    v, f, _ = emu_mc.marching_cubes(c["chi"][10], level, False, recon.lattice_xform(5, c["centre"], c["side"]), recon.REVERSE_FACES["mc"])
    dv, df = mesh.device_buffers()
    assert np.array_equal(df.cpu().numpy(), f) and np.array_equal(R.bits(dv.cpu().numpy()), R.bits(v))
    d_twin = emu.sample(c["ch"][0], 5, c["centre"], c["side"], v)[0]
    assert np.array_equal(R.bits(dens.cpu().numpy()), R.bits(d_twin))
    assert mesh.is_volume                                                      # outward normals: closed, consistent, positive volume
    flipped = recon.reconstruct(dev(c["p"]), dev(-c["nr"]), depth=5)[0]
    assert flipped.is_watertight and flipped.volume == pytest.approx(-mesh.volume, rel=1e-6)
    dual = recon.reconstruct(dev(c["p"]), dev(c["nr"]), depth=5, mc_algo="dmc")[0]
    assert dual.is_volume
    with pytest.raises(ValueError):
        recon.reconstruct(dev(c["p"]), dev(c["nr"]), depth=5, mc_algo="cubes")


def test_outputs_stay_inside_nan_filled_guards():
    import torch
    from r3g import ffi
    c = _case(3)
    n3, guard = R.nodes(3) ** 3, 64
    nq = 65
    q = dev(c["p"][:nq])
    bufs = {name: torch.full((size + 2 * guard,), float("nan"), device="cuda") for name, size in (("b", n3), ("chi", n3), ("v", nq))}
    inner = {name: t[guard:-guard] for name, t in bufs.items()}
    L, ctx = ffi.lib(), ffi.context(0)
    cen = np.ascontiguousarray(c["centre"], np.float64)
    dp, dn = dev(c["p"]), dev(c["nr"])
    with ffi.device_lock(0):
        ffi.check(L.r3g_recon_splat(ctx, dp.data_ptr(), dn.data_ptr(), len(c["p"]), 3, cen.ctypes.data, c["side"], None, None, ffi.stream_ptr()))
        ffi.check(L.r3g_recon_solve(ctx, 10, inner["b"].data_ptr(), inner["chi"].data_ptr(), ffi.stream_ptr()))
        ffi.check(L.r3g_recon_sample(ctx, 1, q.data_ptr(), None, nq, inner["v"].data_ptr(), None, None, ffi.stream_ptr()))
    torch.cuda.synchronize()
    nan_bits = np.float32(np.nan).view(np.uint32)
    for name, t in bufs.items():
        host = t.cpu().numpy().view(np.uint32)
        assert (host[:guard] == nan_bits).all() and (host[-guard:] == nan_bits).all(), name
    assert np.array_equal(R.bits(inner["chi"].cpu().numpy()), R.bits(c["chi"][10]).reshape(-1))
    assert np.array_equal(R.bits(inner["b"].cpu().numpy()), R.bits(c["b"]).reshape(-1))


def test_refusals_and_call_order():
    import torch
    from r3g import ffi
    c = _case(3)
    L = ffi.lib()
    ctx = ffi.new_context(0)                                                  # a context of its own: nothing splatted yet
    dp, dn = dev(c["p"]), dev(c["nr"])
    n = len(c["p"])
    cen = np.ascontiguousarray(c["centre"], np.float64)
    chi = torch.empty(R.nodes(3) ** 3, device="cuda")
    v = torch.empty(n, device="cuda")
    S = ffi.stream_ptr()
    try:
        with ffi.device_lock(0):
            assert L.r3g_recon_solve(ctx, 10, None, chi.data_ptr(), S) == -4                      # R3G_ERR_STATE
            assert L.r3g_recon_sample(ctx, 0, dp.data_ptr(), None, n, v.data_ptr(), None, None, S) == -4

            def splat(points=dp.data_ptr(), normals=dn.data_ptr(), count=n, depth=3, centre=cen.ctypes.data, side=c["side"]):
                return L.r3g_recon_splat(ctx, points, normals, count, depth, centre, side, None, None, S)

            for bad in (dict(depth=1), dict(depth=9), dict(count=0), dict(count=-1), dict(count=2 ** 31), dict(points=None),
                        dict(normals=None), dict(centre=None), dict(side=0.0), dict(side=float("nan")), dict(side=float("inf"))):
                assert splat(**bad) == -1, bad
            assert L.r3g_recon_solve(ctx, 10, None, chi.data_ptr(), S) == -4                      # a refused splat leaves no state
            nan = torch.full((n, 3), float("nan"), device="cuda")
            assert splat(points=nan.data_ptr()) == -1 and b"no usable point" in L.r3g_last_error()
            assert splat() == 0
            assert L.r3g_recon_sample(ctx, 0, dp.data_ptr(), None, n, v.data_ptr(), None, None, S) == 0
            assert L.r3g_recon_sample(ctx, 1, dp.data_ptr(), None, n, v.data_ptr(), None, None, S) == -4      # chi needs a solve
            assert L.r3g_recon_solve(ctx, -1, None, chi.data_ptr(), S) == -1 and L.r3g_recon_solve(ctx, 1001, None, None, S) == -1
            assert L.r3g_recon_solve(ctx, 10, None, chi.data_ptr(), S) == 0
            assert np.array_equal(R.bits(chi.cpu().numpy()), R.bits(c["chi"][10]).reshape(-1))
            assert L.r3g_recon_sample(ctx, 1, dp.data_ptr(), None, n, v.data_ptr(), None, None, S) == 0
            assert L.r3g_recon_sample(ctx, 2, dp.data_ptr(), None, n, v.data_ptr(), None, None, S) == -1
            assert L.r3g_recon_sample(ctx, 0, dp.data_ptr(), None, 0, v.data_ptr(), None, None, S) == -1
            assert L.r3g_recon_sample(ctx, 0, None, None, n, v.data_ptr(), None, None, S) == -1
            assert splat(depth=9) == -1                                                           # a failed splat drops the state
            assert L.r3g_recon_sample(ctx, 0, dp.data_ptr(), None, n, v.data_ptr(), None, None, S) == -4
    finally:
        L.r3g_destroy(ctx)


def test_point_cloud_to_mesh_with_its_own_normals():
    """`.normals` given: reconstruct + trim, no repairs -- fewer vertices than the closed surface, still wound outward"""
    from r3g import cloud, recon
    c = _case(5)
    ok = R.usable(c["p"], c["nr"])
    mesh = cloud.PointCloud(c["p"][ok], normals=c["nr"][ok]).to_mesh(depth=5, trim_quantile=0.05)
    full = recon.reconstruct(dev(c["p"]), dev(c["nr"]), depth=5)[0]
    assert 0.85 * full.n_vertices < mesh.n_vertices <= 0.951 * full.n_vertices     # 5 % below the quantile, plus what they orphan
    assert mesh.is_winding_consistent and not mesh.is_watertight and mesh.volume > 0
    assert mesh.metadata["recon"]["depth"] == 5


def test_mesh_pointcloud_on_a_sphere():
    """4 096 points of a unit sphere, nothing else given (the function estimates and orients its own normals), depth 5: the
    result is to be watertight, consistently wound and of positive volume.  The 2.5 % trim removes patches that touch at pinch
    vertices here (64 boundary edges tangled for `Mesh.fill_holes`, one hole around a patch that hangs on a single vertex):
    this is the case `recon.fill_pinched_loops` is for.  Measured: 1 830 vertices, 3 654 faces, volume 4.165, no broken face."""
    from r3g import recon
    p, _ = orient_ref.fibonacci_sphere(4096)
    mesh = recon.mesh_pointcloud(dev(p), depth=5)
    print("mesh_pointcloud: %d vertices, %d faces, watertight %s, winding %s, volume %.4f, metadata %s" % (
        mesh.n_vertices, mesh.n_faces, mesh.is_watertight, mesh.is_winding_consistent, mesh.volume, mesh.metadata))
    assert mesh.is_volume
