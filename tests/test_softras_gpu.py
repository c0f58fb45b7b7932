"""The soft silhouette on the device (r3g.softras, include/r3g.h "soft silhouettes") against its host twin
(tests/emu/softras_emu.cpp, the same text as csrc/softras_core.h): alpha, face, dist, zbuf, grad_face, grad_pos and both reports,
bit for bit.  What the twin's numbers are worth is the CPU test's business (tests/test_softras_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

import emu_softras as E
import softras_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def device_run(sc, grad_alpha):
    from r3g import softras
    pos, tri = torch.from_numpy(sc["pos"]).cuda(), torch.from_numpy(sc["tri"]).cuda()
    args = (pos, tri, sc["size"], sc["K"], sc["sigma"], sc["blur"])
    alpha, face, dist, zbuf, rep = softras.forward_raw(*args)
    gf, gp, brep = softras.backward_raw(*args, face, dist, torch.from_numpy(grad_alpha).cuda())
    out = {k: v.cpu().numpy() for k, v in (("alpha", alpha), ("face", face), ("dist", dist), ("zbuf", zbuf), ("grad_face", gf), ("grad_pos", gp))}
    out["report"] = {k: rep[k] for k in E.REPORT}
    out["back_report"] = {k: brep[k] for k in E.BACK_REPORT}
    return out


def twin_run(sc, grad_alpha):
    args = (sc["pos"], sc["tri"], sc["size"], sc["K"], sc["sigma"], sc["blur"])
    out = E.forward(*args)
    b = E.backward(*args, out["face"], out["dist"], grad_alpha)
    out.update(grad_face=b["grad_face"], grad_pos=b["grad_pos"], back_report=b["report"])
    return out


def grad_alpha_of(sc, seed=5):
    return np.random.default_rng(seed).uniform(-1, 1, sc["size"]).astype(np.float32)


def check(sc, grad_alpha=None):
    ga = grad_alpha_of(sc) if grad_alpha is None else grad_alpha
    dev, twin = device_run(sc, ga), twin_run(sc, ga)
    assert dev["report"] == twin["report"] and dev["back_report"] == twin["back_report"]
    for k in ("face", "alpha", "dist", "zbuf", "grad_face", "grad_pos"):
        assert dev[k].shape == twin[k].shape, k
        assert np.array_equal(_bits(dev[k]), _bits(twin[k])), k
    return dev


@pytest.mark.parametrize("size", [(1, 1), (7, 9), (8, 8), (9, 7), (63, 65), (65, 63), (1, 65), (8, 63)])
def test_image_sizes(size):
    dev = check(R.random_scene(21, size=size, F=24, K=6, sigma=0.7))
    assert dev["report"]["tiles"] == ((size[0] + 7) // 8) * ((size[1] + 7) // 8)


@pytest.mark.parametrize("K", [1, 2, 20, 32])
def test_list_lengths(K):
    dev = check(R.random_scene(22, F=80, K=K, sigma=1.0, spread=0.6))
    assert (dev["face"][..., -1] >= 0).any() or K > 20      # some pixel fills its list


@pytest.mark.parametrize("F", [0, 1, 63, 64, 65])
def test_face_counts(F):
    dev = check(R.random_scene(23, F=F, K=5))
    if F == 0:
        assert not dev["alpha"].any() and np.all(dev["face"] == -1)
    else:
        assert dev["alpha"].any()


@pytest.mark.parametrize("name", sorted(R.named_scenes()))
def test_named_scenes(name):
    dev = check(R.named_scenes()[name])
    if name == "full_cover":
        assert dev["back_report"]["found"] == 63 * 65 and np.abs(dev["grad_pos"]).max() > 0
    if name == "saturate":
        assert set(np.unique(dev["alpha"]).tolist()) <= {0.0, 1.0} and np.abs(dev["grad_pos"]).max() < 1e-15
    if name == "stacked":
        assert (dev["face"][..., -1] >= 0).any()


def test_shared_vertices():
    dev = check(R.shared_scene(3))
    assert np.abs(dev["grad_pos"][:, :2]).max() > 0 and not dev["grad_pos"][:, 2].any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e30, -1e30])
def test_vertices_that_cannot_be_drawn(bad):
    for column in range(3):
        sc = R.random_scene(24, F=20, K=4)
        sc["pos"][7, column] = bad
        dev = check(sc)
        assert dev["report"]["skipped"] == 1
        assert np.all(np.isfinite(dev["alpha"])) and np.all(np.isfinite(dev["grad_pos"])) and not (dev["face"] == 2).any()


def test_index_outside_the_vertices():
    sc = R.random_scene(25, F=20, K=4)
    sc["tri"][3, 1] = 60
    sc["tri"][9, 0] = -1
    assert check(sc)["report"]["skipped"] == 2


def test_grad_alpha_with_nan_and_inf():
    sc = R.random_scene(26, F=30, K=6, sigma=1.0)
    ga = grad_alpha_of(sc)
    ga[5, 7], ga[11, 3], ga[20, 20] = np.nan, np.inf, -np.inf
    dev = check(sc, ga)
    clean = ga.copy()
    clean[5, 7] = clean[11, 3] = clean[20, 20] = 0.0      # "contributes nothing": the same bits as a zero there
    assert np.array_equal(_bits(dev["grad_pos"]), _bits(device_run(sc, clean)["grad_pos"]))
    assert np.all(np.isfinite(dev["grad_pos"]))


def test_refusals():
    from r3g import ffi, softras
    sc = R.random_scene(27, F=8, K=4)
    pos, tri = torch.from_numpy(sc["pos"]).cuda(), torch.from_numpy(sc["tri"]).cuda()

    def refused(**kw):
        a = dict(size=sc["size"], K=4, sigma=0.5, blur_radius=1.0)
        a.update(kw)
        with pytest.raises(ffi.R3GError) as e:
            softras.forward_raw(pos, tri, a["size"], a["K"], a["sigma"], a["blur_radius"])
        assert e.value.code == -1
        face = torch.full((max(a["size"][0], 1), max(a["size"][1], 1), max(a["K"], 1)), -1, dtype=torch.int32, device="cuda")
        with pytest.raises((ffi.R3GError, ValueError)) as e:
            softras.backward_raw(pos, tri, a["size"], a["K"], a["sigma"], a["blur_radius"], face, face.float(),
                                 torch.zeros(face.shape[:2], device="cuda"))
        assert isinstance(e.value, ValueError) or e.value.code == -1
    for K in (0, -1, 33):
        refused(K=K)
    for sigma in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        refused(sigma=sigma)
    for blur in (-1.0, float("nan")):
        refused(blur_radius=blur)
    for size in ((0, 8), (8, 0), (-1, 8), (16385, 8)):
        refused(size=size)
    # null buffers with non-zero sizes, straight at the C boundary
    L, ctx, rep = ffi.lib(), ffi.context(0), (ctypes.c_int64 * 8)()
    H, W = sc["size"]
    alpha = torch.zeros(H, W, device="cuda")
    face = torch.zeros(H, W, 4, dtype=torch.int32, device="cuda")
    dist, zbuf = face.float(), face.float()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    good = [ctx, p(pos), pos.shape[0], p(tri), tri.shape[0], H, W, 4, 0.5, 1.0, p(alpha), p(face), p(dist), p(zbuf), rep, ffi.stream_ptr()]
    assert L.r3g_softras_forward(*good) == 0
    for i in (1, 3, 10, 11, 12, 13, 14, 0):
        bad = list(good)
        bad[i] = None
        assert L.r3g_softras_forward(*bad) == -1, i
    cs, ci = softras.corner_csr(tri, pos.shape[0])
    gf, gp = torch.zeros(tri.shape[0], 3, 2, device="cuda"), torch.zeros(pos.shape[0], 3, device="cuda")
    brep = (ctypes.c_int64 * 4)()
    good = [ctx, p(pos), pos.shape[0], p(tri), tri.shape[0], H, W, 4, 0.5, 1.0, p(face), p(dist), p(alpha), p(cs), p(ci), p(gf), p(gp), brep,
            ffi.stream_ptr()]
    assert L.r3g_softras_backward(*good) == 0
    for i in (1, 3, 10, 11, 12, 13, 14, 15, 16, 17, 0):
        bad = list(good)
        bad[i] = None
        assert L.r3g_softras_backward(*bad) == -1, i
    assert L.r3g_softras_times(ctx, None) == -1
    torch.cuda.synchronize()


def test_zero_sizes_need_no_buffers():
    from r3g import softras
    empty_p, empty_t = torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    alpha, face, dist, zbuf, rep = softras.forward_raw(empty_p, empty_t, (9, 10), 3, 0.5, 1.0)
    assert not alpha.any() and bool((face == -1).all()) and rep["pairs"] == 0
    gf, gp, brep = softras.backward_raw(empty_p, empty_t, (9, 10), 3, 0.5, 1.0, face, dist, torch.ones(9, 10, device="cuda"))
    assert gf.shape == (0, 3, 2) and gp.shape == (0, 3) and brep["found"] == 0


def test_two_calls_give_the_same_bytes():
    sc = R.random_scene(28, size=(65, 63), F=65, K=20, sigma=1.5, spread=0.6)
    ga = grad_alpha_of(sc)
    a, b = device_run(sc, ga), device_run(sc, ga)
    for k in ("face", "alpha", "dist", "zbuf", "grad_face", "grad_pos"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_autograd_gives_the_raw_gradient():
    from r3g import softras
    sc = R.shared_scene(4)
    tri = torch.from_numpy(sc["tri"]).cuda()
    pos = torch.from_numpy(sc["pos"]).cuda().requires_grad_(True)
    ga = torch.from_numpy(grad_alpha_of(sc)).cuda()
    alpha, face, dist, zbuf = softras.rasterize(pos * 1.0, tri, sc["size"], K=sc["K"], sigma=sc["sigma"], blur_radius=sc["blur"])
    assert alpha.requires_grad and not face.requires_grad and not dist.requires_grad
    (alpha * ga).sum().backward()
    _, gp, _ = softras.backward_raw(pos, tri, sc["size"], sc["K"], sc["sigma"], sc["blur"], face, dist, ga)
    assert torch.equal(pos.grad, gp) and bool(pos.grad[:, :2].abs().max() > 0)
    # the default blur radius is the reference's ln(1 / 1e-4 - 1) sigma
    a2 = softras.rasterize(pos.detach(), tri, sc["size"], K=sc["K"], sigma=sc["sigma"])[0]
    a3 = softras.forward_raw(pos.detach(), tri, sc["size"], sc["K"], sc["sigma"], R.default_blur(sc["sigma"]))[0]
    assert torch.equal(a2, a3)


def test_times():
    from r3g import softras
    check(R.random_scene(29, F=16, K=4))
    ms = softras.times()
    assert set(ms) == set(softras.PASSES) and all(v >= 0 for v in ms.values())
