"""Face-to-cloud distance on the GPU (include/r3g.h r3g_cloud_faces / _backward / _times, r3g/cloud.py face_nearest and
FaceCloudDistance): bit for bit against the host twin of csrc/facecloud_core.h (tests/emu_facecloud.py) on dist2, index, weights, diff,
grad_verts and the report, over the sizes, placements and invalid inputs of DESIGN.md section 4p; guard buffers, repeatability,
autograd against the raw call, the refusals, and the cloud left as it was."""
import ctypes

import numpy as np
import pytest

import emu_facecloud as emu
import facecloud_ref as R

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 64, 65, 4097)
FS = (0, 1, 63, 64, 65, 257)
RESOLUTIONS = (1, 3, 16, None)
GUARD = 64                      # float32 / int32 words on either side of every output
INVALID, STATE = -1, -4


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Guarded:
    """an output of `words` 4-byte words inside a NaN-filled buffer with GUARD words on either side, which must keep every bit"""

    def __init__(self, words, dtype):
        import torch
        self.buf = torch.full((words + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.fill = self.buf.cpu().numpy().view(np.uint32).copy()
        self.words, self.dtype = words, dtype

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def read(self, shape):
        raw = self.buf.cpu().numpy().view(np.uint32)
        assert np.array_equal(raw[:GUARD], self.fill[:GUARD]) and np.array_equal(raw[GUARD + self.words:], self.fill[GUARD + self.words:])
        return raw[GUARD:GUARD + self.words].view(self.dtype).reshape(shape).copy()


def raw_forward(ctx, v, f, n_faces):
    """r3g_cloud_faces on the first n_faces faces, outputs in guarded buffers -> (dist2, index, weights, diff, report)"""
    from r3g import ffi
    out = [Guarded(n_faces, np.float32), Guarded(n_faces, np.int32), Guarded(3 * n_faces, np.float32), Guarded(3 * n_faces, np.float32)]
    rep = (ctypes.c_int64 * 4)()
    ffi.check(ffi.lib().r3g_cloud_faces(ctx, ctypes.c_void_p(v.data_ptr()), v.shape[0], ctypes.c_void_p(f.data_ptr()), n_faces,
                                        *[o.ptr() for o in out], rep, ffi.stream_ptr()))
    shapes = [(n_faces,), (n_faces,), (n_faces, 3), (n_faces, 3)]
    return tuple(o.read(s) for o, s in zip(out, shapes)) + (dict(zip(emu.REPORT, (int(x) for x in rep))),)


def raw_backward(ctx, n_verts, g, index, weights, diff, csr):
    import torch
    from r3g import ffi
    out = Guarded(3 * n_verts, np.float32)
    t = [dev(g), dev(index, np.int32), dev(weights), dev(diff), dev(csr[0], np.int32), dev(csr[1], np.int32)]
    ffi.check(ffi.lib().r3g_cloud_faces_backward(ctx, n_verts, len(g), *[ctypes.c_void_p(x.data_ptr() if x.numel() else None) for x in t], out.ptr(),
                                                 ffi.stream_ptr()))
    torch.cuda.synchronize()
    return out.read((n_verts, 3))


def grad_vector(n, seed):
    """an incoming gradient with a NaN, a +inf and a -inf among ordinary values"""
    g = np.random.default_rng(seed).normal(size=n).astype(np.float32)
    for k, bad in ((2, np.nan), (17, np.inf), (70, -np.inf)):
        if k < n:
            g[k] = bad
    return g


@pytest.mark.parametrize("n", NS)
def test_device_equals_the_twin_bit_for_bit(n):
    """every N x resolution x F: the four outputs, the report and grad_verts, in guard buffers"""
    from r3g import cloud, ffi
    p = R.edge_cloud(n)
    v, f = R.edge_mesh()
    dv, df = dev(v), dev(f, np.int32)
    usable = int(np.isfinite(p).all(1).sum())
    with ffi.device_lock(0):
        ctx = ffi.context(0)
        for res in RESOLUTIONS:
            info = cloud.build(dev(p), res)
            assert info["skipped"] == n - usable
            for nf in FS:
                got = raw_forward(ctx, dv, df, nf)
                want = emu.grid(p, v, f[:nf], res or 0, mode="device")
                assert want[4].pop("resolution") == info["resolution"]
                for a, b in zip(got[:4], want[:4]):
                    assert np.array_equal(bits(a), bits(b)), (n, res, nf)
                assert got[4] == want[4], (n, res, nf)
                csr = emu.corner_csr(f[:nf], len(v))
                g = grad_vector(nf, 7)
                gv = raw_backward(ctx, len(v), g, got[1], got[2], got[3], csr)
                assert np.array_equal(bits(gv), bits(emu.gather(len(v), g, want[1], want[2], want[3], *csr))), (n, res, nf)


def test_the_placements_take_the_paths_they_are_meant_to():
    """resolution 16 over the unit cube: face 1's box is exactly kWideCells cells (narrow), face 2's one more (wide); the invalid faces
    get (NaN 0x7fc00000, -1, 0, 0); a vertex with 0, 1 and 65 corners"""
    from r3g import cloud, ffi
    p = R.edge_cloud(4097)
    v, f = R.edge_mesh()
    with ffi.device_lock(0):
        cloud.build(dev(p), 16)
        one = [raw_forward(ffi.context(0), dev(v), dev(f[k:k + 1], np.int32), 1)[4]["wide"] for k in range(5)]
        d2, ix, w, df, rep = raw_forward(ffi.context(0), dev(v), dev(f, np.int32), len(f))
    assert emu.wide_cells() == 64 and one == [0, 0, 1, 1, 0]
    bad = np.arange(8, 13)
    assert (bits(d2[bad]) == 0x7fc00000).all() and (ix[bad] == -1).all() and not bits(w[bad]).any() and not bits(df[bad]).any()
    assert rep["usable"] == len(f) - len(bad) and np.isfinite(d2[np.setdiff1d(np.arange(len(f)), bad)]).all()
    assert 5 not in ix                                        # the NaN point of the cloud is nobody's nearest
    start, _ = emu.corner_csr(f, len(v))
    corners = np.diff(start)
    assert corners[R.EDGE_HUB] == 65 and corners[41] == 1 and corners[42] == 0
    brute = emu.brute(p, v, f)
    for a, b in zip((d2, ix, w, df), brute[:4]):
        assert np.array_equal(bits(a), bits(b))


def test_two_calls_give_the_same_bytes_and_the_cloud_still_answers():
    from r3g import cloud, ffi
    import torch
    p = R.edge_cloud(4097)
    v, f = R.edge_mesh()
    q = dev(R.edge_cloud(300, seed=3)[10:])
    with ffi.device_lock(0):
        cloud.build(dev(p))
        before = [t.cpu().numpy() for t in cloud.knn(q, 8)]
        a = cloud.face_nearest(dev(v), dev(f, np.int32))
        b = cloud.face_nearest(dev(v), dev(f, np.int32))
        after = [t.cpu().numpy() for t in cloud.knn(q, 8)]
        csr = tuple(dev(x, np.int32) for x in emu.corner_csr(f, len(v)))
        g = dev(grad_vector(len(f), 9))
        ga = cloud.face_nearest_backward(g, a[1], a[2], a[3], csr, len(v))
        gb = cloud.face_nearest_backward(g, b[1], b[2], b[3], csr, len(v))
        times = cloud.faces_times(0)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert a[4] == b[4] and torch.equal(ga.view(torch.int32), gb.view(torch.int32))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, after))
    assert set(times) == set(cloud.FACES_PASSES) and all(t >= 0 for t in times.values())


def test_autograd_against_the_raw_call():
    import torch
    from r3g import cloud, softras
    p = R.edge_cloud(4097)
    v, f = R.edge_mesh()
    dv, df = dev(v).requires_grad_(True), dev(f, np.int32)
    csr = softras.corner_csr(df, len(v))
    want_csr = emu.corner_csr(f, len(v))
    assert np.array_equal(csr[0].cpu().numpy(), want_csr[0]) and np.array_equal(csr[1].cpu().numpy(), want_csr[1])
    weight = dev(np.random.default_rng(12).normal(size=len(f)).astype(np.float32))
    # (no ffi.device_lock around backward(): autograd runs the backward on a thread of its own, which takes the lock itself)
    cloud.build(dev(p))
    d2 = cloud.FaceCloudDistance.apply(dv, df, csr)
    ok = ~torch.isnan(d2.detach())
    (torch.where(ok, d2, torch.zeros_like(d2)) * weight).sum().backward()
    raw = cloud.face_nearest(dv, df)
    g = torch.where(ok, weight, torch.zeros_like(weight))
    want = cloud.face_nearest_backward(g, raw[1], raw[2], raw[3], csr, len(v))
    assert torch.equal(d2.detach().view(torch.int32), raw[0].view(torch.int32))
    assert torch.equal(dv.grad.view(torch.int32), want.view(torch.int32)) and bool(torch.isfinite(dv.grad).all())
    assert float(dv.grad.abs().max()) > 0 and not dv.grad[42].any()


def test_refusals_and_their_codes():
    import torch
    from r3g import ffi
    L = ffi.lib()
    ctx = ctypes.c_void_p()
    ffi.check(L.r3g_create(0, ctypes.byref(ctx)))
    try:
        v, f = R.edge_mesh()
        dv, df = dev(v), dev(f, np.int32)
        nv, nf = len(v), len(f)
        d2, ix = torch.empty(nf, device="cuda"), torch.empty(nf, dtype=torch.int32, device="cuda")
        w, diff = torch.empty((nf, 3), device="cuda"), torch.empty((nf, 3), device="cuda")
        gv = torch.empty((nv, 3), device="cuda")
        cs, ci = (dev(x, np.int32) for x in emu.corner_csr(f, nv))
        rep = (ctypes.c_int64 * 4)(7, 7, 7, 7)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None                 # noqa: E731

        def fwd(nv_=nv, nf_=nf, v_=dv, f_=df, outs=(d2, ix, w, diff), rep_=rep):
            return L.r3g_cloud_faces(ctx, ptr(v_), nv_, ptr(f_), nf_, *[ptr(o) for o in outs], rep_, ffi.stream_ptr())

        def bwd(nv_=nv, nf_=nf, bufs=(d2, ix, w, diff, cs, ci, gv)):
            return L.r3g_cloud_faces_backward(ctx, nv_, nf_, *[ptr(b) for b in bufs], ffi.stream_ptr())

        ms = (ctypes.c_double * 4)()
        assert fwd() == STATE and b"no cloud" in L.r3g_last_error()      # nothing built on this context yet
        assert L.r3g_cloud_faces_times(ctx, ms) == STATE
        assert fwd(nv_=-1) == INVALID and fwd(nf_=-1) == INVALID and fwd(nf_=2 ** 29 + 1) == INVALID and fwd(nv_=2 ** 31) == INVALID
        assert fwd(v_=None) == INVALID and fwd(f_=None) == INVALID and fwd(rep_=None) == INVALID
        for k in range(4):
            assert fwd(outs=tuple(None if j == k else o for j, o in enumerate((d2, ix, w, diff)))) == INVALID
        assert bwd(nv_=-1) == INVALID and bwd(nf_=-1) == INVALID and bwd(nf_=2 ** 29 + 1) == INVALID
        for k in range(7):
            assert bwd(bufs=tuple(None if j == k else o for j, o in enumerate((d2, ix, w, diff, cs, ci, gv)))) == INVALID
        assert bwd(nv_=0, bufs=(d2, ix, w, diff, None, ci, None)) == 0                          # nothing to do
        p = dev(R.edge_cloud(64))
        assert L.r3g_cloud_build(ctx, ptr(p), 64, 0, None, None, ffi.stream_ptr()) == 0
        assert fwd(nf_=0, f_=None, outs=(None,) * 4) == 0 and list(rep) == [0, 0, 0, 0]           # nothing to do, nothing launched
        assert L.r3g_cloud_faces_times(ctx, ms) == STATE
        assert fwd() == 0 and rep[0] == nf - 5
        assert L.r3g_cloud_faces_times(ctx, ms) == 0 and ms[3] == -1.0 and min(ms[:3]) >= 0
        assert bwd() == 0 and L.r3g_cloud_faces_times(ctx, ms) == 0 and ms[3] >= 0
        assert fwd(nv_=0, v_=None) == 0 and rep[0] == 0                                         # every index lies outside [0, 0)
        bad = torch.full((4, 3), float("nan"), device="cuda")
        assert L.r3g_cloud_build(ctx, ptr(bad), 4, 0, None, None, ffi.stream_ptr()) == INVALID  # a failed build: no cloud
        assert fwd() == STATE
    finally:
        L.r3g_destroy(ctx)
    with pytest.raises(ValueError):
        from r3g import cloud
        cloud.face_nearest(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32))          # CPU tensors: there is no CPU path
