"""Texture-stage pixel kernels (csrc/tex_kernels.hip) at their edges: every case of tests/tex_edge_checks.py is launched once
through the C ABI into guard buffers (tests/row_guard.py), compared bit for bit with oracle/tex_ref.py (powf excepted, as in
tests/test_tex_gpu.py) AND with the independent ground truth of tests/tex_truth.py.  The same cases run on the CPU against
the oracle and its mutants in tests/test_tex_truth_cpu.py.  Every index array is in range; nothing here reads or writes
outside a buffer on purpose."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import row_guard as G  # noqa: E402
import tex_edge_checks as ec  # noqa: E402
import tex_support as ts  # noqa: E402
from oracle import tex_ref  # noqa: E402
from parity_support import report  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


class Kernels:
    """the oracle's functions on the GPU: numpy in, numpy out; outputs live in guard buffers whose guards are checked, and
    every result is compared with the oracle before it is handed to the truth"""

    def __init__(self):
        import torch
        from r3g import ffi
        self.torch, self.ffi, self.L, self.ctx = torch, ffi, ffi.lib(), ffi.context(0)

    # -- plumbing
    def dev(self, a, dtype):
        return self.torch.as_tensor(np.ascontiguousarray(np.asarray(a), dtype=dtype)).cuda()

    def out(self, nbytes, kind="f32"):
        """guarded flat buffer with `nbytes` owned bytes after G.OFF guard elements; -> (flat, owned index tensor)"""
        torch = self.torch
        dtype = torch.float32 if kind == "f32" else torch.uint8
        n = nbytes // 4 if kind == "f32" else nbytes
        flat = G.guarded(torch, dtype, G.OFF + n + 64)
        return flat, torch.arange(G.OFF, G.OFF + n, device="cuda")

    def launch(self, tag, call, outs):
        G.run(self.torch, self.ffi, call, tag)
        for flat, idx in outs:
            n, first = G.untouched(self.torch, flat, idx)
            assert n == 0, "%s: %d elements outside the output were written, the first at %d" % (tag, n, first - G.OFF)

    def read(self, flat, idx, dtype, shape):
        return flat[idx].cpu().numpy().view(dtype).reshape(shape).copy()

    def stream(self):
        return G.stream(self.torch)

    # -- the kernels
    def rasterize(self, pos, tri, H, W):
        tri = np.asarray(tri, np.int32).reshape(-1, 3)
        p, t = self.dev(pos, F32), self.dev(tri, np.int32)
        fi, fi_i = self.out(4 * H * W)
        ba, ba_i = self.out(12 * H * W)
        self.launch("rasterize %dx%d F %d" % (H, W, len(tri)),
                    lambda: self.L.r3g_tex_rasterize(self.ctx, G.ptr(p), p.shape[0], G.ptr(t) if len(tri) else None, len(tri), H, W,
                                                     G.ptr(fi, G.OFF), G.ptr(ba, G.OFF), self.stream()), [(fi, fi_i), (ba, ba_i)])
        got = self.read(fi, fi_i, np.int32, (H, W)), self.read(ba, ba_i, F32, (H, W, 3))
        with np.errstate(all="ignore"):
            ref = tex_ref.rasterize(pos, tri, H, W)
        assert np.array_equal(got[0], ref[0]), "face ids differ from the oracle at %d pixels" % (got[0] != ref[0]).sum()
        assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), "barycentrics differ from the oracle"
        return got

    def interpolate(self, attr, tri, fi, bary):
        C, npix = attr.shape[1], int(np.asarray(fi).size)
        a, t = self.dev(attr, F32), self.dev(tri, np.int32)
        f, b = self.dev(np.append(np.asarray(fi).reshape(-1), 0), np.int32), self.dev(np.append(np.asarray(bary).reshape(-1), 0), F32)   # never null
        o, o_i = self.out(4 * npix * C)
        self.launch("interpolate C %d npix %d" % (C, npix),
                    lambda: self.L.r3g_tex_interpolate(self.ctx, G.ptr(a), C, G.ptr(t), G.ptr(f), G.ptr(b), npix, G.ptr(o, G.OFF), self.stream()),
                    [(o, o_i)])
        got = self.read(o, o_i, F32, (npix, C))
        assert np.array_equal(got.view(np.uint32), tex_ref.interpolate(attr, tri, fi, bary).view(np.uint32)), "differs from the oracle"
        return got

    def view_weight(self, fi, depth, normal, thr, edge, vw, power):
        H, W = fi.shape
        f, d, n = self.dev(fi, np.int32), self.dev(depth, F32), self.dev(normal, F32)
        o, o_i = self.out(4 * H * W)
        self.launch("view_weight %dx%d" % (H, W),
                    lambda: self.L.r3g_tex_view_weight(self.ctx, G.ptr(f), G.ptr(d), G.ptr(n), H, W, float(thr), float(edge), float(vw), float(power),
                                                       G.ptr(o, G.OFF), self.stream()), [(o, o_i)])
        got = self.read(o, o_i, F32, (H, W))
        ref = tex_ref.view_weight(fi, depth, normal, thr, edge, vw, power)
        assert np.array_equal(~(got == 0), ~(ref == 0)), "kept pixels differ from the oracle"
        assert np.allclose(got, ref, rtol=2e-6, atol=0, equal_nan=True), "values differ from the oracle beyond powf's last bits"
        return got

    def _acc(self, T):
        a, a_i = self.out(32 * T * T)
        a[a_i] = 0.0                                   # the accumulator is read and written: zeroed, as the contract asks
        return a, a_i

    def bake(self, image, weight, fi, bary, uv, uv_tri, T):
        npix = int(np.asarray(fi).size)
        args = [self.dev(image, F32), self.dev(weight, F32), self.dev(fi, np.int32), self.dev(bary, F32), self.dev(uv, F32), self.dev(uv_tri, np.int32)]
        a, a_i = self._acc(T)
        self.launch("bake T %d npix %d" % (T, npix),
                    lambda: self.L.r3g_tex_bake(self.ctx, *[G.ptr(x) for x in args], npix, T, G.ptr(a, G.OFF), self.stream()), [(a, a_i)])
        got = self.read(a, a_i, np.uint64, (T, T, 4))
        with np.errstate(all="ignore"):
            ref = tex_ref.bake(image, weight, fi, bary, uv, uv_tri, T)
        assert np.array_equal(got, ref), "accumulators differ from the oracle"
        return got

    def bake_gather(self, fu, bu, clip_uv, uv_tri, image, weight, fi, depth, eps):
        T = fu.shape[0]
        H, W = fi.shape
        args = [self.dev(fu, np.int32), self.dev(bu, F32), self.dev(clip_uv, F32), self.dev(uv_tri, np.int32)]
        view = [self.dev(image, F32), self.dev(weight, F32), self.dev(fi, np.int32), self.dev(depth, F32)]
        a, a_i = self._acc(T)
        self.launch("bake_gather T %d view %dx%d" % (T, H, W),
                    lambda: self.L.r3g_tex_bake_gather(self.ctx, *[G.ptr(x) for x in args], T, *[G.ptr(x) for x in view], H, W, float(eps),
                                                       G.ptr(a, G.OFF), self.stream()), [(a, a_i)])
        got = self.read(a, a_i, np.uint64, (T, T, 4))
        with np.errstate(all="ignore"):
            ref = tex_ref.bake_gather(fu, bu, clip_uv, uv_tri, image, weight, fi, depth, eps)
        assert np.array_equal(got, ref), "accumulators differ from the oracle"
        return got

    def bake_finalize(self, acc):
        T = acc.shape[0]
        a = self.dev(acc.view(np.int64), np.int64)
        t, t_i = self.out(12 * T * T)
        m, m_i = self.out(T * T, "u8")
        self.launch("bake_finalize T %d" % T, lambda: self.L.r3g_tex_bake_finalize(self.ctx, G.ptr(a), T, G.ptr(t, G.OFF), G.ptr(m, G.OFF), self.stream()),
                    [(t, t_i), (m, m_i)])
        got = self.read(t, t_i, F32, (T, T, 3)), self.read(m, m_i, np.uint8, (T, T))
        ref = tex_ref.bake_finalize(acc)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1], ref[1]), "differs from the oracle"
        return got

    def inpaint(self, tex, mask, fu, bu, verts, pos_tri, uv, uv_tri, dilate_iters):
        T = mask.shape[0]
        t, t_i = self.out(12 * T * T)
        m, m_i = self.out(T * T, "u8")
        t[t_i] = self.dev(tex, F32).reshape(-1)
        m[m_i] = self.dev(mask, np.uint8).reshape(-1)
        args = [self.dev(fu, np.int32), self.dev(bu, F32), self.dev(verts, F32)]
        rest = [self.dev(pos_tri, np.int32), self.dev(uv, F32), self.dev(uv_tri, np.int32)]
        rounds = ctypes.c_int(-1)
        self.launch("inpaint T %d dilate %d" % (T, dilate_iters),
                    lambda: self.L.r3g_tex_inpaint(self.ctx, G.ptr(t, G.OFF), G.ptr(m, G.OFF), T, G.ptr(args[0]), G.ptr(args[1]), G.ptr(args[2]),
                                                   len(verts), G.ptr(rest[0]), G.ptr(rest[1]), G.ptr(rest[2]), len(pos_tri), int(dilate_iters),
                                                   ctypes.byref(rounds), self.stream()), [(t, t_i), (m, m_i)])
        got = self.read(t, t_i, F32, (T, T, 3)), self.read(m, m_i, np.uint8, (T, T)), rounds.value
        ref = tex_ref.inpaint(tex, mask, fu, bu, verts, pos_tri, uv, uv_tri, dilate_iters)
        assert got[2] == ref[2], "%d rounds, the oracle %d" % (got[2], ref[2])
        assert np.array_equal(got[1], ref[1]), "mask differs from the oracle"
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), "texture differs from the oracle"
        return got


@pytest.fixture(scope="module")
def k():
    return Kernels()


def _ok(result, label):
    fails, m = result
    print(label, m)
    assert not fails, label + ":\n" + "\n".join(fails)
    return m


@pytest.mark.parametrize("name", list(ts.raster_edge_scenes_cached()))
def test_rasterize(k, name):
    m = _ok(ec.check_raster_scene(k, name), name)
    if ec.raster_truth(name)[4] == "closed":
        assert m["holes"] == 0
    for key in ("depth_ratio", "bary_ratio"):
        _note("rasterize " + key, m.get(key, 0.0))
    if name == "F = 1":
        report("tex edges: rasterize, depth excess / bound", WORST.get("rasterize depth_ratio", 0.0), 1.0)
        report("tex edges: rasterize, barycentric error / bound", WORST.get("rasterize bary_ratio", 0.0), 1.0)


@pytest.mark.parametrize("C,npix", ec.INTERP_CASES)
def test_interpolate(k, C, npix):
    m = _ok(ec.check_interpolate(k, C, npix), "interpolate C %d npix %d" % (C, npix))
    _note("interpolate", m["ratio"])
    if (C, npix) == ec.INTERP_CASES[-1]:
        report("tex edges: interpolate, error / bound", WORST.get("interpolate", 0.0), 1.0)


@pytest.mark.parametrize("name", list(ec.view_weight_cases()))
def test_view_weight(k, name):
    _ok(ec.check_view_weight(k, name), name)


@pytest.mark.parametrize("T", ec.BAKE_T)
def test_bake(k, T):
    _ok(ec.check_bake(k, T), "bake T %d" % T)


def test_bake_4096_pixels_into_one_texel(k):
    _ok(ec.check_bake_many(k), "bake 4096 into one")


@pytest.mark.parametrize("name", list(ec.gather_cases()))
def test_bake_gather(k, name):
    _ok(ec.check_gather(k, name), name)


def test_bake_finalize(k):
    m = _ok(ec.check_finalize(k), "finalize")
    report("tex edges: finalize, ulps from the correctly rounded quotient", m["ulps"], 1.0)


@pytest.mark.parametrize("name", list(ec.inpaint_cases()))
def test_inpaint(k, name):
    _ok(ec.check_inpaint(k, name), name)


def test_zero_pixel_calls_return_ok(k):
    """an empty image: R3G_OK and no launch, with the null buffers an empty tensor brings, and nothing written"""
    import torch
    from r3g import texops
    attr = torch.zeros((4, 3), device="cuda")
    tri = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    out = texops.interpolate(attr, tri, torch.zeros((0, 5), dtype=torch.int32, device="cuda"), torch.zeros((0, 5, 3), device="cuda"))
    assert tuple(out.shape) == (0, 5, 3)
    acc = texops.new_accumulator(4, "cuda")
    texops.bake(torch.zeros((0, 5, 3), device="cuda"), torch.zeros((0, 5), device="cuda"), torch.zeros((0, 5), dtype=torch.int32, device="cuda"),
                torch.zeros((0, 5, 3), device="cuda"), torch.zeros((3, 2), device="cuda"), tri, acc)
    torch.cuda.synchronize()
    assert int(acc.abs().sum()) == 0
    a, a_i = k._acc(2)
    img, w, uv, uv_tri, fi, bary = ec.bake_case(2)
    dev = [k.dev(img, F32), k.dev(w, F32), k.dev(fi, np.int32), k.dev(bary, F32), k.dev(uv, F32), k.dev(uv_tri, np.int32)]
    k.launch("bake npix 0", lambda: k.L.r3g_tex_bake(k.ctx, *[G.ptr(x) for x in dev], 0, 2, G.ptr(a, G.OFF), k.stream()), [(a, a_i)])
    assert int(k.read(a, a_i, np.uint64, (2, 2, 4)).sum()) == 0
