"""ctypes loader for tests/emu/softras_emu.cpp (host run of the product's softras core; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None
_I64P = ctypes.POINTER(ctypes.c_int64)
_P, _I, _F, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
MUTANTS = {"blur_less_equal": 1, "no_face_key": 2, "unclipped_depth": 3, "narrow_box": 4, "ignore_endpoint": 5, "divide_out": 6}
REPORT = ("pairs", "used", "skipped", "tiles")
BACK_REPORT = ("found",)


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("softras"))
        lib.r3g_emu_softras_forward.restype = _I
        lib.r3g_emu_softras_forward.argtypes = [_P, _L, _P, _L, _I, _I, _I, _F, _F, _I, _P, _P, _P, _P, _I64P]
        lib.r3g_emu_softras_backward.restype = _I
        lib.r3g_emu_softras_backward.argtypes = [_P, _L, _P, _L, _I, _I, _I, _F, _F, _I, _P, _P, _P, _P, _P, _P, _P, _I64P]
        lib.r3g_emu_softras_sigmoid.restype = None
        lib.r3g_emu_softras_sigmoid.argtypes = [_P, _L, _P]
        _LIB = lib
    return _LIB


def _ptr(a):
    return a.ctypes.data if a.size else None


def sigmoid(x):
    """sr_sigmoid over a float32 array"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    _lib().r3g_emu_softras_sigmoid(_ptr(x), x.size, _ptr(out))
    return out


def corner_csr(tri, n_verts):
    """numpy restatement of r3g.softras.corner_csr: (start int32 [V + 1], ids int32 [valid corners]), corners ascending per vertex"""
    flat = np.ascontiguousarray(tri, np.int64).reshape(-1)
    ok = (flat >= 0) & (flat < n_verts)
    ids = np.argsort(np.where(ok, flat, n_verts), kind="stable")[:int(ok.sum())]
    start = np.zeros(n_verts + 1, np.int64)
    np.cumsum(np.bincount(flat[ok], minlength=n_verts), out=start[1:])
    return start.astype(np.int32), ids.astype(np.int32)


def forward(pos, tri, size, K, sigma, blur_radius, mutant=None):
    """-> dict(alpha [H][W], face, dist, zbuf [H][W][K], report)"""
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    H, W = size
    alpha = np.zeros((H, W), np.float32)
    face = np.zeros((H, W, K), np.int32)
    dist, zbuf = np.zeros((H, W, K), np.float32), np.zeros((H, W, K), np.float32)
    rep = (ctypes.c_int64 * 8)()
    rc = _lib().r3g_emu_softras_forward(_ptr(p), len(p), _ptr(t), len(t), H, W, K, float(np.float32(sigma)), float(np.float32(blur_radius)),
                                        MUTANTS[mutant] if mutant else 0, _ptr(alpha), _ptr(face), _ptr(dist), _ptr(zbuf), rep)
    if rc:
        raise ValueError("softras emu: error %d" % rc)
    return {"alpha": alpha, "face": face, "dist": dist, "zbuf": zbuf, "report": dict(zip(REPORT, list(rep)[:4]))}


def backward(pos, tri, size, K, sigma, blur_radius, face, dist, grad_alpha, mutant=None):
    """-> dict(grad_face [F][3][2], grad_pos [V][3], report)"""
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    H, W = size
    face = np.ascontiguousarray(face, np.int32)
    dist = np.ascontiguousarray(dist, np.float32)
    ga = np.ascontiguousarray(grad_alpha, np.float32)
    assert face.shape == (H, W, K) and dist.shape == (H, W, K) and ga.shape == (H, W)
    cs, ci = corner_csr(t, len(p))
    gf, gp = np.zeros((len(t), 3, 2), np.float32), np.zeros((len(p), 3), np.float32)
    rep = (ctypes.c_int64 * 4)()
    rc = _lib().r3g_emu_softras_backward(_ptr(p), len(p), _ptr(t), len(t), H, W, K, float(np.float32(sigma)), float(np.float32(blur_radius)),
                                         MUTANTS[mutant] if mutant else 0, _ptr(face), _ptr(dist), _ptr(ga), _ptr(cs), _ptr(ci), _ptr(gf), _ptr(gp), rep)
    if rc:
        raise ValueError("softras emu: error %d" % rc)
    return {"grad_face": gf, "grad_pos": gp, "report": dict(zip(BACK_REPORT, list(rep)[:1]))}


def selftest_binary(sanitize=True):
    """the twin with its own main(), as a stand-alone program (host only; -fsanitize=address,undefined) -> path"""
    return emu_build.program("softras", defines=("SOFTRAS_EMU_MAIN",), sanitize=sanitize)
