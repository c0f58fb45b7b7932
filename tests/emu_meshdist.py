"""ctypes loader for tests/emu/meshdist_emu.cpp (host run of the product's meshdist core; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None
_I64P = ctypes.POINTER(ctypes.c_int64)


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("meshdist"))
        lib.r3g_emu_tri_dist2.restype = ctypes.c_float
        lib.r3g_emu_tri_dist2.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.r3g_emu_meshdist_brute.restype = ctypes.c_int
        lib.r3g_emu_meshdist_brute.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, _I64P]
        lib.r3g_emu_meshdist_grid.restype = ctypes.c_int
        lib.r3g_emu_meshdist_grid.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.POINTER(ctypes.c_int), _I64P, _I64P, _I64P]
        _LIB = lib
    return _LIB


def _arrays(verts, faces, points):
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    return v, f, p, np.empty(len(p), np.float32), np.empty(len(p), np.int32)


def tri_dist2(p, abc):
    p = np.ascontiguousarray(p, np.float32)
    abc = np.ascontiguousarray(abc, np.float32)
    return float(_lib().r3g_emu_tri_dist2(p.ctypes.data, abc.ctypes.data))


def brute(points, verts, faces):
    """(a): min over every face of the product's float32 tri_dist2 -> (dist2 float32 [N], face int32 [N], skipped)"""
    v, f, p, d2, fc = _arrays(verts, faces, points)
    sk = ctypes.c_int64(0)
    rc = _lib().r3g_emu_meshdist_brute(v.ctypes.data, len(v), f.ctypes.data, len(f), p.ctypes.data, len(p), d2.ctypes.data,
                                       fc.ctypes.data, ctypes.byref(sk))
    if rc:
        raise ValueError("meshdist emu: error %d" % rc)
    return d2, fc, sk.value


def grid(points, verts, faces, resolution=0, reverse_fill=False):
    """(b): the product's grid build and ring walk in host loops
    -> (dist2, face, info dict: resolution, pairs, skipped, tests)"""
    v, f, p, d2, fc = _arrays(verts, faces, points)
    res, pairs, sk, tests = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = _lib().r3g_emu_meshdist_grid(v.ctypes.data, len(v), f.ctypes.data, len(f), int(resolution), int(bool(reverse_fill)),
                                      p.ctypes.data, len(p), d2.ctypes.data, fc.ctypes.data, ctypes.byref(res),
                                      ctypes.byref(pairs), ctypes.byref(sk), ctypes.byref(tests))
    if rc:
        raise ValueError("meshdist emu: error %d" % rc)
    return d2, fc, {"resolution": res.value, "pairs": pairs.value, "skipped": sk.value, "tests": tests.value}
