"""ctypes loader for tests/emu/meshinside_emu.cpp (host run of the product's meshinside core; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None
_I64P = ctypes.POINTER(ctypes.c_int64)


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("meshinside"))
        lib.r3g_emu_meshinside_brute.restype = ctypes.c_int
        lib.r3g_emu_meshinside_brute.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _I64P]
        lib.r3g_emu_meshinside_grid.restype = ctypes.c_int
        lib.r3g_emu_meshinside_grid.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                ctypes.POINTER(ctypes.c_int), _I64P, _I64P, _I64P]
        _LIB = lib
    return _LIB


def _arrays(verts, faces, points):
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    return v, f, p, np.empty(len(p), np.int32)


def brute(points, verts, faces, axis=2):
    """(a): the sum of the product's `crossed` over every usable face -> (count int32 [N], skipped)"""
    v, f, p, cnt = _arrays(verts, faces, points)
    sk = ctypes.c_int64(0)
    rc = _lib().r3g_emu_meshinside_brute(v.ctypes.data, len(v), f.ctypes.data, len(f), int(axis), p.ctypes.data, len(p),
                                         cnt.ctypes.data, ctypes.byref(sk))
    if rc:
        raise ValueError("meshinside emu: error %d" % rc)
    return cnt, sk.value


def grid(points, verts, faces, axis=2, resolution=0, reverse_fill=False):
    """(b): the product's column build and query in host loops -> (count, info dict: resolution, pairs, skipped, tests)"""
    v, f, p, cnt = _arrays(verts, faces, points)
    res, pairs, sk, tests = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = _lib().r3g_emu_meshinside_grid(v.ctypes.data, len(v), f.ctypes.data, len(f), int(axis), int(resolution),
                                        int(bool(reverse_fill)), p.ctypes.data, len(p), cnt.ctypes.data, ctypes.byref(res),
                                        ctypes.byref(pairs), ctypes.byref(sk), ctypes.byref(tests))
    if rc:
        raise ValueError("meshinside emu: error %d" % rc)
    return cnt, {"resolution": res.value, "pairs": pairs.value, "skipped": sk.value, "tests": tests.value}


def contains(points, verts, faces, axes=(2,)):
    """parity on one axis, or the majority of three -> inside bool [N], or (inside, share of points where all three agree)"""
    par = [(lambda c: (c > 0) & (c % 2 == 1))(brute(points, verts, faces, a)[0]) for a in axes]
    if len(par) == 1:
        return par[0]
    votes = np.sum(par, axis=0)
    agree = (votes == 0) | (votes == len(par))
    return votes * 2 > len(par), float(agree.mean()) if len(agree) else 1.0
