"""ctypes loader for tests/emu/cloud_emu.cpp (host run of the product's cloud core; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None
_I64P = ctypes.POINTER(ctypes.c_int64)


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("cloud"))
        lib.r3g_emu_cloud_brute.restype = ctypes.c_int
        lib.r3g_emu_cloud_brute.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p, _I64P]
        lib.r3g_emu_cloud_grid.restype = ctypes.c_int
        lib.r3g_emu_cloud_grid.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), _I64P, _I64P]
        lib.r3g_emu_cloud_auto_resolution.restype = ctypes.c_int
        lib.r3g_emu_cloud_auto_resolution.argtypes = [ctypes.c_int64, ctypes.c_int]
        _LIB = lib
    return _LIB


def _arrays(points, queries, k):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    return p, q, np.empty((len(q), k), np.float32), np.empty((len(q), k), np.int32)


def brute(queries, points, k=1):
    """(a): the k-list over every usable point -> (dist2 float32 [N,k], index int32 [N,k], skipped)"""
    p, q, d2, ix = _arrays(points, queries, k)
    sk = ctypes.c_int64(0)
    rc = _lib().r3g_emu_cloud_brute(p.ctypes.data, len(p), q.ctypes.data, len(q), int(k), d2.ctypes.data, ix.ctypes.data, ctypes.byref(sk))
    if rc:
        raise ValueError("cloud emu: error %d" % rc)
    return d2, ix, sk.value


def grid(queries, points, k=1, resolution=0, reverse_fill=False):
    """(b): the product's grid build and ring walk in host loops -> (dist2, index, info dict: resolution, skipped, tests)"""
    p, q, d2, ix = _arrays(points, queries, k)
    res, sk, tests = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = _lib().r3g_emu_cloud_grid(p.ctypes.data, len(p), int(resolution), int(bool(reverse_fill)), q.ctypes.data, len(q), int(k),
                                   d2.ctypes.data, ix.ctypes.data, ctypes.byref(res), ctypes.byref(sk), ctypes.byref(tests))
    if rc:
        raise ValueError("cloud emu: error %d" % rc)
    return d2, ix, {"resolution": res.value, "skipped": sk.value, "tests": tests.value}


def auto_resolution(n_usable, per_cell=0):
    """the automatic rule for P = per_cell points per cell (0: the product's own P)"""
    return int(_lib().r3g_emu_cloud_auto_resolution(int(n_usable), int(per_cell)))


def selftest_binary(sanitize=True):
    """the twin with its own main(), as a stand-alone program (host only; -fsanitize=address,undefined) -> path"""
    return emu_build.program("cloud", defines=("CLOUD_EMU_MAIN",), sanitize=sanitize)
