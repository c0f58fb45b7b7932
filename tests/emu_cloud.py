"""ctypes loader for tests/emu/cloud_emu.cpp (host run of csrc/cloud_core.h; test-only)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "3d-re-gen_amd", "csrc")
_SRC = os.path.join(_HERE, "cloud_emu.cpp")
_DEPS = [_SRC] + [os.path.join(_CSRC, h) for h in ("cloud_core.h", "meshdist_core.h", "grid_csr.h")]
_LIB = None
_I64P = ctypes.POINTER(ctypes.c_int64)


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in _DEPS)


def _lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libr3g_cloud_emu.so")
        if _stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-I" + _CSRC, "-o", so, _SRC])
        lib = ctypes.CDLL(so)
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
    exe = os.path.join(_HERE, "cloud_selftest")
    if _stale(exe):
        flags = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-DCLOUD_EMU_MAIN", "-I" + _CSRC] + flags +
                              ["-o", exe, _SRC])
    return exe
