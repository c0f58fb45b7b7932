"""ctypes loader for tests/emu/orient_emu.cpp (host run of csrc/orient_core.h; test-only).  The (k + 1)-rows come from the
cloud twin (tests/emu_cloud.py), as the product takes them from r3g_cloud_knn."""
import ctypes
import os
import subprocess

import numpy as np

import emu_cloud

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "3d-re-gen_amd", "csrc")
_SRC = os.path.join(_HERE, "orient_emu.cpp")
_DEPS = [_SRC] + [os.path.join(_CSRC, h) for h in ("orient_core.h", "recon_core.h")]
_LIB = None
REPORT_FIELDS = ("usable", "trees", "flipped", "rounds", "frustrated")


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in _DEPS)


def _lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libr3g_orient_emu.so")
        if _stale(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-I" + _CSRC, "-o", so, _SRC])
        lib = ctypes.CDLL(so)
        lib.r3g_emu_orient.restype = ctypes.c_int
        lib.r3g_emu_orient.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _LIB = lib
    return _LIB


def usable(points, normals):
    p, n = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    return np.isfinite(p).all(1) & np.isfinite(n).all(1) & (n != 0).any(1)


def rows(points, normals, k):
    """the (k + 1)-list of the usable points against themselves by the cloud twin's brute force -> int32 [N, k + 1]"""
    p = np.array(points, np.float32).reshape(-1, 3)
    ok = usable(p, normals)
    p[~ok] = np.nan
    if not ok.any():
        return np.full((len(p), k + 1), -1, np.int32)
    return emu_cloud.brute(p, p, k + 1)[1]


def orient(points, normals, k, reverse=False):
    """-> (sign int8 [N], tree int32 [N], report dict)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    r = np.ascontiguousarray(rows(p, nr, k), np.int32)
    sign, tree, rep = np.empty(len(p), np.int8), np.empty(len(p), np.int32), np.zeros(8, np.int64)
    rc = _lib().r3g_emu_orient(p.ctypes.data, nr.ctypes.data, len(p), int(k), r.ctypes.data, int(reverse), sign.ctypes.data, tree.ctypes.data,
                               rep.ctypes.data)
    if rc:
        raise ValueError("orient emu: error %d" % rc)
    return sign, tree, {f: int(v) for f, v in zip(REPORT_FIELDS, rep)}


def selftest_binary(sanitize=True):
    """the twin with its own main(), as a stand-alone program (host only; -fsanitize=address,undefined) -> path"""
    exe = os.path.join(_HERE, "orient_selftest")
    if _stale(exe):
        flags = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-DORIENT_EMU_MAIN", "-I" + _CSRC] + flags +
                              ["-o", exe, _SRC])
    return exe
