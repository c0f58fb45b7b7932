"""ctypes loader for tests/emu/orient_emu.cpp (host run of the product's orient core; test-only; built by tests/emu_build.py).  The (k + 1)-rows come from the
cloud twin (tests/emu_cloud.py), as the product takes them from r3g_cloud_knn."""
import ctypes

import numpy as np

import emu_build
import emu_cloud

_LIB = None
REPORT_FIELDS = ("usable", "trees", "flipped", "rounds", "frustrated")


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("orient"))
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
    return emu_build.program("orient", defines=("ORIENT_EMU_MAIN",), sanitize=sanitize)
