"""ctypes loader for tests/emu/plane_emu.cpp (host run of the product's plane core; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None
_I64P = ctypes.POINTER(ctypes.c_int64)
_DP = ctypes.POINTER(ctypes.c_double)
MUTANTS = {"less_equal": 1, "float32_distance": 2, "last_on_tie": 3, "skip_validity": 4}
REPORT = ("n_usable", "n_valid", "best", "best_count", "few")
MOMENTS_REPORT = ("n", "skipped", "few")


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("plane"))
        lib.r3g_emu_plane_ransac.restype = ctypes.c_int
        lib.r3g_emu_plane_ransac.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, _I64P, _DP]
        lib.r3g_emu_plane_moments.restype = ctypes.c_int
        lib.r3g_emu_plane_moments.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, _DP, _I64P]
        lib.r3g_emu_plane_count_points.restype = ctypes.c_int
        _LIB = lib
    return _LIB


def count_points():
    """rows a block of the count pass holds (the sizes around it are edge cases of the product)"""
    return int(_lib().r3g_emu_plane_count_points())


def _run(points, triples, threshold, mode, splits, mutant):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    n, h = len(p), len(t)
    count, mask = np.zeros(h, np.uint32), np.zeros(n, np.uint8)
    rep, plane = (ctypes.c_int64 * 8)(), (ctypes.c_double * 16)()
    rc = _lib().r3g_emu_plane_ransac(p.ctypes.data if n else None, n, t.ctypes.data if h else None, h, float(threshold), mode, splits, mutant,
                                     count.ctypes.data if h else None, mask.ctypes.data if n else None, rep, plane)
    if rc:
        raise ValueError("plane emu: error %d" % rc)
    return {"counts": count, "mask": mask, "report": dict(zip(REPORT, list(rep)[:5])), "plane": np.array(list(plane), np.float64)}


def brute(points, triples, threshold, mutant=None):
    """(a): two plain loops -> dict(counts uint32 [H], mask uint8 [n], report, plane float64 [16]).
    mutant: None or a key of MUTANTS (a deliberate departure from the definition)"""
    return _run(points, triples, threshold, 0, 1, MUTANTS[mutant] if mutant else 0)


def blocks(points, triples, threshold, splits=1):
    """(b): the count pass in the product's block order, the table split `splits` ways -> the same dict"""
    return _run(points, triples, threshold, 1, int(splits), 0)


def moments(points, mask=None):
    """-> dict(out float64 [16] as r3g_plane_moments has it, report)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    out, rep = (ctypes.c_double * 16)(), (ctypes.c_int64 * 4)()
    rc = _lib().r3g_emu_plane_moments(p.ctypes.data if n else None, n, m.ctypes.data if m is not None and n else None, out, rep)
    if rc:
        raise ValueError("plane emu: error %d" % rc)
    return {"out": np.array(list(out), np.float64), "report": dict(zip(MOMENTS_REPORT, list(rep)[:3]))}


def selftest_binary(sanitize=True):
    """the twin with its own main(), as a stand-alone program (host only; -fsanitize=address,undefined) -> path"""
    return emu_build.program("plane", defines=("PLANE_EMU_MAIN",), sanitize=sanitize)
