"""ctypes loader for tests/emu/dbscan_emu.cpp (host run of the product's dbscan core; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None
_I64P = ctypes.POINTER(ctypes.c_int64)
MUTANTS = {"strict_less": 1, "float32_d2": 2, "not_itself": 3, "border_max": 4, "first_appearance": 5}
REPORT = ("n_usable", "n_core", "n_border", "n_noise", "n_clusters", "largest", "largest_size")


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("dbscan"))
        lib.r3g_emu_dbscan.restype = ctypes.c_int
        lib.r3g_emu_dbscan.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double] + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 3 + [_I64P, _I64P]
        lib.r3g_emu_dbscan_auto_resolution.restype = ctypes.c_int
        lib.r3g_emu_dbscan_auto_resolution.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int64]
        _LIB = lib
    return _LIB


def _run(points, eps, min_samples, grid, resolution, reverse_fill, early, mutant):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    label, count, core = np.empty(n, np.int32), np.empty(n, np.uint32), np.empty(n, np.uint8)
    rep, tests = (ctypes.c_int64 * 8)(), ctypes.c_int64(0)
    rc = _lib().r3g_emu_dbscan(p.ctypes.data, n, float(eps), int(min_samples), int(grid), int(resolution), int(bool(reverse_fill)),
                               int(bool(early)), int(mutant), label.ctypes.data, count.ctypes.data, core.ctypes.data, rep, ctypes.byref(tests))
    if rc:
        raise ValueError("dbscan emu: error %d" % rc)
    report = dict(zip(REPORT, list(rep)[:7]))
    return {"labels": label, "counts": count, "core": core.astype(bool), "report": report, "resolution": rep[7], "tests": tests.value}


def brute(points, eps, min_samples, early=False, mutant=None):
    """(a): all pairs of usable points -> dict(labels int32 [n], counts uint32 [n], core bool [n], report, tests).
    mutant: None or a key of MUTANTS (a deliberate departure from the definition)"""
    return _run(points, eps, min_samples, 0, 0, False, early, MUTANTS[mutant] if mutant else 0)


def grid(points, eps, min_samples, resolution=0, reverse_fill=False, early=False):
    """(b): the product's grid build and radius walk in host loops -> the same dict, with the resolution used"""
    return _run(points, eps, min_samples, 1, resolution, reverse_fill, early, 0)


def auto_resolution(lo, hi, eps, n_usable):
    lo, hi = np.ascontiguousarray(lo, np.float32), np.ascontiguousarray(hi, np.float32)
    return int(_lib().r3g_emu_dbscan_auto_resolution(lo.ctypes.data, hi.ctypes.data, float(eps), int(n_usable)))


def selftest_binary(sanitize=True):
    """the twin with its own main(), as a stand-alone program (host only; -fsanitize=address,undefined) -> path"""
    return emu_build.program("dbscan", defines=("DBSCAN_EMU_MAIN",), sanitize=sanitize)
