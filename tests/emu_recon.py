"""ctypes loader for tests/emu/recon_emu.cpp (host run of the product's recon core; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None
_P = ctypes.c_void_p
_I64 = ctypes.c_int64
FIXED = 2.0 ** 30


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("recon"))
        lib.r3g_emu_recon_splat.restype = _I64
        lib.r3g_emu_recon_splat.argtypes = [_P, _P, _I64, ctypes.c_int, _P, ctypes.c_double, ctypes.c_int, _P]
        lib.r3g_emu_recon_rhs.restype = ctypes.c_int
        lib.r3g_emu_recon_rhs.argtypes = [_P, ctypes.c_int, _P, ctypes.c_double, _P]
        lib.r3g_emu_recon_vcycles.restype = ctypes.c_int
        lib.r3g_emu_recon_vcycles.argtypes = [_P, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, _P]
        lib.r3g_emu_recon_sample.restype = _I64
        lib.r3g_emu_recon_sample.argtypes = [ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_double, _P, _P, _I64, ctypes.c_int, _P,
                                             ctypes.POINTER(_I64)]
        _LIB = lib
    return _LIB


def _f3(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _centre(c):
    return np.ascontiguousarray(c, np.float64).reshape(3)


def nodes(depth):
    return 2 ** depth + 1


def splat(points, normals, depth, centre, side, reverse=False):
    """-> (channels int64 [4, n, n, n], usable)"""
    p, nr, c = _f3(points), _f3(normals), _centre(centre)
    n = nodes(depth)
    ch = np.empty((4, n, n, n), np.int64)
    used = _lib().r3g_emu_recon_splat(p.ctypes.data, nr.ctypes.data, len(p), int(depth), c.ctypes.data, float(side), int(reverse), ch.ctypes.data)
    if used < 0:
        raise ValueError("recon emu: refused")
    return ch, int(used)


def rhs(channels, depth, centre, side):
    """-> b float32 [n, n, n]"""
    ch, c = np.ascontiguousarray(channels, np.int64), _centre(centre)
    n = nodes(depth)
    b = np.empty((n, n, n), np.float32)
    assert _lib().r3g_emu_recon_rhs(ch.ctypes.data, int(depth), c.ctypes.data, float(side), b.ctypes.data) == 0
    return b


def vcycles(b, depth, side, cycles=10, mutant=0):
    """-> chi float32 [n, n, n] after `cycles` V-cycles from 0"""
    b = np.ascontiguousarray(b, np.float32)
    n = nodes(depth)
    assert b.shape == (n, n, n)
    chi = np.empty((n, n, n), np.float32)
    assert _lib().r3g_emu_recon_vcycles(b.ctypes.data, int(depth), float(side), int(cycles), int(mutant), chi.ctypes.data) == 0
    return chi


def sample(field, depth, centre, side, points, normals=None, reverse=False):
    """field: int64 [n, n, n] (the density channel) or float32 [n, n, n] -> (values float32 [N], fixed-point sum, count)"""
    field = np.ascontiguousarray(field)
    assert field.dtype in (np.int64, np.float32) and field.shape == (nodes(depth),) * 3
    p, c = _f3(points), _centre(centre)
    nr = _f3(normals) if normals is not None else None
    v = np.empty(len(p), np.float32)
    s = _I64(0)
    cnt = _lib().r3g_emu_recon_sample(0 if field.dtype == np.int64 else 1, field.ctypes.data, int(depth), c.ctypes.data, float(side),
                                      p.ctypes.data, nr.ctypes.data if nr is not None else None, len(p), int(reverse), v.ctypes.data,
                                      ctypes.byref(s))
    if cnt < 0:
        raise ValueError("recon emu: refused")
    return v, int(s.value), int(cnt)


def selftest_binary(sanitize=True):
    """the twin with its own main(), as a stand-alone program (host only; -fsanitize=address,undefined) -> path"""
    return emu_build.program("recon", defines=("RECON_EMU_MAIN",), sanitize=sanitize)
