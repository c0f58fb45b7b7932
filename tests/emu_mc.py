"""ctypes loader for tests/emu/mc_emu.cpp (host emulation of the HIP launch structure; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("mc"))
        lib.r3g_emu_mc.restype = ctypes.c_int
        lib.r3g_emu_mc.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                   ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                   ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_uint)]
        lib.r3g_emu_free.argtypes = [ctypes.c_void_p]
        _LIB = lib
    return _LIB


def marching_cubes(vol, level, classic=False, xform=None, reversed_faces=True):
    """-> (verts, faces, flags).  xform = (grid_size[3], bbox_size[3], bbox_min[3]) or None."""
    vol = np.ascontiguousarray(vol, np.float32)
    pv, pf = ctypes.c_void_p(), ctypes.c_void_p()
    nv, nf, fl = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint()
    xf = None
    if xform is not None:
        xf = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64) for a in xform]))
    rc = _lib().r3g_emu_mc(vol.ctypes.data, *vol.shape, float(level), int(classic),
                           xf.ctypes.data if xf is not None else None, int(reversed_faces),
                           ctypes.byref(pv), ctypes.byref(pf), ctypes.byref(nv), ctypes.byref(nf), ctypes.byref(fl))
    assert rc == 0, rc
    v = np.ctypeslib.as_array(ctypes.cast(pv, ctypes.POINTER(ctypes.c_float)), (max(nv.value, 1), 3))[:nv.value].copy()
    f = np.ctypeslib.as_array(ctypes.cast(pf, ctypes.POINTER(ctypes.c_int32)), (max(nf.value, 1), 3))[:nf.value].copy()
    _lib().r3g_emu_free(pv)
    _lib().r3g_emu_free(pf)
    return v, f, fl.value
