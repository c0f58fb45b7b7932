"""ctypes loader for tests/emu/dmc_emu.cpp (host emulation of the HIP dual-marching-cubes launch structure; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("dmc"))
        lib.r3g_emu_dmc.restype = ctypes.c_int
        lib.r3g_emu_dmc.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                    ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                    ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                    ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_int64)]
        lib.r3g_emu_dmc_free.argtypes = [ctypes.c_void_p]
        _LIB = lib
    return _LIB


def dual_marching_cubes(vol, level, manifold=True, xform=None, reversed_faces=False):
    """-> (verts, faces, flags, n_flipped).  xform = (grid_size[3], bbox_size[3], bbox_min[3]) or None.
    flags: 1 some sample <= level, 2 some sample >= level, 4 some sample NaN (the C ABI's range test)."""
    vol = np.ascontiguousarray(vol, np.float32)
    pv, pf = ctypes.c_void_p(), ctypes.c_void_p()
    nv, nf, fl, nfl = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint(), ctypes.c_int64()
    xf = None
    if xform is not None:
        xf = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64).reshape(3) for a in xform]))
    rc = _lib().r3g_emu_dmc(vol.ctypes.data, *vol.shape, float(level), int(manifold),
                            xf.ctypes.data if xf is not None else None, int(reversed_faces),
                            ctypes.byref(pv), ctypes.byref(pf), ctypes.byref(nv), ctypes.byref(nf), ctypes.byref(fl),
                            ctypes.byref(nfl))
    assert rc == 0, rc
    v = np.ctypeslib.as_array(ctypes.cast(pv, ctypes.POINTER(ctypes.c_float)), (max(nv.value, 1), 3))[:nv.value].copy()
    f = np.ctypeslib.as_array(ctypes.cast(pf, ctypes.POINTER(ctypes.c_int32)), (max(nf.value, 1), 3))[:nf.value].copy()
    _lib().r3g_emu_dmc_free(pv)
    _lib().r3g_emu_dmc_free(pf)
    return v, f, fl.value, nfl.value
