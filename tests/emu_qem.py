"""ctypes loader for tests/emu/qem_emu.cpp (host run of the product's edge-collapse bodies; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("qem"))
        lib.r3g_emu_qem.restype = ctypes.c_int
        lib.r3g_emu_qem.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p,
                                    ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.POINTER(ctypes.c_int)]
        _LIB = lib
    return _LIB


def reduce_faces(verts, faces, max_faces):
    """-> (verts float32 [V,3], faces int32 [F,3], rounds)"""
    v = np.ascontiguousarray(verts, np.float32).copy()
    f = np.ascontiguousarray(faces, np.int32).copy()
    nv, nf, rounds = ctypes.c_int64(len(v)), ctypes.c_int64(len(f)), ctypes.c_int(0)
    rc = _lib().r3g_emu_qem(v.ctypes.data, ctypes.byref(nv), f.ctypes.data, ctypes.byref(nf), int(max_faces),
                            ctypes.byref(rounds))
    assert rc == 0
    return v[:nv.value].copy(), f[:nf.value].copy(), rounds.value
