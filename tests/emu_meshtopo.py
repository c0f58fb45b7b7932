"""ctypes loader for tests/emu/meshtopo_emu.cpp (host run of the product's meshtopo core; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None
_I64P = ctypes.POINTER(ctypes.c_int64)

REPORT_FIELDS = ("usable", "skipped", "vref", "edges", "boundary", "clash", "nonmanifold", "bodies", "unorientable", "euler",
                 "nonfinite", "six_volume_q", "vol_scale", "two_area_q", "area_scale", "has_verts")


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("meshtopo"))
        lib.r3g_emu_meshtopo_build.restype = ctypes.c_int
        lib.r3g_emu_meshtopo_build.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.POINTER(ctypes.c_int)]
        lib.r3g_emu_meshtopo_orient.restype = ctypes.c_int
        lib.r3g_emu_meshtopo_orient.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                ctypes.c_int, _I64P, _I64P, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p]
        _LIB = lib
    return _LIB


class EmuError(ValueError):
    def __init__(self, code):
        super().__init__("meshtopo emu: error %d" % code)
        self.code = code


def _arrays(verts, faces, n_verts):
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).copy()
    v = None if verts is None else np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    nv = len(v) if v is not None else int(n_verts)
    return v, nv, f


def _out(nf):
    return np.empty((nf, 3), np.int32), np.empty(nf, np.int32), np.empty(nf, np.uint8), np.zeros(16, np.int64)


def report_dict(r):
    return {k: int(x) for k, x in zip(REPORT_FIELDS, r)}


def build(verts, faces, n_verts=None, reverse=False):
    """-> dict(mate [F,3], body [F], flip [F], report dict, rounds); verts None: topology only (n_verts required)"""
    v, nv, f = _arrays(verts, faces, n_verts)
    mate, body, flip, rep = _out(len(f))
    rounds = ctypes.c_int(0)
    rc = _lib().r3g_emu_meshtopo_build(None if v is None else v.ctypes.data, nv, f.ctypes.data, len(f), int(bool(reverse)),
                                       mate.ctypes.data, body.ctypes.data, flip.ctypes.data, rep.ctypes.data, ctypes.byref(rounds))
    if rc:
        raise EmuError(rc)
    return {"mate": mate, "body": body, "flip": flip, "report": report_dict(rep), "rounds": rounds.value}


def orient(verts, faces, outward, n_verts=None, reverse=False):
    """-> dict(faces: the rewritten copy, faces_reversed, bodies_reversed, and the state after: mate, body, flip, report)"""
    v, nv, f = _arrays(verts, faces, n_verts)
    mate, body, flip, rep = _out(len(f))
    nfr, nbr = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = _lib().r3g_emu_meshtopo_orient(None if v is None else v.ctypes.data, nv, f.ctypes.data, len(f), int(outward),
                                        int(bool(reverse)), ctypes.byref(nfr), ctypes.byref(nbr), mate.ctypes.data,
                                        body.ctypes.data, flip.ctypes.data, rep.ctypes.data)
    if rc:
        raise EmuError(rc)
    return {"faces": f, "faces_reversed": nfr.value, "bodies_reversed": nbr.value, "mate": mate, "body": body, "flip": flip,
            "report": report_dict(rep)}
