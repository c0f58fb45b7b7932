"""ctypes loader for tests/emu/meshfill_emu.cpp (host run of the product's meshfill core over the mate table of
tests/emu/meshtopo_emu.cpp; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None

REPORT_FIELDS = ("boundary", "loops", "tangled", "filled", "oversize", "longest", "loop_edges", "faces_added", "verts_added",
                 "rounds", "max_loop", "mode", "n_faces", "n_verts")
MODES = {"fan": 0, "centroid": 1}


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("meshfill"))
        lib.r3g_emu_meshfill_plan.restype = ctypes.c_int
        lib.r3g_emu_meshfill_plan.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.r3g_emu_meshfill_emit.restype = ctypes.c_int
        lib.r3g_emu_meshfill_emit.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.r3g_emu_meshfill_loops.restype = ctypes.c_int
        lib.r3g_emu_meshfill_loops.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _LIB = lib
    return _LIB


class EmuError(ValueError):
    def __init__(self, code):
        super().__init__("meshfill emu: error %d" % code)
        self.code = code


def report_dict(r):
    return {k: int(x) for k, x in zip(REPORT_FIELDS, r)}


def plan(verts, faces, max_loop=64, mode="fan", n_verts=None, reverse=False):
    """-> dict(report, loop_start int64 [loops + 1], loop_verts int32, status int32 [loops], new_faces int32 [faces_added, 3],
    new_verts float32 [verts_added, 3]); verts None: mode "fan" only (n_verts required)"""
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    v = None if verts is None else np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    nv = len(v) if v is not None else int(n_verts)
    rep = np.zeros(16, np.int64)
    lib = _lib()
    rc = lib.r3g_emu_meshfill_plan(None if v is None else v.ctypes.data, nv, f.ctypes.data, len(f), int(max_loop),
                                   MODES.get(mode, mode), int(bool(reverse)), rep.ctypes.data)
    if rc:
        raise EmuError(rc)
    r = report_dict(rep)
    out = {"report": r, "loop_start": np.zeros(r["loops"] + 1, np.int64), "loop_verts": np.zeros(r["loop_edges"], np.int32),
           "status": np.zeros(r["loops"], np.int32), "new_faces": np.zeros((r["faces_added"], 3), np.int32),
           "new_verts": np.zeros((r["verts_added"], 3), np.float32)}
    assert lib.r3g_emu_meshfill_loops(out["loop_start"].ctypes.data, out["loop_verts"].ctypes.data, out["status"].ctypes.data) == 0
    assert lib.r3g_emu_meshfill_emit(out["new_faces"].ctypes.data, out["new_verts"].ctypes.data) == 0
    return out


def fill_holes(verts, faces, max_loop=64, mode="fan", n_verts=None, reverse=False):
    """-> (verts float32 or None, faces int32, report): the input followed by what the plan adds"""
    p = plan(verts, faces, max_loop, mode, n_verts, reverse)
    f = np.concatenate([np.ascontiguousarray(faces, np.int32).reshape(-1, 3), p["new_faces"]])
    v = None if verts is None else np.concatenate([np.ascontiguousarray(verts, np.float32).reshape(-1, 3), p["new_verts"]])
    return v, f, p["report"]
