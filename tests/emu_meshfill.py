"""ctypes loader for tests/emu/meshfill_emu.cpp (host run of csrc/meshfill_core.h over the mate table of
tests/emu/meshtopo_emu.cpp; test-only)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB = None

REPORT_FIELDS = ("boundary", "loops", "tangled", "filled", "oversize", "longest", "loop_edges", "faces_added", "verts_added",
                 "rounds", "max_loop", "mode", "n_faces", "n_verts")
MODES = {"fan": 0, "centroid": 1}


def _lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libr3g_meshfill_emu.so")
        srcs = [os.path.join(_HERE, "meshfill_emu.cpp"), os.path.join(_HERE, "meshtopo_emu.cpp")]
        csrc = os.path.join(_ROOT, "3d-re-gen_amd", "csrc")
        deps = srcs + [os.path.join(csrc, "meshfill_core.h"), os.path.join(csrc, "meshtopo_core.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-w",
                                   "-I" + csrc, "-o", so] + srcs)
        lib = ctypes.CDLL(so)
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
