"""ctypes loader for tests/emu/meshfit_emu.cpp (host run of the product's meshdist and meshfit cores; test-only; built by tests/emu_build.py)."""
import ctypes

import numpy as np

import emu_build

_LIB = None
_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_int64
_D = ctypes.c_double

POINT, PLANE = 0, 1
TERMS = {POINT: 18, PLANE: 37}
IDENTITY = np.array([1.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(emu_build.shared("meshfit"))
        lib.r3g_emu_mf_tri_closest.restype = None
        lib.r3g_emu_mf_tri_closest.argtypes = [_P, _P, _L, _P, _P, _P]
        lib.r3g_emu_mf_closest.restype = _I
        lib.r3g_emu_mf_closest.argtypes = [_P, _L, _P, _L, _I, _P, _L, _P, _P, _P]
        lib.r3g_emu_mf_step.restype = _I
        lib.r3g_emu_mf_step.argtypes = [_P, _L, _P, _L, _I, _P, _L, _P, _P, _I, _D, _P, ctypes.POINTER(_L), _P]
        lib.r3g_emu_mf_fit.restype = _I
        lib.r3g_emu_mf_fit.argtypes = [_P, _L, _P, _L, _P, _L, _P, _P, _I, _I, _I, _D, _D, _P, _P]
        lib.r3g_emu_mf_solve.restype = _I
        lib.r3g_emu_mf_solve.argtypes = [_P, _I, _I, _P, _P, ctypes.POINTER(_I)]
        lib.r3g_emu_mf_compose.restype = None
        lib.r3g_emu_mf_compose.argtypes = [_P, _P, _P]
        _LIB = lib
    return _LIB


def _mesh(verts, faces):
    return (np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3))


def _weights(w, n):
    if w is None:
        return None, None
    w = np.ascontiguousarray(w, np.float32).reshape(-1)
    assert len(w) == n
    return w, w.ctypes.data


def tri_closest(points, tris):
    """points [N,3] against triangles [N,3,3], one each -> (dist2 of tri_dist2, dist2 of tri_closest, closest [N,3])"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    assert len(p) == len(t)
    a, b, q = np.empty(len(p), np.float32), np.empty(len(p), np.float32), np.empty((len(p), 3), np.float32)
    _lib().r3g_emu_mf_tri_closest(p.ctypes.data, t.ctypes.data, len(p), a.ctypes.data, b.ctypes.data, q.ctypes.data)
    return a, b, q


def closest(points, verts, faces, resolution=0):
    """-> (dist2 float32 [N], face int32 [N], closest float32 [N,3])"""
    v, f = _mesh(verts, faces)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    d2, fc, q = np.empty(len(p), np.float32), np.empty(len(p), np.int32), np.empty((len(p), 3), np.float32)
    rc = _lib().r3g_emu_mf_closest(v.ctypes.data, len(v), f.ctypes.data, len(f), int(resolution), p.ctypes.data, len(p),
                                   d2.ctypes.data, fc.ctypes.data, q.ctypes.data)
    if rc:
        raise ValueError("meshfit emu: error %d" % rc)
    return d2, fc, q


def step(points, verts, faces, mode, xform=None, weights=None, max_dist=float("inf"), resolution=0):
    """one accumulation -> (sums float64 [18 | 37], used, centre float64 [3])"""
    v, f = _mesh(verts, faces)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    w, wp = _weights(weights, len(p))
    x = np.ascontiguousarray(IDENTITY if xform is None else xform, np.float64)
    assert x.shape == (13,)
    sums, centre, used = np.zeros(37), np.zeros(3), _L(0)
    rc = _lib().r3g_emu_mf_step(v.ctypes.data, len(v), f.ctypes.data, len(f), int(resolution), p.ctypes.data, len(p), wp,
                                x.ctypes.data, int(mode), float(max_dist), sums.ctypes.data, ctypes.byref(used), centre.ctypes.data)
    if rc:
        raise ValueError("meshfit emu: error %d" % rc)
    return sums[:TERMS[mode]], used.value, centre


def fit(points, verts, faces, mode=PLANE, with_scale=False, init=None, weights=None, max_iterations=30, tolerance=1e-7,
        max_dist=float("inf")):
    """the loop of r3g_meshfit -> (matrix float64 [4,4], info dict)"""
    v, f = _mesh(verts, faces)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    w, wp = _weights(weights, len(p))
    m0 = None if init is None else np.ascontiguousarray(init, np.float64).reshape(16)
    m, info = np.zeros(16), np.zeros(5)
    rc = _lib().r3g_emu_mf_fit(v.ctypes.data, len(v), f.ctypes.data, len(f), p.ctypes.data, len(p), wp,
                               None if m0 is None else m0.ctypes.data, int(mode), int(bool(with_scale)), int(max_iterations),
                               float(tolerance), float(max_dist), m.ctypes.data, info.ctypes.data)
    if rc:
        raise ValueError("meshfit emu: error %d" % rc)
    return m.reshape(4, 4), {"iterations": int(info[0]), "converged": bool(info[1]), "rms": float(info[2]), "used": int(info[3]),
                             "scale": float(info[4])}


def solve(sums, mode, with_scale=False, centre=(0.0, 0.0, 0.0)):
    """the host solver on given sums -> (s, R [3,3], t [3], dropped columns)"""
    s = np.zeros(37)
    s[:len(sums)] = sums
    c = np.ascontiguousarray(centre, np.float64)
    out, dropped = np.zeros(13), _I(0)
    rc = _lib().r3g_emu_mf_solve(s.ctypes.data, int(mode), int(bool(with_scale)), c.ctypes.data, out.ctypes.data, ctypes.byref(dropped))
    if rc:
        raise ValueError("meshfit emu: error %d" % rc)
    return float(out[0]), out[1:10].reshape(3, 3).copy(), out[10:13].copy(), dropped.value


def compose(a, b):
    a = np.ascontiguousarray(a, np.float64).reshape(16)
    b = np.ascontiguousarray(b, np.float64).reshape(16)
    out = np.zeros(16)
    _lib().r3g_emu_mf_compose(a.ctypes.data, b.ctypes.data, out.ctypes.data)
    return out.reshape(4, 4)
