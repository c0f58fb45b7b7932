"""ctypes loader for tests/emu/facecloud_twin.cpp (host run of the product's face-to-cloud core; test-only).  Built by tests/emu_build.py:
`library()` is emu_build.shared("facecloud") and `selftest_binary()` emu_build.program("facecloud", ...), so the flags that decide
the twin's arithmetic are that builder's and nobody's copy.  The row `"facecloud": ["facecloud_twin.cpp"]` is put into
emu_build.TWINS for the length of the call and taken out again: tests/emu_build.py itself stays as it is, and the source's name is
not *_emu.cpp, because the registry test holds the written table to the *_emu.cpp files present.  Built on first use, by content."""
import ctypes

import numpy as np

import emu_build

SOURCES = ["facecloud_twin.cpp"]
_LIB = None
_I64P = ctypes.POINTER(ctypes.c_int64)
_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64

MUTANTS = {"none": 0, "tie_less_equal": 1, "no_bin_margin": 2, "no_slack": 3, "stop_without_other": 4, "ring_without_corners": 5, "swap_bc": 6}
MODES = {"device": 0, "narrow": 1, "wide": 2}
REPORT = ("usable", "tests", "wide", "max_ring")


def _with_row(build):
    """build() while emu_build.TWINS carries this twin's row"""
    table = emu_build.TWINS
    emu_build.TWINS = dict(table, facecloud=SOURCES)
    try:
        return build()
    finally:
        emu_build.TWINS = table


def library():
    """the twin as a shared library for ctypes -> path (fresh by content, as every artefact of emu_build)"""
    return _with_row(lambda: emu_build.shared("facecloud"))


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(library())
        lib.r3g_emu_facecloud_wide_cells.restype = _I
        lib.r3g_emu_facecloud_wide_cells.argtypes = []
        lib.r3g_emu_facecloud_brute.restype = _I
        lib.r3g_emu_facecloud_brute.argtypes = [_P, _L, _P, _L, _P, _L, _I, _P, _P, _P, _P, _I64P]
        lib.r3g_emu_facecloud_grid.restype = _I
        lib.r3g_emu_facecloud_grid.argtypes = [_P, _L, _I, _I, _I, _I, _P, _L, _P, _L, _P, _P, _P, _P, _I64P, ctypes.POINTER(_I)]
        lib.r3g_emu_facecloud_gather.restype = _I
        lib.r3g_emu_facecloud_gather.argtypes = [_L, _L, _P, _P, _P, _P, _P, _P, _P]
        lib.r3g_emu_facecloud_tri.restype = _I
        lib.r3g_emu_facecloud_tri.argtypes = [_P, _P, _L, _P, _P, _P, _P, _P]
        _LIB = lib
    return _LIB


def wide_cells():
    """the product's kWideCells"""
    return int(_lib().r3g_emu_facecloud_wide_cells())


def _arrays(points, verts, faces):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    n = len(f)
    return p, v, f, np.empty(n, np.float32), np.empty(n, np.int32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)


def brute(points, verts, faces, mutant="none"):
    """(a): every usable point against every face -> (dist2 [F], index [F], weights [F,3], diff [F,3], report dict)"""
    p, v, f, d2, ix, w, df = _arrays(points, verts, faces)
    rep = (ctypes.c_int64 * 4)()
    rc = _lib().r3g_emu_facecloud_brute(p.ctypes.data, len(p), v.ctypes.data, len(v), f.ctypes.data, len(f), MUTANTS[mutant], d2.ctypes.data,
                                        ix.ctypes.data, w.ctypes.data, df.ctypes.data, rep)
    if rc:
        raise ValueError("facecloud emu: error %d" % rc)
    return d2, ix, w, df, dict(zip(REPORT, (int(x) for x in rep)))


def grid(points, verts, faces, resolution=0, reverse_fill=False, mode="device", mutant="none"):
    """(b): the cloud's grid and the product's walk in host loops -> (dist2, index, weights, diff, report dict with `resolution`).
    mode "device": wide above kWideCells cells, as the kernels classify; "narrow" / "wide": every face down that enumeration"""
    p, v, f, d2, ix, w, df = _arrays(points, verts, faces)
    rep, res = (ctypes.c_int64 * 4)(), ctypes.c_int(0)
    rc = _lib().r3g_emu_facecloud_grid(p.ctypes.data, len(p), int(resolution), int(bool(reverse_fill)), MODES[mode], MUTANTS[mutant], v.ctypes.data,
                                       len(v), f.ctypes.data, len(f), d2.ctypes.data, ix.ctypes.data, w.ctypes.data, df.ctypes.data, rep,
                                       ctypes.byref(res))
    if rc:
        raise ValueError("facecloud emu: error %d" % rc)
    return d2, ix, w, df, dict(zip(REPORT, (int(x) for x in rep)), resolution=res.value)


def gather(n_verts, grad_dist2, index, weights, diff, corner_start, corner_ids):
    """the backward of fc_gather on the host -> grad_verts float32 [V,3]"""
    g = np.ascontiguousarray(grad_dist2, np.float32).reshape(-1)
    ix = np.ascontiguousarray(index, np.int32).reshape(-1)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, 3)
    df = np.ascontiguousarray(diff, np.float32).reshape(-1, 3)
    cs = np.ascontiguousarray(corner_start, np.int32).reshape(-1)
    ci = np.ascontiguousarray(corner_ids, np.int32).reshape(-1)
    if len(cs) != n_verts + 1 or not (len(g) == len(ix) == len(w) == len(df)):
        raise ValueError("facecloud emu: gather sizes")
    out = np.empty((n_verts, 3), np.float32)
    rc = _lib().r3g_emu_facecloud_gather(int(n_verts), len(g), g.ctypes.data, ix.ctypes.data, w.ctypes.data, df.ctypes.data, cs.ctypes.data,
                                         ci.ctypes.data, out.ctypes.data)
    if rc:
        raise ValueError("facecloud emu: error %d" % rc)
    return out


def corner_csr(faces, n_verts):
    """r3g.softras.corner_csr on the host: for every vertex its corners 3 f + a in ascending order; indices outside [0, V) are in no list
    -> (corner_start int32 [V + 1], corner_ids int32)"""
    flat = np.ascontiguousarray(faces, np.int32).reshape(-1)
    ok = (flat >= 0) & (flat < n_verts)
    ids = np.nonzero(ok)[0]
    order = np.argsort(flat[ids], kind="stable")
    start = np.zeros(n_verts + 1, np.int64)
    np.add.at(start, flat[ids] + 1, 1)
    return np.cumsum(start).astype(np.int32), ids[order].astype(np.int32)


def tri_pairs(points, triangles):
    """tri_nearest_w and section 4f's tri_closest on n (point, triangle [3,3]) pairs -> (d2_w, r_w, weights, d2_closest, r_closest)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.float32).reshape(-1, 9)
    n = len(p)
    d2w, rw, w, d2c, rc_ = np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty((n, 3), np.float32)
    _lib().r3g_emu_facecloud_tri(p.ctypes.data, t.ctypes.data, n, d2w.ctypes.data, rw.ctypes.data, w.ctypes.data, d2c.ctypes.data, rc_.ctypes.data)
    return d2w, rw, w, d2c, rc_


def selftest_binary(sanitize=True):
    """the twin with its own main(), as a stand-alone program (host only; -fsanitize=address,undefined) -> path"""
    return _with_row(lambda: emu_build.program("facecloud", defines=("FACECLOUD_EMU_MAIN",), sanitize=sanitize))
