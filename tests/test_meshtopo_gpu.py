"""Mesh topology on the GPU (include/r3g.h r3g_meshtopo_*, r3g/meshtopo.py, Mesh.is_watertight ..., compat trimesh.repair):
mate, body, flip, every report field and the rewritten faces equal to the host twin of csrc/meshtopo_core.h
(tests/emu_meshtopo.py), exactly."""
import ctypes
import os

import numpy as np
import pytest

import emu_meshtopo as emu
import meshdist_ref as mref
import meshtopo_ref as ref

pytestmark = pytest.mark.gpu

_CACHE = {}


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def gpu_state(verts, faces, n_verts=None):
    """build + mates + bodies -> the twin's dict (report without the derived entries)"""
    from r3g import ffi, meshtopo
    with ffi.device_lock(0):
        rep = meshtopo.build(None if verts is None else dev(verts), dev(faces, np.int32), n_verts)
        mate = meshtopo.mates(0).cpu().numpy()
        body, flip = (t.cpu().numpy() for t in meshtopo.bodies(0))
    return {"mate": mate, "body": body, "flip": flip, "report": {k: rep[k] for k in emu.REPORT_FIELDS}, "derived": rep}


def assert_same(g, e):
    assert g["report"] == e["report"]
    for k in ("mate", "body", "flip"):
        assert np.array_equal(g[k], e[k]), k


def golden_b():
    if "B" not in _CACHE:
        v, f = ref.golden_mesh("B")
        _CACHE["B"] = (v, f, emu.build(v, f))
    return _CACHE["B"]


@pytest.mark.parametrize("nf", [1, 63, 64, 65, 4097, None])
def test_prefixes_of_the_noise_mesh_equal_the_twin(nf):
    """prefixes open boundaries and non-manifold fans, and cross the wave and block edges; None: the whole mesh"""
    v, f, whole = golden_b()
    e = whole if nf is None else emu.build(v, f[:nf])
    assert_same(gpu_state(v, f if nf is None else f[:nf]), e)
    if nf is None:
        assert e["report"]["bodies"] > 1
        assert_same(gpu_state(None, f, len(v)), emu.build(None, f, n_verts=len(v)))


@pytest.mark.parametrize("name", ["cube", "cube_reversed_0", "cube_reversed_5", "moebius", "shared_edge", "two_balls", "torus"])
def test_fixtures_equal_the_twin(name):
    from r3g import meshtopo
    v, f = {"cube": ref.cube, "cube_reversed_0": lambda: ref.cube_reversed(0), "cube_reversed_5": lambda: ref.cube_reversed(5),
            "moebius": ref.moebius, "shared_edge": ref.shared_edge, "two_balls": ref.two_balls, "torus": ref.torus}[name]()
    assert_same(gpu_state(v, f), emu.build(v, f))
    for outward in (0, 1, 2):
        e = emu.orient(v, f, outward)
        dv, df = dev(v), dev(f, np.int32)
        out, info = meshtopo.fix_winding(dv, df) if outward == 0 else meshtopo.fix_normals(dv, df, multibody=outward == 1)
        assert out.data_ptr() == df.data_ptr()                           # in place
        assert np.array_equal(out.cpu().numpy(), e["faces"])
        assert (info["faces_reversed"], info["bodies_reversed"]) == (e["faces_reversed"], e["bodies_reversed"])
        assert {k: info["report"][k] for k in emu.REPORT_FIELDS} == e["report"]
        # idempotent: a second call on its own output reverses nothing
        out2, info2 = meshtopo.fix_winding(dv, out) if outward == 0 else meshtopo.fix_normals(dv, out, multibody=outward == 1)
        assert info2["faces_reversed"] == 0 and info2["bodies_reversed"] == 0 and np.array_equal(out2.cpu().numpy(), e["faces"])


@pytest.mark.parametrize("cube_first", [True, False])
def test_an_unorientable_body_weighs_on_no_reversal(cube_first):
    """the outward cube beside a Moebius strip whose det-sum is large and negative: outward 1 and 2 leave the cube outward (or
    turn it outward), never touch the strip, and a second and third call reverse nothing"""
    from r3g import meshtopo
    v, f = ref.cube_and_moebius(cube_first)
    g = gpu_state(v, f)
    assert_same(g, emu.build(v, f))
    assert g["report"]["bodies"] == 2 and g["report"]["unorientable"] == 1 and g["report"]["six_volume_q"] < 0
    cube_faces = np.arange(12) + (0 if cube_first else len(f) - 12)
    inward = f.copy()
    inward[cube_faces] = inward[cube_faces][:, ::-1]
    dv = dev(v)
    for outward in (1, 2):
        for start, want in ((f, (0, 0)), (inward, (12, 1))):
            e = emu.orient(v, start, outward)
            out, info = meshtopo.fix_normals(dv, dev(start, np.int32), multibody=outward == 1)
            assert np.array_equal(out.cpu().numpy(), f) and np.array_equal(e["faces"], f)
            assert (info["faces_reversed"], info["bodies_reversed"]) == want == (e["faces_reversed"], e["bodies_reversed"])
            for _ in range(2):
                out, info = meshtopo.fix_normals(dv, out, multibody=outward == 1)
                assert info["faces_reversed"] == 0 and info["bodies_reversed"] == 0 and np.array_equal(out.cpu().numpy(), f)


def test_face_adjacency_has_one_row_per_shared_edge():
    from r3g import meshtopo
    for v, f in (ref.double_face(), ref.cube(), ref.shared_edge()):
        adj = meshtopo.face_adjacency(dev(v), dev(f, np.int32)).cpu().numpy()
        assert np.array_equal(adj, ref.build(v, f)["adjacency"])
    assert meshtopo.face_adjacency(*(dev(a, t) for a, t in zip(ref.double_face(), (np.float32, np.int32)))).tolist() == [[0, 1]] * 3


def test_long_chain_and_its_permutation():
    """a strip of 4097 triangles, every other one reversed: the chain is as long as the mesh"""
    from r3g import ffi, meshtopo
    v, f = ref.strip(4097)
    e = emu.build(v, f)
    r0 = ffi.counter("meshtopo_rounds"), ffi.counter("meshtopo_builds")
    g = gpu_state(v, f)
    assert ffi.counter("meshtopo_rounds") > r0[0] and ffi.counter("meshtopo_builds") == r0[1] + 1
    assert_same(g, e)
    assert np.array_equal(g["flip"], np.arange(4097) % 2) and g["report"]["bodies"] == 1 and g["report"]["clash"] == 4096
    out, info = meshtopo.fix_winding(dev(v), dev(f, np.int32))
    changed = np.flatnonzero((out.cpu().numpy() != f).any(1))
    assert np.array_equal(changed, np.arange(1, 4097, 2)) and info["faces_reversed"] == 2048
    assert info["report"]["clash"] == 0
    # the same mesh with its faces permuted: the same report, and mate is the permuted image
    perm = np.random.default_rng(3).permutation(4097)
    gp = gpu_state(v, f[perm])
    assert gp["report"] == g["report"]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(4097)
    m = g["mate"][perm]                                                  # mates of the new faces, in old half-edge ids
    want = np.where(m >= 0, 3 * inv[np.maximum(m, 0) // 3] + m % 3, m)
    assert np.array_equal(gp["mate"], want)
    assert_same(gp, emu.build(v, f[perm]))


def sphere65():
    """the product's marching cubes and dual marching cubes of the 65^3 sphere (golden A), on the device"""
    if "sphere" not in _CACHE:
        from r3g import dmc, mc
        vol = dev(mref.sphere_volume(400))
        _CACHE["sphere"] = {"mc": mc.marching_cubes(vol, 0.5), "dmc": dmc.dual_marching_cubes(vol, 0.5)}
    return _CACHE["sphere"]


@pytest.mark.parametrize("algo", ["mc", "dmc"])
def test_the_products_spheres_are_closed_surfaces(algo):
    """Both generators give a watertight, consistently wound sphere of Euler number 2 and of positive volume as the stage ships
    it.  r3g.mc.marching_cubes itself returns skimage's face order, which winds this field inward (the oracle's mesh of the
    same volume does: tests/test_meshtopo_cpu.py::test_golden_sphere); the stage's mesh is mc.extract_mesh, which carries the
    faces[:, ::-1] of hy3dgen's export, and that one has to be positive.  Dual marching cubes winds outward by itself."""
    from r3g import mc, meshtopo
    v, f = sphere65()[algo]
    rep = meshtopo.build(v, f)
    assert rep["watertight"] and rep["winding_consistent"] and rep["euler"] == 2 and rep["bodies"] == 1
    assert rep["unorientable"] == 0 and rep["skipped"] == 0
    assert_same(gpu_state(v.cpu().numpy(), f.cpu().numpy()), emu.build(v.cpu().numpy(), f.cpu().numpy()))
    if algo == "mc":
        assert rep["six_volume_q"] < 0
        shipped = meshtopo.build(v, f.flip(1).contiguous())
        assert shipped["six_volume_q"] == -rep["six_volume_q"] and shipped["winding_consistent"] and shipped["watertight"]
        v, f = mc.extract_mesh(dev(mref.sphere_volume(400)), 0.5)
        rep = meshtopo.build(v, f)
        assert rep["watertight"] and rep["winding_consistent"] and rep["euler"] == 2 and rep["bodies"] == 1
    assert rep["six_volume_q"] > 0 and rep["volume"] > 0
    out, info = meshtopo.fix_normals(v, f.clone())
    assert info["faces_reversed"] == 0 and info["bodies_reversed"] == 0


def test_reduced_sphere_equals_the_twin():
    """after the quadric edge collapse only device == twin is asserted; what the report shows is recorded in profiles/meshtopo.md"""
    from r3g import meshops
    v, f = sphere65()["mc"]
    rv, rf = meshops.reduce_faces(v, f, 2000)
    rv, rf = rv.cpu().numpy(), rf.cpu().numpy()
    g = gpu_state(rv, rf)
    assert_same(g, emu.build(rv, rf))
    print("reduce_faces(sphere65, 2000):", g["report"])


def test_mesh_and_the_trimesh_stand_in():
    import importlib.util
    import r3g
    from r3g.mesh import Mesh
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(r3g.__file__))), "compat", "trimesh", "__init__.py")
    spec = importlib.util.spec_from_file_location("r3g_compat_trimesh", path)      # under a private name: sys.modules keeps no trimesh
    trimesh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(trimesh)
    assert trimesh.__r3g_compat__
    v, f = ref.cube_reversed(5)
    m = trimesh.Trimesh(v, f, process=False)
    assert m.is_watertight and not m.is_winding_consistent and not m.is_volume
    assert m.euler_number == 2 and m.body_count == 1
    assert len(m.face_adjacency) == 18 and np.array_equal(m.face_adjacency, ref.build(v, f)["adjacency"])
    trimesh.repair.fix_normals(m)
    assert np.array_equal(m.faces, ref.cube()[1]) and m.is_winding_consistent and m.is_volume
    assert m.volume == 1.0 and m.area == 6.0
    assert m.invert().volume == -1.0 and not m.is_volume
    trimesh.repair.fix_inversion(m, multibody=True)
    assert m.volume == 1.0 and np.array_equal(m.faces, ref.cube()[1])
    trimesh.repair.fix_winding(m)
    assert np.array_equal(m.faces, ref.cube()[1])
    assert len(trimesh.repair.broken_faces(m)) == 0
    open_cube = Mesh(v, ref.cube()[1][:-1])
    assert not open_cube.is_watertight
    assert trimesh.repair.broken_faces(open_cube, color=[255, 0, 0, 255]).tolist() == ref.build(v, ref.cube()[1][:-1])["broken"].tolist()
    assert (open_cube.face_colors[trimesh.repair.broken_faces(open_cube)] == [255, 0, 0, 255]).all()
    dm = Mesh.from_device(dev(v), dev(f, np.int32))                      # a device-born mesh
    assert dm.fix_normals(multibody=True) is dm and np.array_equal(dm.faces, ref.cube()[1])


def test_error_paths_and_non_finite_vertices():
    import torch
    from r3g import ffi, meshtopo
    lib = ffi.lib()
    fresh = ffi.new_context(0)
    try:
        raw = (ctypes.c_int64 * 16)()
        buf = torch.empty(64, dtype=torch.int32, device="cuda")
        none = ctypes.c_void_p(0)
        assert lib.r3g_meshtopo_report(fresh, raw) == -4                  # R3G_ERR_STATE
        assert lib.r3g_meshtopo_mates(fresh, ctypes.c_void_p(buf.data_ptr()), none) == -4
        assert lib.r3g_meshtopo_bodies(fresh, ctypes.c_void_p(buf.data_ptr()), none, none) == -4
        assert lib.r3g_meshtopo_build(fresh, none, 8, ctypes.c_void_p(buf.data_ptr()), 0, raw, none) == -1
        assert lib.r3g_meshtopo_build(fresh, none, 8, ctypes.c_void_p(buf.data_ptr()), (1 << 29) + 1, raw, none) == -1
        assert lib.r3g_meshtopo_orient(fresh, none, 8, ctypes.c_void_p(buf.data_ptr()), 4, 3, None, None, none) == -1
        assert lib.r3g_meshtopo_orient(fresh, none, 8, ctypes.c_void_p(buf.data_ptr()), 4, 1, None, None, none) == -1
        # a failed build leaves no state, on a context that had one
        v, f = ref.cube()
        dv, df = dev(v), dev(f, np.int32)
        torch.cuda.synchronize()
        assert lib.r3g_meshtopo_build(fresh, ctypes.c_void_p(dv.data_ptr()), 8, ctypes.c_void_p(df.data_ptr()), 12, raw, none) == 0
        assert lib.r3g_meshtopo_report(fresh, raw) == 0
        bad = f.copy()
        bad[7, 1] = 8
        dbad = dev(bad, np.int32)
        torch.cuda.synchronize()
        assert lib.r3g_meshtopo_build(fresh, ctypes.c_void_p(dv.data_ptr()), 8, ctypes.c_void_p(dbad.data_ptr()), 12, raw, none) == -2
        assert lib.r3g_meshtopo_report(fresh, raw) == -4
        assert lib.r3g_meshtopo_orient(fresh, ctypes.c_void_p(dv.data_ptr()), 8, ctypes.c_void_p(dbad.data_ptr()), 12, 2, None, None, none) == -2
        assert np.array_equal(dbad.cpu().numpy(), bad)                   # nothing was rewritten
    finally:
        lib.r3g_destroy(fresh)
    with pytest.raises(ffi.R3GError) as err:
        meshtopo.build(dv, dev(np.array([[0, 1, -1]]), np.int32))
    assert err.value.code == -2
    w = v.copy()
    w[3, 1] = np.nan
    g, e = gpu_state(w, f), emu.build(w, f)
    assert_same(g, e)
    clean = emu.build(v, f)
    assert g["report"]["nonfinite"] == int((f == 3).any(1).sum()) and np.array_equal(g["mate"], clean["mate"])
    assert all(g["report"][k] == clean["report"][k] for k in ("edges", "boundary", "clash", "nonmanifold", "bodies", "euler"))
    extra = np.concatenate([f, [[2, 2, 5]]])                             # a face that repeats an index is skipped
    assert_same(gpu_state(v, extra), emu.build(v, extra))
