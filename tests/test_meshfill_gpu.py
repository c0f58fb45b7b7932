"""Hole filling on the GPU (include/r3g.h r3g_meshfill_*, r3g/meshfill.py, Mesh.fill_holes, compat trimesh.repair.fill_holes):
every report field, loop_start, loop_verts, status, the appended faces and the appended float32 vertices equal to the host twin of
csrc/meshfill_core.h (tests/emu_meshfill.py), exactly."""
import ctypes

import numpy as np
import pytest

import emu_meshfill as emu
import emu_meshtopo as temu
import meshfill_ref as ref
import meshtopo_ref as tref

pytestmark = pytest.mark.gpu

_CACHE = {}


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def gpu_plan(verts, faces, max_loop=64, mode="fan", n_verts=None):
    """plan + loops + emit through the C ABI -> the twin's dict"""
    import torch
    from r3g import ffi, meshfill
    f = dev(faces, np.int32)
    v = None if verts is None else dev(verts)
    with ffi.device_lock(0):
        _, _, rep = meshfill._plan(v, f, n_verts, max_loop, mode)
        start = torch.full((rep["loops"] + 1,), -7, dtype=torch.int64, device="cuda")
        lverts = torch.full((rep["loop_edges"],), -7, dtype=torch.int32, device="cuda")
        status = torch.full((rep["loops"],), -7, dtype=torch.int32, device="cuda")
        new_f = torch.full((rep["faces_added"], 3), -7, dtype=torch.int32, device="cuda")
        new_v = torch.full((rep["verts_added"], 3), -7.0, dtype=torch.float32, device="cuda")
        L = ffi.lib()
        ffi.check(L.r3g_meshfill_loops(ffi.context(0), ctypes.c_void_p(start.data_ptr()), ctypes.c_void_p(lverts.data_ptr() if rep["loops"] else 0),
                                       ctypes.c_void_p(status.data_ptr() if rep["loops"] else 0), ffi.stream_ptr()))
        ffi.check(L.r3g_meshfill_emit(ffi.context(0), ctypes.c_void_p(new_f.data_ptr() if rep["faces_added"] else 0),
                                      ctypes.c_void_p(new_v.data_ptr() if rep["verts_added"] else 0), ffi.stream_ptr()))
        torch.cuda.synchronize()
    return {"report": rep, "loop_start": start.cpu().numpy(), "loop_verts": lverts.cpu().numpy(), "status": status.cpu().numpy(),
            "new_faces": new_f.cpu().numpy(), "new_verts": new_v.cpu().numpy()}


def assert_same(g, e):
    assert g["report"] == e["report"]
    for k in ("loop_start", "loop_verts", "status", "new_faces"):
        assert np.array_equal(g[k], e[k]), k
    assert g["new_verts"].tobytes() == e["new_verts"].tobytes()


def topo_fields(rep):
    return {k: rep[k] for k in temu.REPORT_FIELDS}


def golden_b():
    if "B" not in _CACHE:
        _CACHE["B"] = tref.golden_mesh("B")
    return _CACHE["B"]


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 129, 4097])
def test_open_cones_equal_the_twin(n):
    """one loop of n edges: across the wave edge, the block edge and the round counts; both modes; max_loop = n fills it (watertight,
    Euler number 2), max_loop = n - 1 leaves it oversize and returns the tensors as given; a seeded permutation moves the leader"""
    from r3g import ffi, meshfill
    v, f = ref.cone(n)
    for faces in (f, ref.permuted(f, n)):
        dv, df = dev(v), dev(faces, np.int32)
        for mode in ("fan", "centroid"):
            e = emu.plan(v, faces, max_loop=n, mode=mode)
            assert_same(gpu_plan(v, faces, max_loop=n, mode=mode), e)
            assert (e["report"]["filled"], e["report"]["longest"], e["report"]["rounds"]) == (1, n, max(1, (n - 1).bit_length()))
            ov, of, info = meshfill.fill_holes(dv, df, max_loop=n, mode=mode)
            ev, ef, _ = emu.fill_holes(v, faces, max_loop=n, mode=mode)
            assert np.array_equal(of.cpu().numpy(), ef) and ov.cpu().numpy().tobytes() == ev.tobytes()
            assert {k: info[k] for k in emu.REPORT_FIELDS} == e["report"]
            assert topo_fields(info["topology"]) == temu.build(ev, ef)["report"]
            assert info["topology"]["watertight"] and info["topology"]["euler"] == 2 and info["topology"]["winding_consistent"]
            if n == 3:
                with pytest.raises(ffi.R3GError) as err:             # max_loop = n - 1 = 2 is below the smallest loop there is
                    meshfill.fill_holes(dv, df, max_loop=2, mode=mode)
                assert err.value.code == -1
                continue
            assert_same(gpu_plan(v, faces, max_loop=n - 1, mode=mode), emu.plan(v, faces, max_loop=n - 1, mode=mode))
            ov, of, info = meshfill.fill_holes(dv, df, max_loop=n - 1, mode=mode)
            assert ov is dv and of is df
            assert (info["oversize"], info["filled"], info["faces_added"], info["verts_added"]) == (1, 0, 0, 0)
            assert not info["topology"]["watertight"] and info["topology"]["boundary"] == n


def test_open_tube_has_two_loops_in_leader_order():
    from r3g import meshfill
    v, f = ref.tube(65)
    for mode in ("fan", "centroid"):
        e = emu.plan(v, f, max_loop=65, mode=mode)
        g = gpu_plan(v, f, max_loop=65, mode=mode)
        assert_same(g, e)
        assert g["report"]["loops"] == 2 and g["loop_start"].tolist() == [0, 65, 130] and g["status"].tolist() == [0, 0]
        assert g["loop_verts"][0] == 0 and g["loop_verts"][65] >= 65          # the lower rim holds half-edge 0: it leads
    start, lverts, status = meshfill.boundary_loops(dev(v), dev(f, np.int32), max_loop=64)
    assert np.array_equal(start.cpu().numpy(), e["loop_start"]) and np.array_equal(lverts.cpu().numpy(), e["loop_verts"])
    assert status.tolist() == [1, 1]
    start2, lverts2, _ = meshfill.boundary_loops(None, dev(f, np.int32), n_verts=len(v))
    assert np.array_equal(start2.cpu().numpy(), e["loop_start"]) and np.array_equal(lverts2.cpu().numpy(), e["loop_verts"])


def test_bow_tie_is_tangled_and_left_alone():
    from r3g import meshfill
    v, f = ref.bow_tie()
    g = gpu_plan(v, f)
    assert_same(g, emu.plan(v, f))
    assert g["report"]["boundary"] == 10 and g["report"]["tangled"] == 10 and g["report"]["loops"] == 0 and g["report"]["faces_added"] == 0
    dv, df = dev(v), dev(f, np.int32)
    ov, of, info = meshfill.fill_holes(dv, df)
    assert ov is dv and of is df and info["tangled"] == info["boundary"] == 10


def test_reversed_face_breaks_the_loop_until_the_winding_is_fixed():
    from r3g import meshfill, meshtopo
    v, f = ref.cone(7)
    bent = f.copy()
    bent[3] = bent[3, ::-1]
    g = gpu_plan(v, bent)
    assert_same(g, emu.plan(v, bent))
    assert g["report"]["loops"] == 0 and g["report"]["tangled"] == g["report"]["boundary"] == 7 and g["report"]["faces_added"] == 0
    dv, df = dev(v), dev(bent, np.int32)
    fixed, _ = meshtopo.fix_winding(dv, df)
    ov, of, info = meshfill.fill_holes(dv, fixed, max_loop=7)
    ev, ef, erep = emu.fill_holes(v, temu.orient(v, bent, 0)["faces"], max_loop=7)
    assert np.array_equal(of.cpu().numpy(), ef) and {k: info[k] for k in emu.REPORT_FIELDS} == erep
    assert info["filled"] == 1 and info["faces_added"] == 5 and info["topology"]["watertight"]


def test_closed_cube_has_nothing_to_fill():
    import torch
    from r3g import ffi, meshfill
    v, f = tref.cube()
    before = ffi.counter("meshfill_plans"), ffi.counter("meshfill_rounds"), ffi.counter("meshtopo_builds")
    g = gpu_plan(v, f)
    assert_same(g, emu.plan(v, f))
    assert (ffi.counter("meshfill_plans"), ffi.counter("meshfill_rounds"), ffi.counter("meshtopo_builds")) == (before[0] + 1, before[1], before[2] + 1)
    assert g["report"]["boundary"] == 0 and g["report"]["rounds"] == 0 and g["loop_start"].tolist() == [0]
    # emit writes nothing
    guard = torch.full((4, 3), -7, dtype=torch.int32, device="cuda")
    with ffi.device_lock(0):
        meshfill._plan(dev(v), dev(f, np.int32), None, 64, "centroid")
        ffi.check(ffi.lib().r3g_meshfill_emit(ffi.context(0), ctypes.c_void_p(guard.data_ptr()), ctypes.c_void_p(0), ffi.stream_ptr()))
    torch.cuda.synchronize()
    assert (guard == -7).all()
    # a plan with a boundary moves the round counter by twice its rounds
    r0 = ffi.counter("meshfill_rounds")
    g = gpu_plan(v, f[:-2])
    assert ffi.counter("meshfill_rounds") - r0 == 2 * g["report"]["rounds"] == 4


@pytest.mark.parametrize("nf", [1, 63, 64, 65, 4097])
def test_prefixes_of_the_noise_mesh_equal_the_twin(nf):
    """prefixes hold boundaries, non-manifold fans, clashes and skipped faces all at once"""
    v, f = golden_b()
    for mode in ("fan", "centroid"):
        for max_loop in (4, 64):
            assert_same(gpu_plan(v, f[:nf], max_loop=max_loop, mode=mode), emu.plan(v, f[:nf], max_loop=max_loop, mode=mode))
    assert_same(gpu_plan(None, f[:nf], n_verts=len(v)), emu.plan(None, f[:nf], n_verts=len(v)))


def test_error_paths():
    import torch
    from r3g import ffi, meshfill
    v, f = tref.cube()
    dv, df = dev(v), dev(f[:-2], np.int32)
    ctx = ffi.new_context(0)
    try:
        L = ffi.lib()
        rep = (ctypes.c_int64 * 16)()
        out = torch.zeros((4, 3), dtype=torch.int32, device="cuda")

        def plan(faces, nv, max_loop, mode, verts=dv):
            return L.r3g_meshfill_plan(ctx, ctypes.c_void_p(verts.data_ptr() if verts is not None else 0), nv,
                                       ctypes.c_void_p(faces.data_ptr()), faces.shape[0], max_loop, mode, rep, ffi.stream_ptr())

        def emit():
            return L.r3g_meshfill_emit(ctx, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(0), ffi.stream_ptr())

        state_err = emit()                                        # emit before any plan
        assert state_err == -4                                    # R3G_ERR_STATE
        with pytest.raises(ffi.R3GError) as err:
            ffi.check(state_err)
        assert "no successful r3g_meshfill_plan" in str(err.value)
        assert L.r3g_meshfill_loops(ctx, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(0), ctypes.c_void_p(0), ffi.stream_ptr()) == state_err
        assert plan(df, 8, 2, 0) == -1 and plan(df, 8, 64, 2) == -1 and plan(df, 8, 64, -1) == -1
        assert plan(df, 8, 64, 1, verts=None) == -1 and plan(df[:0], 8, 64, 0) == -1
        bad = f[:-2].copy()
        bad[4, 1] = 8
        assert plan(dev(bad, np.int32), 8, 64, 0) == -2
        assert plan(df, 7, 64, 0) == -2
        assert emit() == state_err                                # a failed plan leaves no state
        assert plan(df, 8, 64, 0) == 0 and rep[7] == 2 and emit() == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy()[:2], emu.plan(v, f[:-2])["new_faces"])
        assert plan(df, 8, 2, 0) == -1 and emit() == state_err   # ... and takes the earlier one away
    finally:
        ffi.lib().r3g_destroy(ctx)
    with pytest.raises(ValueError):
        meshfill.fill_holes(dv, df, mode="ear")


def test_second_fill_adds_nothing():
    from r3g import meshfill
    for v0, f0, kw in ((tref.cube()[0], tref.cube()[1][:-2], {}), (ref.tube(65)[0], ref.tube(65)[1], {"max_loop": 65}),
                       (ref.cone(129)[0], ref.permuted(ref.cone(129)[1], 1), {"max_loop": 129, "mode": "centroid"})):
        ov, of, info = meshfill.fill_holes(dev(v0), dev(f0, np.int32), **kw)
        assert info["faces_added"] > 0 and info["oversize"] == 0 and info["tangled"] == 0
        ov2, of2, info2 = meshfill.fill_holes(ov, of, **kw)
        assert ov2 is ov and of2 is of and info2["boundary"] == 0 and info2["faces_added"] == 0


def test_mesh_and_the_trimesh_stand_in():
    from r3g.mesh import Mesh
    trimesh = ref.trimesh_stand_in()
    v, f = tref.cube()
    m = Mesh(v, f[:-2], process=False)
    assert not m.is_watertight
    assert m.fill_holes() is True and m.is_watertight and m.n_faces == 12 and m.n_vertices == 8
    assert np.array_equal(ref.canonical(m.faces), ref.canonical(np.concatenate([f[:-2], emu.plan(v, f[:-2])["new_faces"]])))
    m = trimesh.Trimesh(v, f[:-2], process=False)
    assert trimesh.repair.fill_holes(m) is True and m.is_watertight and m.is_volume
    m = Mesh(v, f[:-2], process=False)
    assert m.fill_holes(mode="centroid") is True and m.n_vertices == 9 and m.n_faces == 14 and m.vertices[8].tolist() == [0.5, 0.5, 1.0]
    with pytest.raises(ValueError):
        Mesh(v, f[:-2], vertex_colors=np.zeros((8, 4), np.uint8)).fill_holes(mode="centroid")
    # an L = 5 hole is beyond the compat default (trimesh's reach: triangles and quads)
    cv, cf = ref.cone(5)
    m = trimesh.Trimesh(cv, cf, process=False)
    assert trimesh.repair.fill_holes(m) is False and not m.is_watertight and m.n_faces == 5
    assert m.fill_holes() is True and m.n_faces == 8
    # the reference's repair sequence on an open mesh
    m = trimesh.Trimesh(v, f[:-2], process=False)
    trimesh.repair.fill_holes(m)
    trimesh.repair.fix_winding(m)
    trimesh.repair.fix_normals(m, multibody=True)
    assert len(trimesh.repair.broken_faces(m)) == 0 and m.is_volume
