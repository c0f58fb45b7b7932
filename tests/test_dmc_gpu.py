"""Dual marching cubes on the GPU (include/r3g.h r3g_dmc_count / r3g_dmc_emit, r3g/dmc.py, mc_algo="dmc" of the hy3dgen
mirror, the stage's r3g_mc_algo key) against the numpy restatement of DESIGN.md section 4c (tests/dmc_ref.py).
Bar: faces equal as integers, vertices equal bit for bit, in index space and through an output transform."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dmc_ref
from mc_volumes import CHUNK_BLOCKS, active_cells, chunk_edge_volumes, golden_volume, small_volumes
from test_dmc_cpu import bits_equal, check_padded_b, check_padded_small, check_sphere, padded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def gpu_dmc(vol, level, manifold=True, xform=None):
    """through the Python binding's internal entry (the same two C calls as dual_marching_cubes, plus an xform)"""
    from r3g import dmc
    v, f = dmc._run(dev(vol), level, manifold, xform, False)
    return v.cpu().numpy(), f.cpu().numpy()


def assert_gpu_equals_restatement(vol, level, tag, manifolds=(True, False)):
    n = np.array(vol.shape, np.float64)
    xf = (n - 1.0, np.array([2.02, 2.0, 1.5]), np.array([-1.01, -1.0, 0.3]))
    for manifold in manifolds:
        for xform in (None, xf):
            rv, rf, _ = dmc_ref.dual_marching_cubes(vol, level, manifold, xform)
            v, f = gpu_dmc(vol, level, manifold, xform)
            assert v.dtype == np.float32 and f.dtype == np.int32
            assert np.array_equal(f, rf), (tag, manifold, xform is not None)
            assert bits_equal(v, rv), (tag, manifold, xform is not None)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "B-padded"])
def test_goldens_equal_the_restatement(name):
    vol, level = golden_volume(name[0])
    if name.endswith("padded"):
        vol = padded(vol)
    assert_gpu_equals_restatement(vol, level, name, manifolds=(True,) if name == "D" else (True, False))


def test_small_volumes_and_error_codes():
    from r3g import dmc, ffi
    vols = small_volumes()
    names = [k for k in vols if not k.startswith("level_")]
    assert {"noise_ragged", "smooth_ragged", "noise_thin", "nan", "plane", "two_blobs", "minimal"} <= set(names)
    codes = {}
    for k in names:
        level = float(vols["level_" + k])
        try:
            dmc_ref.dual_marching_cubes(vols[k], level)
        except dmc_ref.DmcError as want:
            exc = {dmc_ref.R3G_ERR_LEVEL_RANGE: ffi.LevelRangeError, dmc_ref.R3G_ERR_NO_SURFACE: ffi.NoSurfaceError}[want.code]
            with pytest.raises(exc):
                dmc.dual_marching_cubes(dev(vols[k]), level)
            codes[k] = want.code
            continue
        assert_gpu_equals_restatement(vols[k], level, k)
    assert codes["outside_level"] == -10 and codes["lone_equal_below"] == -11 and codes["minimal"] == -11
    # the public entry is the manifold form in index space
    v, f = dmc.dual_marching_cubes(dev(vols["two_blobs"]), 0.5)
    rv, rf, _ = dmc_ref.dual_marching_cubes(vols["two_blobs"], 0.5)
    assert np.array_equal(f.cpu().numpy(), rf) and bits_equal(v.cpu().numpy(), rv)
    # the raw codes of the C ABI
    L = ffi.lib()
    ctx = ffi.context(0)
    nv, nf = ctypes.c_int64(), ctypes.c_int64()
    for k, code in (("outside_level", -10), ("lone_equal_below", -11), ("minimal", -11)):
        g = dev(vols[k])
        assert L.r3g_dmc_count(ctx, g.data_ptr(), *g.shape, float(vols["level_" + k]), 1, ctypes.byref(nv), ctypes.byref(nf),
                               None) == code, k


def test_random_ragged_volumes_equal_the_restatement():
    rng = np.random.default_rng(4321)
    for it in range(10):
        shape = tuple(int(x) for x in rng.integers(2, 60, 3))
        vol = rng.standard_normal(shape).astype(np.float32)
        if it % 3 == 1:
            vol = np.round(vol * 2).astype(np.float32)          # samples equal to the level
        if it % 3 == 2:
            for _ in range(2):
                for ax in range(3):
                    vol = (np.roll(vol, 1, ax) + 2 * vol + np.roll(vol, -1, ax)) / 4
        try:
            dmc_ref.dual_marching_cubes(vol, 0.0)
        except dmc_ref.DmcError:
            continue
        assert_gpu_equals_restatement(vol, 0.0, shape)


@pytest.mark.parametrize("shape", [(65, 65, 65), (65, 65, 66)])
def test_scan_chunk_edge_equals_the_restatement(shape):
    """1024 and 1040 blocks: the block-sum scan's chunk of 1024 blocks ends with the grid, and hands over to a second
    workgroup; the surface crosses the blocks either side of the edge (as tests/test_mc_gpu.py, same volumes)"""
    field, shifted, cells = chunk_edge_volumes(shape)
    nblk = -(-int(np.prod([n - 1 for n in shape])) // 256)
    act = np.flatnonzero(active_cells(shifted, 0.0).reshape(-1)) // 256
    assert {CHUNK_BLOCKS - 1, min(CHUNK_BLOCKS, nblk - 1)} <= set(act.tolist())
    rv, _, _ = dmc_ref.dual_marching_cubes(shifted, 0.0)
    for c in cells:         # the restatement's mesh has a vertex inside each cell the constant was chosen for
        lo = np.array(c, np.float32)
        assert np.any(np.all((rv >= lo) & (rv <= lo + 1), axis=1)), c
    assert_gpu_equals_restatement(field, 0.0, (shape, "field"))
    assert_gpu_equals_restatement(shifted, 0.0, (shape, "shifted"))


@pytest.mark.parametrize("name", ["A", "D"])
def test_golden_spheres_properties(name):
    vol, level = golden_volume(name)
    v, f = gpu_dmc(vol, level)
    check_sphere(name, v, f)


def test_manifold_rule_on_padded_noise():
    def run(vol, level, manifold):
        v, f = gpu_dmc(vol, level, manifold)
        return v, f, None
    check_padded_b(run)
    check_padded_small(run)


def test_emit_without_count_is_a_state_error_and_arguments_are_checked():
    import torch
    from r3g import ffi
    L = ffi.lib()
    ctx = ffi.new_context(0)
    try:
        v = torch.zeros((16, 3), device="cuda")
        f = torch.zeros((16, 3), dtype=torch.int32, device="cuda")
        assert L.r3g_dmc_emit(ctx, v.data_ptr(), f.data_ptr(), None, 0, None) == -4          # R3G_ERR_STATE
        nv, nf = ctypes.c_int64(), ctypes.c_int64()
        g = torch.zeros((1, 4, 4), device="cuda")
        assert L.r3g_dmc_count(ctx, g.data_ptr(), 1, 4, 4, 0.0, 1, ctypes.byref(nv), ctypes.byref(nf), None) == -1
        # a count that fails leaves no state behind for emit
        g = torch.full((4, 4, 4), -1.0, device="cuda")
        assert L.r3g_dmc_count(ctx, g.data_ptr(), 4, 4, 4, 0.0, 1, ctypes.byref(nv), ctypes.byref(nf), None) == -10
        assert L.r3g_dmc_emit(ctx, v.data_ptr(), f.data_ptr(), None, 0, None) == -4
        # reverse_faces writes every triangle backwards
        vols = small_volumes()
        g = dev(vols["smooth_12"])
        assert L.r3g_dmc_count(ctx, g.data_ptr(), *g.shape, 0.0, 1, ctypes.byref(nv), ctypes.byref(nf), None) == 0
        rv, rf, _ = dmc_ref.dual_marching_cubes(vols["smooth_12"], 0.0)
        assert (nv.value, nf.value) == (len(rv), len(rf))
        v = torch.empty((nv.value, 3), device="cuda")
        f = torch.empty((nf.value, 3), dtype=torch.int32, device="cuda")
        assert L.r3g_dmc_emit(ctx, v.data_ptr(), f.data_ptr(), None, 1, None) == 0
        assert np.array_equal(f.cpu().numpy(), rf[:, ::-1])
        assert L.r3g_dmc_emit(ctx, v.data_ptr(), f.data_ptr(), None, 0, None) == 0             # emit may be repeated
        assert np.array_equal(f.cpu().numpy(), rf) and bits_equal(v.cpu().numpy(), rv)
    finally:
        L.r3g_destroy(ctx)


def test_counted_mc_and_dmc_states_coexist():
    """a context holds a counted marching-cubes state and a counted dual-marching-cubes state at once: neither count
    touches the other's workspace, grid or layout"""
    import torch
    from oracle import mc as omc
    from r3g import ffi
    vols = small_volumes()
    X, lx = vols["smooth_12"], float(vols["level_smooth_12"])
    Y, ly = vols["noise_ragged"], float(vols["level_noise_ragged"])
    assert X.shape != Y.shape
    wv, wf = omc.marching_cubes(X, lx)
    rv, rf, _ = dmc_ref.dual_marching_cubes(Y, ly)
    L = ffi.lib()
    ctx = ffi.new_context(0)
    try:
        gx, gy = dev(X), dev(Y)
        nv, nf, mv, mf = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        assert L.r3g_mc_count(ctx, gx.data_ptr(), *gx.shape, lx, 0, ctypes.byref(nv), ctypes.byref(nf), None) == 0
        assert L.r3g_dmc_count(ctx, gy.data_ptr(), *gy.shape, ly, 1, ctypes.byref(mv), ctypes.byref(mf), None) == 0
        assert (nv.value, nf.value, mv.value, mf.value) == (len(wv), len(wf), len(rv), len(rf))
        v = torch.empty((nv.value, 3), device="cuda")
        f = torch.empty((nf.value, 3), dtype=torch.int32, device="cuda")
        assert L.r3g_mc_emit(ctx, v.data_ptr(), f.data_ptr(), None, 1, None) == 0      # reversed: skimage's winding
        dv = torch.empty((mv.value, 3), device="cuda")
        df = torch.empty((mf.value, 3), dtype=torch.int32, device="cuda")
        assert L.r3g_dmc_emit(ctx, dv.data_ptr(), df.data_ptr(), None, 0, None) == 0
        assert np.array_equal(f.cpu().numpy(), wf) and bits_equal(v.cpu().numpy(), wv)
        assert np.array_equal(df.cpu().numpy(), rf) and bits_equal(dv.cpu().numpy(), rv)
    finally:
        L.r3g_destroy(ctx)


def test_second_grid_size_reuses_the_workspace():
    rng = np.random.default_rng(9)
    a = rng.standard_normal((40, 41, 42)).astype(np.float32)
    b = rng.standard_normal((9, 9, 9)).astype(np.float32)
    c = rng.standard_normal((50, 50, 50)).astype(np.float32)
    want = {k: dmc_ref.dual_marching_cubes(x, 0.0)[:2] for k, x in (("a", a), ("b", b), ("c", c))}
    for k, x in (("a", a), ("b", b), ("a", a), ("c", c), ("b", b)):       # shrink, regrow, grow past the first allocation
        v, f = gpu_dmc(x, 0.0)
        assert np.array_equal(f, want[k][1]) and bits_equal(v, want[k][0]), k


def test_golden_sphere_through_the_hierarchical_decoder_gives_the_dense_mesh():
    """the extractor reads only the corners of mixed cells (the argument of DESIGN.md section 4a): the hierarchical grid,
    which holds the field's values there and parent fill elsewhere, gives the dense grid's mesh bit for bit"""
    import torch
    from r3g import dmc, hier
    vol, level = golden_volume("D")
    R = vol.shape[0] - 1
    vols = {}

    def field_fn(idx, Rl):
        if Rl not in vols:
            st = R // Rl
            vols[Rl] = dev(vol[::st, ::st, ::st]).reshape(-1)
        return vols[Rl][idx.long()]
    grid, stats = hier.decode(field_fn, R, level, 0.95)
    assert stats["levels"] == [64, 128, 256] and stats["evaluated"] < stats["dense_points"]
    assert not torch.equal(grid, dev(vol))                       # it is not the dense grid
    v, f = dmc.dual_marching_cubes(grid, level)
    dv, df = dmc.dual_marching_cubes(dev(vol), level)
    assert torch.equal(f, df) and torch.equal(v.view(torch.int32), dv.view(torch.int32))
    check_sphere("D", v.cpu().numpy(), f.cpu().numpy())


# ---- the public switches, on synthetic weights ---------------------------------------------------------------------
def _image():
    from PIL import Image
    rng = np.random.default_rng(0)
    img = np.zeros((96, 80, 4), np.uint8)
    img[20:70, 15:60, :3] = rng.integers(0, 255, (50, 45, 3))
    img[20:70, 15:60, 3] = 255
    return Image.fromarray(img, "RGBA")


def expected_pipeline_mesh(grid, level):
    n = np.array(grid.shape, np.float64)
    v, f, _ = dmc_ref.dual_marching_cubes(grid, level, True, (n - 1.0, np.ones(3), np.zeros(3)))
    return dmc_ref.upstream_frame(v, grid.shape), f


def test_pipeline_mc_algo(monkeypatch):
    import torch
    from hy3dgen.shapegen import (DegenerateFaceRemover, FaceReducer, FloaterRemover, Hunyuan3DDiTFlowMatchingPipeline)
    monkeypatch.delenv("R3G_VOLUME_DECODER", raising=False)
    pipe = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained("synthetic:mini:0", device="cuda:0")
    pil = _image()
    R = 64

    def run(**kw):
        mesh = pipe(image=pil, num_inference_steps=3, octree_resolution=R, generator=torch.manual_seed(1234567), **kw)[0]
        assert mesh is not None
        return mesh, pipe.last_grid.cpu().numpy()
    level = pipe.cfg["mc_level"]
    m_none, g_none = run()
    m_mc, g_mc = run(mc_algo="mc")
    assert np.array_equal(g_none.view(np.uint32), g_mc.view(np.uint32))
    assert np.array_equal(m_none.faces, m_mc.faces) and np.array_equal(m_none.vertices, m_mc.vertices)
    m_dmc, g_dmc = run(mc_algo="dmc")
    assert np.array_equal(g_dmc.view(np.uint32), g_mc.view(np.uint32))
    dv, df = m_dmc.device_buffers()
    wv, wf = expected_pipeline_mesh(g_dmc, level)
    assert np.array_equal(df.cpu().numpy(), wf) and bits_equal(dv.cpu().numpy(), wv)
    assert len(m_dmc.faces) != len(m_mc.faces)
    with pytest.raises(NotImplementedError):
        pipe(image=pil, num_inference_steps=3, octree_resolution=R, mc_algo="foo")
    # the attribute serves calls that pass None, through the hierarchical decoder too, and for a list of images
    pipe.mc_algo = "dmc"
    pipe.enable_flashvdm()
    m_h, g_h = run()
    assert pipe.last_hier_stats is not None
    hv, hf = m_h.device_buffers()
    wv, wf = expected_pipeline_mesh(g_h, level)
    assert np.array_equal(hf.cpu().numpy(), wf) and bits_equal(hv.cpu().numpy(), wv)
    pipe.enable_flashvdm(False)
    meshes = pipe(image=[pil, pil], num_inference_steps=3, octree_resolution=R,
                  generator=[torch.Generator().manual_seed(1234567) for _ in range(2)])
    assert len(meshes) == 2 and np.array_equal(meshes[0].faces, m_dmc.faces) and np.array_equal(meshes[0].vertices, m_dmc.vertices)
    # the cleaners run on the dmc mesh
    n0 = m_dmc.n_faces
    # (how far the edge collapse gets depends on the field: a synthetic checkpoint's may be many small closed components, each
    # of which bounds it; what is asserted is that every cleaner accepts the mesh and the collapse reduces it)
    mesh = FaceReducer()(DegenerateFaceRemover()(FloaterRemover()(m_dmc)), max_facenum=n0 // 2)
    assert 0 < mesh.n_faces < n0 and np.isfinite(mesh.vertices).all()
    assert mesh.faces.min() >= 0 and mesh.faces.max() < mesh.n_vertices


def test_stage_script_writes_glbs_with_dmc(tmp_path):
    import yaml
    sys.path.insert(0, ROOT)
    from bench import synthetic_crop
    from gltf_validate import validate_glb
    from r3g.mesh import load_glb
    inp, out = tmp_path / "prepped", tmp_path / "out"
    inp.mkdir()
    for i in range(2):
        synthetic_crop(i).save(inp / ("obj__(%d, %d).png" % (i, i)))
    cfg = {"mini": True, "num_inf_steps_hy": 5, "octree_resolution_hy": 64, "num_chunks_hy": 16000, "seed": 1234567,
           "remesh": False, "input_folder_hy": str(inp), "output_folder_hy": str(out), "use_banana": False,
           "prepped_for_hunyuan": str(tmp_path / "unused"), "jobs_per_gpu": 1, "use_all_available_cuda": False,
           "r3g_weights": "synthetic:{model}", "r3g_mc_algo": "dmc"}
    script = os.path.join(ROOT, "3d-re-gen_amd", "stage", "run.py")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")

    def stage(cfg, name):
        cfgp = tmp_path / name
        cfgp.write_text(yaml.safe_dump(cfg))
        return subprocess.run([sys.executable, script, "--config", str(cfgp)], capture_output=True, text=True, timeout=900, env=env)
    r = stage(cfg, "config.yaml")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert sorted(os.listdir(out)) == ["obj__(0, 0)", "obj__(1, 1)"]
    rep = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"stage"')][-1])
    assert rep["ok"] == 2
    for stem in os.listdir(out):
        data = (out / stem / (stem + ".glb")).read_bytes()
        got = validate_glb(data)
        m = load_glb(str(out / stem / (stem + ".glb")))
        assert len(m.faces) > 0 and np.array_equal(got["indices"].astype(np.int64), m.faces)
        assert np.isfinite(m.vertices).all()
    bad = stage(dict(cfg, r3g_mc_algo="diso", output_folder_hy=str(tmp_path / "out2")), "bad.yaml")
    assert bad.returncode != 0 and "r3g_mc_algo" in bad.stdout + bad.stderr and "mc, dmc" in bad.stdout + bad.stderr
