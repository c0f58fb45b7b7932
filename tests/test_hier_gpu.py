"""Hierarchical volume decoding on the GPU (include/r3g.h r3g_hier_*, r3g_grid_query_points, r3g_grid_query_hier; r3g/hier.py;
enable_flashvdm of the hy3dgen mirror) against the numpy restatement of the planner (tests/hier_ref.py), the dense decoder and the
golden marching-cubes vectors recorded from scikit-image.  Everything here is an equality of integers or of float bits: the planner
is integer work, and a listed point goes through the same launches as the same point of a dense pass."""
import hashlib
import json
import os

import numpy as np
import pytest

import hier_ref
from parity_support import bf16_round_matrices, report

pytestmark = pytest.mark.gpu


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


# ---- the planner, model-free -------------------------------------------------------------------------------------
def check_level(G, lam, beta, last, tag):
    """select / indices / merge of one level on the coarse grid G against the reference; returns the reference mask"""
    import torch
    from r3g import hier
    F = hier_ref.plan(G, lam, beta, last)
    want = hier_ref.active_indices(F)
    g = dev(G)
    count = hier.select(g, lam, beta, last)
    assert count == len(want), "%s: %d active points, the reference has %d" % (tag, count, len(want))
    idx = hier.indices(count, g.device)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want), tag
    # merge: values at the active points, the floor parent everywhere else
    vals = torch.arange(count, dtype=torch.float32, device=g.device) * 0.5 - 7.25
    fine = hier.merge(g, vals)
    n = 2 * G.shape[0] - 1
    assert tuple(fine.shape) == (n, n, n)
    Ft = torch.from_numpy(F).cuda()
    parent = dev(hier_ref.fill(np.asarray(G, np.float32), n))
    assert torch.equal(fine[Ft], vals), tag
    # (bit patterns: NaN parents must come through as they are)
    assert torch.equal(fine[~Ft].view(torch.int32), parent[~Ft].view(torch.int32)), tag
    return F


@pytest.mark.parametrize("name", hier_ref.ANALYTIC)
def test_select_and_merge_equal_the_reference_on_every_level_of_the_analytic_fields(name):
    dense, lam = hier_ref.analytic_field(name)
    at = hier_ref.strided(dense)
    L = hier_ref.levels(256)
    assert L == [64, 128, 256]
    G = np.array(at(L[0]), np.float32)
    for li in range(1, len(L)):
        F = check_level(G, lam, 0.95, li == len(L) - 1, "%s level %d" % (name, L[li]))
        N = hier_ref.fill(G, L[li] + 1)
        N[F] = at(L[li])[F]
        G = N


def test_select_and_merge_on_a_smooth_random_field():
    from mc_volumes import _smooth
    rng = np.random.default_rng(20261016)
    v = _smooth(rng, (65, 65, 65), 6)
    v = (v / np.abs(v).max() * 5).astype(np.float32)
    for beta in (0.95, 0.0):
        for last in (True, False):
            check_level(v, 0.0, beta, last, "smooth random beta=%g last=%d" % (beta, last))


def test_select_and_merge_edge_cases():
    n = 65
    I, J, K = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    clipped = (900. - ((I - 10.) ** 2 + (J - 32.) ** 2 + (K - 60.) ** 2)).astype(np.float32)     # a sphere cut by two faces of the grid
    bad = clipped.copy()
    bad[20:22, 30:35, 50:55] = np.nan
    bad[0, 0, 0], bad[5, 5, 5], bad[64, 64, 64] = np.inf, -np.inf, np.nan
    for last in (True, False):
        check_level(clipped, 0.5, 0.95, last, "clipped sphere last=%d" % last)
        check_level(bad, 0.5, 0.95, last, "NaN / inf samples last=%d" % last)
        check_level(clipped, 0.5, 0.0, last, "beta = 0 last=%d" % last)
        check_level(clipped, 0.1 + 0.2, 0.3, last, "a level that is no float last=%d" % last)
        for nc in (2, 3):
            G = np.full((nc, nc, nc), -1, np.float32)
            G[0, 0, 0] = 1
            check_level(G, 0.0, 0.95, last, "n_coarse=%d last=%d" % (nc, last))
            check_level(-G, 0.0, 0.0, last, "n_coarse=%d inverted last=%d" % (nc, last))
    # one word exactly full / straddling: 64 | n^3 never holds for odd n, so the last word is always partial; 33^3 -> 65^3
    check_level(np.zeros((33, 33, 33), np.float32), 0.0, 0.95, True, "all band")


def test_a_field_without_a_candidate_is_pure_parent_fill_and_has_no_surface():
    import torch
    from r3g import ffi, hier, mc
    G = np.full((33, 33, 33), 7.0, np.float32)
    for last in (True, False):
        F = check_level(G, 0.0, 0.95, last, "constant field")
        assert F.sum() == 0
    g = dev(G)
    assert hier.select(g, 0.0) == 0
    fine = hier.merge(g, torch.empty(0, device=g.device))
    assert torch.equal(fine, torch.full((65, 65, 65), 7.0, device=g.device))
    grid, stats = hier.decode(lambda idx, R: torch.full((idx.numel(),), 7.0, device="cuda"), 128, 0.0)
    assert stats["evaluated_per_level"] == [65 ** 3, 0] and torch.equal(grid, torch.full((129, 129, 129), 7.0, device="cuda"))
    with pytest.raises((ffi.LevelRangeError, ffi.NoSurfaceError)) as dense_err:      # what the dense grid of this field raises today
        mc.marching_cubes(dev(np.full((129, 129, 129), 7.0, np.float32)), 0.0)
    with pytest.raises((ffi.LevelRangeError, ffi.NoSurfaceError)) as hier_err:
        mc.marching_cubes(grid, 0.0)
    assert hier_err.type is dense_err.type and str(hier_err.value) == str(dense_err.value)


def test_call_order_and_arguments_are_checked():
    import ctypes
    import torch
    from r3g import ffi
    L = ffi.lib()
    ctx = ffi.new_context(0)
    try:
        out = torch.zeros(27, dtype=torch.int32, device="cuda")
        assert L.r3g_hier_indices(ctx, out.data_ptr(), None) == -4           # R3G_ERR_STATE: no select yet
        g = torch.zeros((1, 1, 1), device="cuda")
        n = ctypes.c_int64()
        assert L.r3g_hier_select(ctx, g.data_ptr(), 1, 0.0, 0.95, 1, ctypes.byref(n), None) == -1
        assert L.r3g_hier_select(ctx, g.data_ptr(), 646, 0.0, 0.95, 1, ctypes.byref(n), None) == -1
        g = torch.zeros((2, 2, 2), device="cuda")
        assert L.r3g_hier_select(ctx, g.data_ptr(), 2, 0.0, -1.0, 1, ctypes.byref(n), None) == -1
        assert L.r3g_hier_merge(ctx, g.data_ptr(), None, out.data_ptr(), None) == -4
    finally:
        L.r3g_destroy(ctx)


# ---- pinned to the real scikit-image -------------------------------------------------------------------------------
def decode_volume(dense, lam, beta=0.95):
    import torch
    from r3g import hier
    R = dense.shape[0] - 1
    vols = {}

    def field_fn(idx, Rl):
        if Rl not in vols:
            st = R // Rl
            vols[Rl] = dev(dense[::st, ::st, ::st]).reshape(-1)
        return vols[Rl][idx.long()]
    return hier.decode(field_fn, R, lam, beta)


def test_golden_sphere_through_the_hierarchical_decoder_gives_the_scikit_image_mesh(golden_dir):
    from mc_volumes import golden_volume
    from r3g import mc
    with open(os.path.join(golden_dir, "mc_sha.json")) as f:
        g = json.load(f)["D"]
    vol, level = golden_volume("D")
    grid, stats = decode_volume(vol, level)
    _, _, per_level = hier_ref.hier(hier_ref.strided(vol), 256, level, 0.95)
    assert stats["levels"] == [64, 128, 256] and stats["evaluated_per_level"] == per_level
    report("hier: golden D sphere, evaluated share of 257^3 (reported)", stats["evaluated"] / stats["dense_points"], 1.0)
    v, f = mc.marching_cubes(grid, level)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert (len(v), len(f), sha(f), sha(v)) == (g["V"], g["F"], g["faces_sha"], g["verts_sha"])


@pytest.mark.parametrize("name", hier_ref.ANALYTIC[1:])
def test_analytic_fields_through_the_hierarchical_decoder_give_the_dense_mesh(name):
    import torch
    from r3g import mc
    dense, lam = hier_ref.analytic_field(name)
    grid, stats = decode_volume(dense, lam)
    G, F, per_level = hier_ref.hier(hier_ref.strided(dense), 256, lam, 0.95)
    assert stats["evaluated_per_level"] == per_level
    assert torch.equal(grid.view(torch.int32), dev(G).view(torch.int32))
    report("hier: %s, evaluated share of 257^3 (reported)" % name, stats["evaluated"] / stats["dense_points"], 1.0)
    v, f = mc.marching_cubes(grid, lam)
    dv, df = mc.marching_cubes(dev(dense), lam)
    assert torch.equal(f, df) and torch.equal(v.view(torch.int32), dv.view(torch.int32))


# ---- the geo decoder at listed points ------------------------------------------------------------------------------
class Setup:
    def __init__(self, cfg, seed, grid_chunk, edit=None):
        from oracle import hy3d_torch as H
        from r3g import model as M
        self.cfg = cfg
        self.sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=seed))
        if edit is not None:
            edit(self.sd)
        self.chunk = grid_chunk if grid_chunk else 131072
        self.gpu = M.ShapeModel(cfg, self.sd, 0, grid_chunk=grid_chunk)

    def decode_latents(self, seed):
        import torch
        lat = torch.randn(self.cfg["vae"]["num_latents"], self.cfg["vae"]["embed_dim"], generator=torch.Generator().manual_seed(seed))
        self.gpu.vae_decode(lat)


def _tiny_cfg():
    from oracle import hy3d_torch as H
    return H.tiny_config()


def _wide_cfg():
    from oracle import hy3d_torch as H
    return H.wide_config(depth=1, depth_single=1, vae_layers=1, cond_layers=1)


@pytest.fixture(scope="module")
def tiny():
    return Setup(_tiny_cfg(), 3, 4096)


@pytest.fixture(scope="module")
def tiny_default_pass():
    return Setup(_tiny_cfg(), 3, 0)


@pytest.fixture(scope="module")
def wide():
    return Setup(_wide_cfg(), 11, 4096)


@pytest.fixture(scope="module")
def wide_default_pass():
    return Setup(_wide_cfg(), 11, 0)


def listed_points_equal_dense(s, R, tag):
    import torch
    from r3g import ffi
    L = ffi.lib()
    total = (R + 1) ** 3
    two_and_a_bit = 2 * s.chunk + 777
    assert total > two_and_a_bit
    g = torch.Generator().manual_seed(R * 1000 + s.chunk)
    lists = {
        "contiguous run": torch.arange(1000, 1000 + 777),
        "about 3000 ascending": torch.sort(torch.randperm(total, generator=g)[:3001]).values,
        "two full passes + 777 ascending": torch.sort(torch.randperm(total, generator=g)[:two_and_a_bit]).values,
        "unsorted with repeats": torch.randint(0, total, (1500,), generator=g),
        "first and last point": torch.tensor([0, total - 1]),
    }
    s.decode_latents(7)
    try:
        for lnd in (1, 0):
            for ln3 in (1, 0):
                ffi.check(L.r3g_set_option(b"geo_lnd_fused", lnd))
                ffi.check(L.r3g_set_option(b"geo_ln3_fold", ln3))
                dense = s.gpu.grid_query(1.01, R).reshape(-1).clone()
                for name, idx in lists.items():
                    got = s.gpu.grid_query_points(1.01, R, idx.to(torch.int32).cuda())
                    want = dense[idx.cuda()]
                    same = torch.equal(got.view(torch.int32), want.view(torch.int32))
                    assert same, "%s, %s, geo_lnd_fused=%d geo_ln3_fold=%d: %d of %d logits differ from the dense grid's" % (
                        tag, name, lnd, ln3, int((got.view(torch.int32) != want.view(torch.int32)).sum()), idx.numel())
                assert s.gpu.grid_query_points(1.01, R, torch.empty(0, dtype=torch.int32)).numel() == 0
    finally:
        ffi.check(L.r3g_set_option(b"geo_lnd_fused", 1))
        ffi.check(L.r3g_set_option(b"geo_ln3_fold", 1))


def test_listed_points_equal_the_dense_grid_tiny(tiny):
    listed_points_equal_dense(tiny, 40, "tiny, passes of 4096")


def test_listed_points_equal_the_dense_grid_tiny_default_pass(tiny_default_pass):
    listed_points_equal_dense(tiny_default_pass, 64, "tiny, passes of 131072")


def test_listed_points_equal_the_dense_grid_wide(wide):
    listed_points_equal_dense(wide, 40, "wide, passes of 4096")


def test_listed_points_equal_the_dense_grid_wide_default_pass(wide_default_pass):
    listed_points_equal_dense(wide_default_pass, 64, "wide, passes of 131072")


def test_listed_points_are_refused_in_fp8_mode_and_out_of_order_calls_fail(wide):
    import torch
    from r3g import ffi
    L = ffi.lib()
    wide.decode_latents(7)
    idx = torch.arange(10, dtype=torch.int32).cuda()
    try:
        ffi.check(L.r3g_set_option(b"geo_fp8", 1))
        with pytest.raises(ffi.R3GError):
            wide.gpu.grid_query_points(1.01, 16, idx)
        with pytest.raises(ffi.R3GError):
            wide.gpu.grid_query_hier(1.01, 128)
    finally:
        ffi.check(L.r3g_set_option(b"geo_fp8", 0))
    assert wide.gpu.grid_query_points(1.01, 16, idx).numel() == 10


@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_the_query_side_cache_survives_a_hierarchical_decode(which):
    """dense (builds the cache), hierarchical, dense: the third equals the first and the cache was not allocated again.  The cache
    exists for the bf16 residual stream only (width % 256 == 0): `tiny` (width 128) never has one, and its counter must not move at
    all; `wide` builds it with the first dense query."""
    import torch
    from r3g import ffi
    s = Setup(_tiny_cfg(), 3, 4096) if which == "tiny" else Setup(_wide_cfg(), 11, 4096)
    has_cache = s.cfg["vae"]["width"] % 256 == 0
    s.decode_latents(18)
    R = 40
    builds0 = ffi.counter("geo_q_cache_builds")
    first = s.gpu.grid_query(1.01, R).clone()
    built = ffi.counter("geo_q_cache_builds")
    assert built == builds0 + (1 if has_cache else 0)
    grid, stats = s.gpu.grid_query_hier(1.01, R, 0.0, 0.95, min_resolution=10)
    assert stats["levels"] == [10, 20, 40] and stats["dense_points"] == 41 ** 3
    assert ffi.counter("geo_q_cache_builds") == built
    third = s.gpu.grid_query(1.01, R)
    assert torch.equal(third, first)
    assert ffi.counter("geo_q_cache_builds") == built
    # and a dense query of another resolution does rebuild it (the counter sees what it is meant to see)
    s.gpu.grid_query(1.01, 20)
    assert ffi.counter("geo_q_cache_builds") == built + (1 if has_cache else 0)
    # the hierarchical grid itself: every evaluated point of the finest level is the dense value
    at = {Rl: s.gpu.grid_query(1.01, Rl).cpu().numpy() for Rl in stats["levels"]}
    G, F, per_level = hier_ref.hier(lambda Rl: at[Rl], R, 0.0, 0.95, min_res=10)
    assert stats["evaluated_per_level"] == per_level
    assert np.array_equal(grid.cpu().numpy().view(np.uint32), G.view(np.uint32))
    assert np.array_equal(grid.cpu().numpy()[F], at[R][F])


# ---- the model's field, end to end -----------------------------------------------------------------------------------
def object_like(sd):
    # FourierEmbedder layout [x y z | sin(e) 24 | cos(e) 24], e = coordinate-major x 8 frequencies 2^k: keep k <= 1
    # (the recipe of tests/test_cfg4_gpu.py)
    w = sd["vae.geo_decoder.query_proj.weight"].clone()
    for c in range(3):
        for k in range(2, 8):
            w[:, 3 + c * 8 + k] = 0
            w[:, 27 + c * 8 + k] = 0
    sd["vae.geo_decoder.query_proj.weight"] = w


@pytest.mark.parametrize("field", ["object-like", "noise-like"])
@pytest.mark.parametrize("R", [128, 256])
def test_model_field_end_to_end(field, R):
    """The hierarchical grid of the geo decoder's own field against the dense one: every point the finest level evaluated holds the
    dense value, the whole grid equals the reference planner's run on the dense grids of the levels, the library's unsafe-cell count
    equals the reference's, and where no cell is missed or unsafe the two meshes are identical arrays.  Evaluated share, missed and
    unsafe cells are reported (missed cells on synthetic weights are a property of the field)."""
    import torch
    from r3g import ffi, hier, mc
    L = ffi.lib()
    s = Setup(_wide_cfg(), 11, 0, object_like if field == "object-like" else None)
    s.decode_latents(21)
    lv = hier_ref.levels(R)
    try:
        ffi.check(L.r3g_set_option(b"geo_q_cache", 0))        # three resolutions in a row: no 68 GB cache per resolution
        at = {Rl: s.gpu.grid_query(1.01, Rl).cpu().numpy() for Rl in lv}
    finally:
        ffi.check(L.r3g_set_option(b"geo_q_cache", 1))
    dense = at[R]
    dv, df = mc.marching_cubes(dev(dense), 0.0)
    for beta, btag in ((0.95, "0.95"), (0.05 * float(np.abs(at[lv[0]]).max()), "0.05 max|coarse logit|")):
        grid, stats = s.gpu.grid_query_hier(1.01, R, 0.0, beta)
        G, F, per_level = hier_ref.hier(lambda Rl: at[Rl], R, 0.0, beta)
        assert stats["levels"] == lv and stats["evaluated_per_level"] == per_level
        g = grid.cpu().numpy()
        assert np.array_equal(g[F].view(np.uint32), dense[F].view(np.uint32)), "an evaluated point differs from the dense grid"
        assert np.array_equal(g.view(np.uint32), G.view(np.uint32))
        # the model-free route with the decoder as its field is the same computation
        grid2, stats2 = hier.decode(lambda idx, Rl: s.gpu.grid_query_points(1.01, Rl, idx), R, 0.0, beta)
        assert torch.equal(grid2.view(torch.int32), grid.view(torch.int32)) and stats2["evaluated_per_level"] == per_level
        missed, unsafe = hier_ref.missed_and_unsafe(dense, G, F, 0.0)
        assert stats["unsafe_cells"] == unsafe
        tag = "hier: wide %s field, R=%d, band %s: " % (field, R, btag)
        report(tag + "evaluated share (reported)", stats["evaluated"] / stats["dense_points"], 1.0)
        report(tag + "missed cells (reported)", missed, 1e18)
        report(tag + "unsafe cells (reported)", unsafe, 1e18)
        print("%sshare %.4f missed %d unsafe %d" % (tag, stats["evaluated"] / stats["dense_points"], missed, unsafe))
        if missed == 0 and unsafe == 0:
            v, f = mc.marching_cubes(grid, 0.0)
            assert torch.equal(f, df) and torch.equal(v.view(torch.int32), dv.view(torch.int32))
    del s
    torch.cuda.empty_cache()


# ---- the public switch ---------------------------------------------------------------------------------------------
def test_pipeline_enable_flashvdm(monkeypatch):
    import torch
    from PIL import Image
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    monkeypatch.delenv("R3G_VOLUME_DECODER", raising=False)
    pipe = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained("synthetic:mini:0", device="cuda:0")
    rng = np.random.default_rng(0)
    img = np.zeros((96, 80, 4), np.uint8)
    img[20:70, 15:60, :3] = rng.integers(0, 255, (50, 45, 3))
    img[20:70, 15:60, 3] = 255
    pil = Image.fromarray(img, "RGBA")
    R = 128

    def run():
        mesh = pipe(image=pil, num_inference_steps=3, octree_resolution=R, generator=torch.manual_seed(1234567))[0]
        assert mesh is not None
        return np.array(mesh.vertices), np.array(mesh.faces), pipe.last_grid.clone()
    v0, f0, g0 = run()                                             # never enabled
    assert pipe.last_hier_stats is None and pipe.timings["grid_points_evaluated"] == (R + 1) ** 3
    pipe.enable_flashvdm()
    v1, f1, g1 = run()
    st = pipe.last_hier_stats
    assert tuple(g1.shape) == (R + 1,) * 3 and len(f1) > 0
    assert st["levels"] == hier_ref.levels(R) == [64, 128] and st["dense_points"] == (R + 1) ** 3
    # No level evaluates more than its own lattice; for the finest that is "evaluated <= dense_points".  (The SUM over the levels
    # also counts the 65^3 points of level 0: on a field that is all band -- a synthetic checkpoint's at band 0.95 may be -- it is
    # dense_points + 65^3, so the sum is reported, not bounded.)
    assert st["evaluated_per_level"][0] == 65 ** 3 and 0 < st["evaluated_per_level"][1] <= st["dense_points"]
    assert st["evaluated"] == sum(st["evaluated_per_level"])
    assert pipe.timings["grid_points_evaluated"] == st["evaluated"]
    report("hier: synthetic:mini pipeline, R=128, band 0.95: evaluated share (reported)", st["evaluated"] / st["dense_points"], 2.0)
    pipe.enable_flashvdm(False)
    v2, f2, g2 = run()
    assert pipe.last_hier_stats is None
    assert torch.equal(g2.view(torch.int32), g0.view(torch.int32))
    assert np.array_equal(f2, f0) and np.array_equal(v2, v0)
    # a list of images goes through the same helper
    pipe.enable_flashvdm()
    meshes = pipe(image=[pil, pil], num_inference_steps=3, octree_resolution=R,
                  generator=[torch.Generator().manual_seed(1234567) for _ in range(2)])
    assert len(meshes) == 2 and pipe.last_hier_stats["levels"] == [64, 128]
    assert np.array_equal(np.array(meshes[0].faces), f1) and np.array_equal(np.array(meshes[0].vertices), v1)
