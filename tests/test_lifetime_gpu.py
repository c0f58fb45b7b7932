"""Lifetimes of the library's device buffers (csrc/dev_buf.h), read off the gauge r3g_get_counter("device_bytes_live"): a context
that is created, used and destroyed gives back every byte it took.  Three such cycles run in one process; the gauge after the
second and the third destroy equals its value after the first (the first cycle also warms the process-lifetime statics, which do
not go through the type, and other tests of the process may have left workspaces in the shared context).  All assertions
are exact equalities on the counter; no free-memory measurement is involved.

A cycle covers every buffer of the model (arena, modulation tables, the query-side cache, both LayerNorm folds, the fp8 weight
copies and scale vectors, the top-k selection buffers, the hierarchical decoder's grids and lists, the DiT batch arena) and one of
each state family of a context: a surface extractor's state (marching cubes), a grid in CSR form with its pair list (mesh distance,
point cloud), a plain workspace with a planner state (the hierarchical select), and the UNet's arena behind a context of its own.

Left out, each because reaching it costs another fixture: the Poisson lattices (ReconState: a cloud with normals and a solve), the
narrow-decoder tail's fragment stream (a checkpoint with a narrow geo decoder), and the UNet's condition store and skip stack
(a 2.5D reference pass / a whole-model forward)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

WIDTH, HEADS, CHUNK, R = 256, 4, 128, 8      # the smallest width with the bf16 stream, the cache, both folds and fp8; 729 points = 6 passes
CACHE_BYTES = ((R + 1) ** 3 + CHUNK - 1) // CHUNK * CHUNK * WIDTH * 2 * 2      # x0 and Q, bf16, every pass of the grid


def _cycle(torch, L, ffi, fixtures):
    from r3g import mc, model as M, unet as RU
    from switch_table import switched
    cfg, sd, usd, ucfg = fixtures
    live = lambda: ffi.counter("device_bytes_live")      # noqa: E731
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    before = live()
    gpu = M.ShapeModel(cfg, sd, 0, grid_chunk=CHUNK, private_ctx=True)
    ctx = gpu.ctx
    try:
        assert live() > before                                # the model's arena
        g = torch.Generator().manual_seed(7)
        gpu.vae_decode(torch.randn(cfg["vae"]["num_latents"], cfg["vae"]["embed_dim"], generator=g))
        with_arena = live()
        builds = ffi.counter("geo_q_cache_builds")
        plain = gpu.grid_query(1.01, R).clone()               # builds the cache; both folds
        assert ffi.counter("geo_q_cache_builds") == builds + 1 and live() >= with_arena + CACHE_BYTES
        with switched(L, ffi, geo_fp8=1):
            assert bool(torch.isfinite(gpu.grid_query(1.01, R)).all())
        with switched(L, ffi, geo_kv_topk=64):
            assert bool(torch.isfinite(gpu.grid_query(1.01, R)).all())
        with switched(L, ffi, geo_ln3_fold=0):
            assert bool(torch.isfinite(gpu.grid_query(1.01, R)).all())
        gpu.grid_query_hier(1.01, R, min_resolution=R // 2)   # two levels: the level grids, the active list and its logits
        assert torch.equal(gpu.grid_query(1.01, R), plain)    # every switch is back, and the cache still serves the same logits
        assert ffi.counter("geo_q_cache_builds") == builds + 1
        cond2 = torch.randn(2, gpu.cond_tokens, cfg["cond"]["hidden_size"], generator=g).to(torch.bfloat16)
        cond2[1] = 0
        lat = gpu.flow_sample(torch.randn(gpu.num_latents, gpu.in_channels, generator=g), cond2, 2, 5.0)      # the DiT batch arena
        assert bool(torch.isfinite(lat).all())
        held = live()
        gpu.trim()
        assert live() == held - CACHE_BYTES
        # geometry on the same private context
        idx = np.indices((9, 9, 9)).astype(np.float32) - 4
        v, f = mc.extract_mesh(torch.from_numpy(9.5 - (idx ** 2).sum(0)).cuda(), 0.0, ctx=ctx)
        assert len(v) and len(f)
        tv = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32, device="cuda")
        tf = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32, device="cuda")
        ffi.check(L.r3g_meshdist_build(ctx, ptr(tv), 4, ptr(tf), 4, 0, None, None, None, ffi.stream_ptr()))
        pts = torch.rand(64, 3, generator=g).cuda()
        ffi.check(L.r3g_cloud_build(ctx, ptr(pts), 64, 0, None, None, ffi.stream_ptr()))
        assert live() > held - CACHE_BYTES
        # one resnet block of the texture UNet, behind a context of its own
        with RU.UnetBlocks(usd, max_hw=64, max_channels=max(ucfg["block_out_channels"]), temb_dim=ucfg["temb_dim"],
                           ctx_dim=ucfg["cross_attention_dim"], ctx_tokens=ucfg["ctx_tokens"], groups=ucfg["groups"]) as unet:
            out = unet.resnet("down_blocks.0.resnets.0", torch.randn(1, 64, 8, 8, generator=g), torch.randn(1, ucfg["temb_dim"], generator=g), 64)
            assert bool(torch.isfinite(out).all())
        assert not {n: v for n, v in (("geo_fp8", 0), ("geo_kv_topk", 0), ("geo_ln3_fold", 1)) if ffi.option(n) != v}
    finally:
        torch.cuda.synchronize()
        L.r3g_destroy(ctx)
    return live()


def test_a_context_goes_with_its_events_whichever_were_made():
    """the timing events of a context (csrc/events.h) are made on first use, family by family: a context is destroyed after no use
    at all, after DBSCAN alone, after a plane fit alone and after a soft-silhouette forward without its backward, and the process
    goes on to run a call on the shared context"""
    import torch
    from r3g import cloud, ffi
    L = ffi.lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    g = torch.Generator().manual_seed(11)
    pts = torch.rand(256, 3, generator=g).cuda()
    lab = torch.zeros(256, dtype=torch.int32, device="cuda")
    triples = torch.randint(0, 256, (32, 3), generator=g).to(torch.int32).cuda()
    pos = torch.tensor([[4.0, 4.0, 1.0], [28.0, 6.0, 1.0], [10.0, 27.0, 1.0]], device="cuda")
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda")
    alpha, face = torch.empty(32, 32, device="cuda"), torch.empty(32, 32, 2, dtype=torch.int32, device="cuda")
    dist, zbuf = torch.empty(32, 32, 2, device="cuda"), torch.empty(32, 32, 2, device="cuda")
    rep, plane = (ctypes.c_int64 * 8)(), (ctypes.c_double * 16)()
    uses = {
        "none": lambda ctx: 0,
        "dbscan": lambda ctx: L.r3g_cloud_dbscan(ctx, ptr(pts), 256, 0.1, 3, 0, ptr(lab), None, rep, ffi.stream_ptr()),
        "plane": lambda ctx: L.r3g_plane_ransac(ctx, ptr(pts), 256, ptr(triples), 32, 0.05, None, None, rep, plane, ffi.stream_ptr()),
        "softras": lambda ctx: L.r3g_softras_forward(ctx, ptr(pos), 3, ptr(tri), 1, 32, 32, 2, 1.0, 4.0, ptr(alpha), ptr(face), ptr(dist),
                                                     ptr(zbuf), rep, ffi.stream_ptr()),
    }
    live = ffi.counter("device_bytes_live")
    for name, use in uses.items():
        ctx = ffi.new_context(0)
        try:
            ffi.check(use(ctx))
        finally:
            torch.cuda.synchronize()
            L.r3g_destroy(ctx)
        assert ffi.counter("device_bytes_live") == live, name
    assert float(alpha.max()) > 0.5 and int(rep[1]) == 1      # the triangle was drawn: one face used
    labels, report = cloud.dbscan(pts, 0.1, 3)               # the shared context, afterwards
    assert tuple(labels.shape) == (256,) and report["n_usable"] == 256


def test_three_create_use_destroy_cycles_leave_the_same_bytes_live():
    import torch
    from oracle import hy3d_torch as H, unet_torch as U
    from parity_support import bf16_round_matrices
    from r3g import ffi
    L = ffi.lib()
    cfg = H.tiny_config()
    cfg["vae"].update(width=WIDTH, heads=HEADS)
    sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=3))
    ucfg = U.small_config()
    usd = {k: (t.to(torch.bfloat16).float() if t.ndim >= 2 else t) for k, t in U.synthetic_state_dict(ucfg, seed=3).items()}
    after = [_cycle(torch, L, ffi, (cfg, sd, usd, ucfg)) for _ in range(3)]
    print("device_bytes_live after each destroy:", after)
    assert after[1] == after[0] and after[2] == after[0], after
