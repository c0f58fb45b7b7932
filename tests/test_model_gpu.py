"""GPU parity of the DiT / VAE / geo-decoder / conditioner paths (through the C ABI) against the
PyTorch-CPU fp32 restatement oracle/hy3d_torch.py on identical seeded synthetic weights.

The checkpoint (weights) is bf16-representable on both sides (matrices are rounded to bf16 once, as a real
bf16 checkpoint would be), so the differences measured here are kernel arithmetic only:
bf16 GEMM operands / fp32 accumulation / fp32 residual stream.  The checkpoint is the "unit" one of
oracle.hy3d_torch.synthetic_state_dict: every branch contributes O(1) to its residual stream, so that a wiring error
inside a block is far outside the tolerances.  Tolerances live in tests/parity_support.py (TOL) and
tests/test_mutation_cpu.py proves, hazard by hazard, that a mis-wired block moves the same metric by >= 5x of them.
Measured values are reported in the pytest terminal summary (tests/conftest.py).
"""
import numpy as np
import pytest

from parity_support import TOL, bf16_round_matrices, rel_l2, report

pytestmark = pytest.mark.gpu


class Setup:
    def __init__(self, cfg, seed):
        import torch
        from oracle import hy3d_torch as H
        from r3g import model as M
        torch.manual_seed(0)
        self.cfg = cfg
        self.sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=seed))
        self.oracle = H.load_state_dict(H.ShapePipeline(cfg), self.sd)
        self.gpu = M.ShapeModel(cfg, self.sd, 0, grid_chunk=4096)
        self.H = H


@pytest.fixture(scope="module")
def tiny():
    from oracle import hy3d_torch as H
    return Setup(H.tiny_config(), 3)


def _inputs(s, seed=0):
    from parity_support import dit_inputs
    return dit_inputs(s.cfg, seed)


def _block_deltas(s, x, t, cond, tag):
    """For every block k: the GPU's branch contribution stream_{k+1} - stream_k against the oracle block applied to the
    GPU's OWN stream_k (so the comparison isolates block k; nothing accumulated upstream of it enters)."""
    import torch
    import parity_support as P
    m = s.oracle.model
    nd, ns = len(m.double_blocks), len(m.single_blocks)
    B, n_cond = x.shape[0], cond.shape[1]
    _, _, vec = P.dit_prologue(m, x, t, cond)
    streams = []
    for k in range(nd + ns + 1):
        s.gpu.dit_forward(x, t, cond, min(k, nd), max(0, k - nd))
        streams.append(s.gpu.dit_stream(B).cpu())
    worst = 0.0
    for k in range(nd + ns):
        ref = P.dit_block_apply(m, k, streams[k], vec, n_cond) - streams[k]
        got = streams[k + 1] - streams[k]
        assert torch.isfinite(got).all()
        err = P.block_delta_error(got, ref, n_cond, k < nd)
        # branch contributions are O(1) of the stream: a near-identity block could not pass by accident
        assert float(ref.norm() / streams[k].norm()) > 0.1
        report("%s block %2d delta" % (tag, k), err, TOL["block_delta"])
        worst = max(worst, err)
    return worst


def test_dit_block_deltas_tiny(tiny):
    x, t, cond = _inputs(tiny)
    assert _block_deltas(tiny, x, t, cond, "tiny") <= TOL["block_delta"]


def test_dit_block_deltas_small_q():
    """the q/k RMSNorm eps (1e-6): a first-order term only when mean(q^2) ~ eps.  Same blocks on the checkpoint whose
    q / k rows are scaled by 1e-3 (tests/test_mutation_cpu.py::test_qk_norm_eps_needs_small_q: eps 1e-5, 1e-7 or 0
    would move these contributions by >= 5x the tolerance)."""
    import parity_support as P
    from oracle import hy3d_torch as H
    s = Setup.__new__(Setup)
    from r3g import model as M
    s.cfg = H.tiny_config()
    s.sd = P.small_qk_state_dict(bf16_round_matrices(H.synthetic_state_dict(s.cfg, seed=3)), s.cfg)
    s.oracle = H.load_state_dict(H.ShapePipeline(s.cfg), s.sd)
    s.gpu = M.ShapeModel(s.cfg, s.sd, 0, grid_chunk=4096)
    x, t, cond = P.dit_inputs(s.cfg, 0)
    assert _block_deltas(s, x, t, cond, "small-q") <= TOL["block_delta"]


def test_conditioner_tokens(tiny):
    import torch
    g = torch.Generator().manual_seed(1)
    S = tiny.cfg["cond"]["image_size"]
    img = torch.randn(3, S, S, generator=g)
    ref = tiny.oracle.conditioner.main_image_encoder.model(img[None]).last_hidden_state[0]
    out = tiny.gpu.cond_encode(img)
    err = rel_l2(out.float(), ref)
    report("tiny conditioner tokens", err, TOL["conditioner"])
    assert err <= TOL["conditioner"]


@pytest.mark.parametrize("nd,ns", [(0, 0), (1, 0), (2, 0), (2, 1), (-1, -1)])
def test_dit_forward_blocks(tiny, nd, ns):
    import torch
    x, t, cond = _inputs(tiny)
    with torch.no_grad():
        ref = tiny.oracle.model(x, t, cond, n_double=None if nd < 0 else nd, n_single=None if ns < 0 else ns)
    out = tiny.gpu.dit_forward(x, t, cond, nd, ns)
    assert torch.isfinite(out).all()
    err = rel_l2(out, ref)
    report("tiny dit forward nd=%d ns=%d" % (nd, ns), err, TOL["dit_forward_tiny"])
    assert err <= TOL["dit_forward_tiny"]


def test_fp16_checkpoint_is_rounded_to_bf16_and_what_that_costs():
    """Upstream ships fp16 weights (model.fp16.safetensors); this build stores matrices in bf16, i.e. RE-ROUNDS them (3 mantissa
    bits less).  Every other parity test pre-rounds the synthetic checkpoint to bf16 on both sides and therefore cannot see
    that step.  Here the oracle keeps the fp16 values: the extra error of the ingest rounding is measured and bounded."""
    import torch
    from oracle import hy3d_torch as H
    from r3g import model as M
    from parity_support import dit_inputs
    cfg = H.tiny_config()
    sd16 = {k: (v.to(torch.float16).to(torch.float32) if torch.is_floating_point(v) and v.ndim >= 2 else v.clone())
            for k, v in H.synthetic_state_dict(cfg, seed=31).items()}
    oracle16 = H.load_state_dict(H.ShapePipeline(cfg), sd16)
    gpu = M.ShapeModel(cfg, sd16, 0, grid_chunk=4096)           # the loader rounds the fp16-valued matrices to bf16
    oracle_b = H.load_state_dict(H.ShapePipeline(cfg), bf16_round_matrices(sd16))
    x, t, cond = dit_inputs(cfg, 7)
    with torch.no_grad():
        ref16 = oracle16.model(x, t, cond)
        refb = oracle_b.model(x, t, cond)
    out = gpu.dit_forward(x, t, cond)
    e_same = rel_l2(out, refb)          # against the same (bf16-rounded) weights: the usual kernel error
    e_fp16 = rel_l2(out, ref16)         # against the checkpoint as shipped: kernel error + weight re-rounding
    report("tiny dit forward, fp16 checkpoint: vs oracle on the bf16-rounded weights", e_same, TOL["dit_forward_tiny"])
    report("tiny dit forward, fp16 checkpoint: vs oracle on the fp16 weights as shipped", e_fp16, 2 * TOL["dit_forward_tiny"])
    assert e_same <= TOL["dit_forward_tiny"] and e_fp16 <= 2 * TOL["dit_forward_tiny"]
    assert e_fp16 > e_same              # the re-rounding is visible, not hidden


def test_dit_forward_batch1(tiny):
    import torch
    x, t, cond = _inputs(tiny, 4)
    with torch.no_grad():
        ref = tiny.oracle.model(x[:1], t[:1], cond[:1])
    assert rel_l2(tiny.gpu.dit_forward(x[:1], t[:1], cond[:1]), ref) <= TOL["dit_forward_tiny"]


def test_flow_sample_matches_restated_scheduler(tiny):
    import torch
    x, _, cond = _inputs(tiny, 2)
    lat0 = x[0]
    steps, g = 6, 5.0
    trace = []
    ref = tiny.oracle.sample(cond, lat0[None].clone(), steps, g, trace=trace)[0]
    out = tiny.gpu.flow_sample(lat0.clone(), cond, steps, g)
    err = rel_l2(out, ref)
    report("tiny flow_sample 6 steps", err, TOL["flow_sample"])
    assert err <= TOL["flow_sample"]
    # the last Euler step has d_sigma = 0 (sigmas = linspace(0,1,N) + trailing 1), upstream quirk
    assert torch.equal(trace[-1], trace[-2])


def _fifty_steps(s, tag, seed):
    """50 Euler steps x CFG 2 (the reference's num_inf_steps_hy, src/config.yaml) against the oracle's sampler: the stated
    SURVEY 8(c) tolerance for 50-step latents is 3e-2 rel-L2"""
    import torch
    x, _, cond = _inputs(s, seed)
    lat0 = x[0]
    ref = s.oracle.sample(cond, lat0[None].clone(), 50, 5.0)[0]
    out = s.gpu.flow_sample(lat0.clone(), cond, 50, 5.0)
    assert torch.isfinite(out).all()
    err = rel_l2(out, ref)
    report("%s flow_sample 50 steps x CFG (guidance 5)" % tag, err, TOL["flow_sample_50"])
    return err, out, lat0, cond


def test_flow_sample_fifty_steps_tiny(tiny):
    err, out, lat0, cond = _fifty_steps(tiny, "tiny", 31)
    assert err <= TOL["flow_sample_50"]
    # the sampler moved the latents by O(1): the tolerance is not met by standing still
    assert rel_l2(out, lat0) > 0.3


def test_flow_sample_fifty_steps_mini_dims():
    """hunyuan3d-dit-v2-mini's widths and token counts (hidden 1024, 16 heads, 512 latents + 1370 context tokens), 50 steps x
    CFG 2.  Depth 1 + 2 instead of the model's 8 + 16: the fp32 oracle runs the same 50 steps on the box's host cores, and at
    full depth that alone took 9 minutes of a GPU lease (measured once, round 3: 2.9e-3 at 8 + 16 blocks, tolerance 3e-2;
    profiles/r03_parity_measured.json).  Every block at full depth is covered by test_full_depth_dit_forward."""
    from oracle import hy3d_torch as H
    cfg = H.mini_config()
    cfg["dit"].update(depth=1, depth_single_blocks=2)
    cfg["vae"].update(num_decoder_layers=1)
    cfg["cond"].update(num_hidden_layers=1)
    s = Setup(cfg, 41)
    err, out, lat0, _ = _fifty_steps(s, "mini-dims (depth 1+2)", 5)
    assert err <= TOL["flow_sample_50"]
    assert rel_l2(out, lat0) > 0.3


def test_fifty_steps_full_width_dedup_against_plain_batch(wide):
    """50 steps at full width (4442 tokens, depth 1 + 1): the de-duplicated CFG batch against the plain one -- two valid
    bf16 evaluations of the same sampler.  (Both against the 50-step fp32 oracle at this width: 2.06e-3 / 2.07e-3, measured
    once in round 3 -- 70 s of host time per run, so the oracle leg runs at 8 steps here.)"""
    import torch
    from r3g import ffi
    L = ffi.lib()
    x, _, cond = _inputs(wide, 15)
    lat0 = x[0]
    outs = {}
    for steps in (50, 8):
        a = wide.gpu.flow_sample(lat0.clone(), cond, steps, 5.0).clone()
        try:
            ffi.check(L.r3g_set_option(b"cfg_dedup", 0))
            b = wide.gpu.flow_sample(lat0.clone(), cond, steps, 5.0).clone()
        finally:
            ffi.check(L.r3g_set_option(b"cfg_dedup", 1))
        outs[steps] = (a, b)
        report("full-width %d steps: cfg dedup vs plain batch" % steps, rel_l2(a, b), TOL["same_function"])
        assert torch.isfinite(a).all() and rel_l2(a, b) <= TOL["same_function"]
    ref = wide.oracle.sample(cond, lat0[None].clone(), 8, 5.0)[0]
    ea, eb = rel_l2(outs[8][0], ref), rel_l2(outs[8][1], ref)
    report("full-width 1+1 flow_sample 8 steps (dedup)", ea, TOL["flow_sample"])
    report("full-width 1+1 flow_sample 8 steps (plain batch)", eb, TOL["flow_sample"])
    assert ea <= TOL["flow_sample"] and eb <= TOL["flow_sample"]


def test_skipping_the_zero_step_changes_nothing(tiny):
    """upstream's last step has d_sigma = 0; its DiT evaluation is skipped by default (x += 0 * v)"""
    import torch
    from r3g import ffi
    L = ffi.lib()
    x, _, cond = _inputs(tiny, 8)
    a = tiny.gpu.flow_sample(x[0].clone(), cond, 7, 5.0).clone()
    try:
        ffi.check(L.r3g_set_option(b"skip_zero_step", 0))
        b = tiny.gpu.flow_sample(x[0].clone(), cond, 7, 5.0).clone()
        ffi.check(L.r3g_set_option(b"cfg_dedup", 0))
        c = tiny.gpu.flow_sample(x[0].clone(), cond, 7, 5.0).clone()
        ffi.check(L.r3g_set_option(b"skip_zero_step", 1))
        d = tiny.gpu.flow_sample(x[0].clone(), cond, 7, 5.0).clone()
    finally:
        ffi.check(L.r3g_set_option(b"skip_zero_step", 1))
        ffi.check(L.r3g_set_option(b"cfg_dedup", 1))
    assert torch.equal(a, b) and torch.equal(c, d)


def _batch_inputs(s, n, seed):
    import torch
    from parity_support import dit_inputs
    lats, conds = [], []
    for o in range(n):
        x, _, cond = dit_inputs(s.cfg, seed + 7 * o)
        lats.append(x[0])
        conds.append(cond)
    return torch.stack(lats), torch.stack(conds).to(torch.bfloat16)


@pytest.mark.parametrize("which,n", [("tiny", 2), ("tiny", 3), ("tiny", 4), ("tiny", 5), ("wide", 2), ("wide", 4)])
def test_objects_sharing_a_launch_get_bit_identical_results(which, n, tiny, wide):
    """r3g_flow_sample_batch: n objects go through every DiT layer in one launch (more rows: the full-width GEMMs move from
    128x128 to 256x256 tiles, the attention grid gets 2n entries, 5 objects = a launch of 4 and one of 1).  A row does
    not know its neighbours: each object's latents must equal its single-object run BIT FOR BIT."""
    import torch
    st = tiny if which == "tiny" else wide
    lat, cond = _batch_inputs(st, n, 100)
    steps = 3 if which == "tiny" else 2
    single = [st.gpu.flow_sample(lat[o].clone(), cond[o], steps, 5.0).clone() for o in range(n)]
    both = st.gpu.flow_sample_batch(lat.clone(), cond, steps, 5.0)
    assert not torch.equal(single[0], single[1])
    for o in range(n):
        assert torch.equal(both[o], single[o]), "object %d of %d differs: max |d| %.3e" % (
            o, n, float((both[o] - single[o]).abs().max()))
    # and against the oracle, object 1 (the batch path is the one under test)
    ref = st.oracle.sample(cond[1].float(), lat[1][None].clone(), steps, 5.0)[0]
    assert rel_l2(both[1], ref) <= TOL["flow_sample"]
    # plain (non-dedup) contexts: the batch entry point falls back to one object after the other
    cond_nu = cond.clone()
    cond_nu[:, 1] = torch.randn_like(cond_nu[:, 1].float()).to(torch.bfloat16)
    if which == "tiny":
        c = st.gpu.flow_sample_batch(lat.clone(), cond_nu, 2, 2.0)
        for o in range(n):
            assert torch.equal(c[o], st.gpu.flow_sample(lat[o].clone(), cond_nu[o], 2, 2.0))


def test_linear1_as_one_persistent_launch_and_sliced_epilogues_are_bit_identical(wide):
    """Round 6: at four objects per launch a single block's [fused QKV | MLP-in + GELU] runs as ONE persistent launch of the phased
    kernel (option gemm_mixed; the QKV tiles' epilogue on the persistent kernel, in 64-row passes through the wave's slices of the
    idle k-tile buffer: option gemm_epi_slices).  Same tiles, same k order: every combination of the two options gives the same bits."""
    import torch
    from r3g import ffi
    L = ffi.lib()
    lat, cond = _batch_inputs(wide, 4, 300)
    names = ("gemm_mixed", "gemm_phased_persistent", "gemm_phased")
    c0 = {n: ffi.counter(n) for n in names}
    want = wide.gpu.flow_sample_batch(lat.clone(), cond, 2, 5.0).clone()
    c1 = {n: ffi.counter(n) for n in names}
    # the bits are the same either way, so the launch counters say which form ran: by default the single block's linear1 is the mixed
    # launch and the double block's QKV pair a persistent one
    assert c1["gemm_mixed"] > c0["gemm_mixed"] and c1["gemm_phased_persistent"] > c0["gemm_phased_persistent"]
    base_phased = c1["gemm_phased"] - c0["gemm_phased"]
    try:
        for mixed, slices, pqkv in ((0, 1, 1), (1, 0, 1), (0, 0, 1), (1, 1, 0), (0, 0, 0)):
            ffi.check(L.r3g_set_option(b"gemm_mixed", mixed))
            ffi.check(L.r3g_set_option(b"gemm_epi_slices", slices))
            ffi.check(L.r3g_set_option(b"gemm_persistent_qkv", pqkv))       # the double blocks' QKV pair on the persistent kernel
            c0 = {n: ffi.counter(n) for n in names}
            got = wide.gpu.flow_sample_batch(lat.clone(), cond, 2, 5.0)
            c1 = {n: ffi.counter(n) for n in names}
            assert torch.equal(got, want), "gemm_mixed=%d gemm_epi_slices=%d gemm_persistent_qkv=%d: max |d| %.3e" % (
                mixed, slices, pqkv, float((got - want).abs().max()))
            # the mixed launch needs both switches (its QKV half IS a persistent fused-QKV launch) ...
            assert (c1["gemm_mixed"] > c0["gemm_mixed"]) == bool(mixed and pqkv), (mixed, slices, pqkv)
            # ... and without gemm_persistent_qkv every fused-QKV launch leaves the persistent kernel for the one-tile-per-workgroup form
            if not pqkv:
                assert c1["gemm_phased"] - c0["gemm_phased"] > base_phased, (mixed, slices, pqkv)
    finally:
        ffi.check(L.r3g_set_option(b"gemm_mixed", 1))
        ffi.check(L.r3g_set_option(b"gemm_epi_slices", 1))
        ffi.check(L.r3g_set_option(b"gemm_persistent_qkv", 1))
    for _ in range(2):                                   # stable from run to run (an LDS hazard would show as rare diffs)
        assert torch.equal(wide.gpu.flow_sample_batch(lat.clone(), cond, 2, 5.0), want)


def test_pipeline_takes_a_list_of_images():
    """upstream's batch dimension: pipe(image=[...]) -> one mesh per image; with one generator per image every object is
    what its own single-image call gives (grids bit-identical, hence meshes identical)"""
    import torch
    from PIL import Image
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    from oracle import hy3d_torch as H
    cfg = H.tiny_config()
    sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=5))
    pipe = Hunyuan3DDiTFlowMatchingPipeline(cfg, sd, "cuda:0", grid_chunk=2048)
    rng = np.random.default_rng(3)
    imgs = []
    for k in range(3):
        arr = np.zeros((90, 80, 4), np.uint8)
        arr[15 + k:70, 10:60 - 3 * k, :3] = rng.integers(0, 255, (55 - k, 50 - 3 * k, 3))
        arr[15 + k:70, 10:60 - 3 * k, 3] = 255
        imgs.append(Image.fromarray(arr, "RGBA"))
    kw = dict(num_inference_steps=4, octree_resolution=24, num_chunks=999, output_type="trimesh")
    singles, grids = [], []
    for im in imgs:
        singles.append(pipe(image=im, generator=torch.manual_seed(77), **kw)[0])
        grids.append(pipe.last_grid.clone())
    many = pipe(image=imgs, generator=[torch.Generator().manual_seed(77) for _ in imgs], **kw)
    assert len(many) == 3 and torch.equal(pipe.last_grid, grids[2])
    for a, b in zip(singles, many):
        assert np.array_equal(a.faces, b.faces) and np.array_equal(a.vertices, b.vertices)
    assert not np.array_equal(singles[0].vertices, singles[1].vertices)
    # ONE generator for the list: one draw of shape (n, N, C), upstream's prepare_latents
    one = pipe(image=imgs[:2], generator=torch.manual_seed(77), **kw)
    assert len(one) == 2 and all(m is not None and len(m.faces) > 0 for m in one)
    # host preparation of the call's images ahead of time on a thread (what the stage script and bench.py do for the NEXT
    # launch group): the same meshes, and torch's thread count is never touched
    threads = torch.get_num_threads()
    try:
        pipe.prefetch(imgs)
        ahead = pipe(image=imgs, generator=[torch.Generator().manual_seed(77) for _ in imgs], **kw)
        assert pipe._prefetched == {}                         # picked up by that call
    finally:
        pipe.close_prefetch()
    assert torch.get_num_threads() == threads
    for a, b in zip(many, ahead):
        assert np.array_equal(a.faces, b.faces) and np.array_equal(a.vertices, b.vertices)


def test_vae_and_grid_query(tiny):
    import torch
    g = torch.Generator().manual_seed(7)
    lat = torch.randn(tiny.cfg["vae"]["num_latents"], tiny.cfg["vae"]["embed_dim"], generator=g)
    R = 16
    with torch.no_grad():
        grid_ref, z_ref = tiny.oracle.latents_to_grid(lat[None], R, 1000)
    z = tiny.gpu.vae_decode(lat, return_z=True)
    err = rel_l2(z, z_ref[0])
    report("tiny vae latents", err, TOL["vae_latents"])
    assert err <= TOL["vae_latents"]
    grid = tiny.gpu.grid_query(1.01, R)
    d = (grid.cpu() - grid_ref).abs().max().item() / grid_ref.abs().max().item()
    report("tiny grid logits", d, TOL["grid_logits"])
    assert d <= TOL["grid_logits"]
    # a sub-range query writes only its own slots and matches the full query exactly
    part = torch.full_like(grid, float("nan"))
    tiny.gpu.grid_query(1.01, R, out=part, start=1000, count=777)
    flat, pf = grid.reshape(-1), part.reshape(-1)
    assert torch.equal(pf[1000:1777], flat[1000:1777])
    assert torch.isnan(pf[:1000]).all() and torch.isnan(pf[1777:]).all()


def test_query_side_cache_of_the_geo_decoder_is_bit_identical(tiny):
    """option geo_q_cache: what a grid point computes before it meets the object's latents (Fourier features, query_proj, ln_1,
    c_q, q-norm) stays in HBM after its first evaluation.  First pass (builds), second pass (hits), another object (hits),
    cache off, a sub-range query in the middle of a pass, and new weights (the cache must be dropped) -- all bit-identical."""
    import torch
    from r3g import ffi
    from r3g import model as M
    L = ffi.lib()
    g = torch.Generator().manual_seed(18)
    lat_a = torch.randn(tiny.cfg["vae"]["num_latents"], tiny.cfg["vae"]["embed_dim"], generator=g)
    lat_b = torch.randn(tiny.cfg["vae"]["num_latents"], tiny.cfg["vae"]["embed_dim"], generator=g)
    R = 40                                   # 41^3 = 68 921 points = 16 full passes of 4 096 + a partial one
    m = M.ShapeModel(tiny.cfg, tiny.sd, 0, grid_chunk=4096)
    try:
        ffi.check(L.r3g_set_option(b"geo_q_cache", 0))
        m.vae_decode(lat_a)
        ref_a = m.grid_query(1.01, R).clone()
        m.vae_decode(lat_b)
        ref_b = m.grid_query(1.01, R).clone()
        ffi.check(L.r3g_set_option(b"geo_q_cache", 1))
        m.vae_decode(lat_a)
        assert torch.equal(m.grid_query(1.01, R), ref_a)          # builds the cache
        assert torch.equal(m.grid_query(1.01, R), ref_a)          # served from it
        m.vae_decode(lat_b)
        assert torch.equal(m.grid_query(1.01, R), ref_b)          # another object, same cache
        part = torch.zeros_like(ref_b)
        m.grid_query(1.01, R, out=part, start=5000, count=9000)   # starts inside a pass: computed the old way
        assert torch.equal(part.reshape(-1)[5000:14000], ref_b.reshape(-1)[5000:14000])
        part.zero_()
        m.grid_query(1.01, R, out=part, start=8192, count=4096 * 3 + 5)   # canonical passes 2..4 from the cache + a fragment
        assert torch.equal(part.reshape(-1)[8192:8192 + 4096 * 3 + 5], ref_b.reshape(-1)[8192:8192 + 4096 * 3 + 5])
        # an option that changes what the cached Q rows hold (generation 1 kernels take a plain Q, the default ones a
        # pre-scaled Q): the passes built before the switch must not be served after it
        try:
            ffi.check(L.r3g_set_option(b"attn_generation", 1))
            with_stale_risk = m.grid_query(1.01, R).clone()
            ffi.check(L.r3g_set_option(b"geo_q_cache", 0))
            assert torch.equal(m.grid_query(1.01, R), with_stale_risk)
        finally:
            ffi.check(L.r3g_set_option(b"attn_generation", 7))
            ffi.check(L.r3g_set_option(b"geo_q_cache", 1))
        assert (with_stale_risk - ref_b).abs().max() <= 2e-2 * ref_b.abs().max()
        # other weights through the same context: the cache of the old ones must not survive
        from oracle import hy3d_torch as H
        sd2 = bf16_round_matrices(H.synthetic_state_dict(tiny.cfg, seed=77))
        m2 = M.ShapeModel(tiny.cfg, sd2, 0, grid_chunk=4096)
        m2.vae_decode(lat_a)
        with_cache = m2.grid_query(1.01, R).clone()
        ffi.check(L.r3g_set_option(b"geo_q_cache", 0))
        m2.vae_decode(lat_a)
        assert torch.equal(m2.grid_query(1.01, R), with_cache) and not torch.equal(with_cache, ref_a)
    finally:
        ffi.check(L.r3g_set_option(b"geo_q_cache", 1))


def test_grid_is_independent_of_internal_chunking(tiny):
    import torch
    from r3g import model as M
    g = torch.Generator().manual_seed(8)
    lat = torch.randn(tiny.cfg["vae"]["num_latents"], tiny.cfg["vae"]["embed_dim"], generator=g)
    tiny.gpu.vae_decode(lat)
    a = tiny.gpu.grid_query(1.01, 12).clone()
    other = M.ShapeModel(tiny.cfg, tiny.sd, 0, grid_chunk=640)
    other.vae_decode(lat)
    b = other.grid_query(1.01, 12)
    assert torch.equal(a, b)


def test_end_to_end_pipeline_tiny():
    """image -> mesh through the hy3dgen mirror; the mesh must be EXACTLY what the marching-cubes oracle
    extracts from the GPU's own grid (faces and vertices bit-exact for an identical SDF grid), and the grid
    itself must be within tolerance of the fp32 oracle pipeline."""
    import torch
    from PIL import Image
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    from oracle import hy3d_torch as H
    from oracle import mc as omc
    cfg = H.tiny_config()
    sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=5))
    pipe = Hunyuan3DDiTFlowMatchingPipeline(cfg, sd, "cuda:0", grid_chunk=2048)
    rng = np.random.default_rng(0)
    img = np.zeros((96, 80, 4), np.uint8)
    img[20:70, 15:60, :3] = rng.integers(0, 255, (50, 45, 3))
    img[20:70, 15:60, 3] = 255
    pil = Image.fromarray(img, "RGBA")
    mesh = pipe(image=pil, num_inference_steps=4, octree_resolution=24, num_chunks=999,
                generator=torch.manual_seed(1234567), output_type="trimesh")[0]
    grid = pipe.last_grid.cpu().numpy()
    ov, of = omc.hy3d_mesh(grid, 0.0, 1.01, 24)
    assert np.array_equal(mesh.faces, of.astype(np.int64))
    assert np.array_equal(mesh.vertices.astype(np.float32).view(np.uint32), ov.view(np.uint32))
    oracle = H.load_state_dict(H.ShapePipeline(cfg), sd)
    _, grid_ref = oracle(pil, num_inference_steps=4, octree_resolution=24, num_chunks=999,
                         generator=torch.manual_seed(1234567))
    d = np.abs(grid - grid_ref.numpy()).max() / np.abs(grid_ref.numpy()).max()
    report("tiny end-to-end grid (4 steps)", float(d), 2e-2)
    assert d <= 2e-2


@pytest.fixture(scope="module")
def wide():
    from oracle import hy3d_torch as H
    return Setup(H.wide_config(depth=1, depth_single=1, vae_layers=1, cond_layers=1), 11)


def test_full_width_dit_block_pair(wide):
    """Full widths and token counts of hunyuan3d-dit-v2-0 (hidden 1024, 16 heads, 3072 + 1370 tokens, CFG batch 2),
    one double + one single block: branch contributions block by block, then the velocity."""
    import torch
    x, t, cond = _inputs(wide, 1)
    assert _block_deltas(wide, x, t, cond, "full-width") <= TOL["block_delta"]
    with torch.no_grad():
        ref = wide.oracle.model(x, t, cond)
    out = wide.gpu.dit_forward(x, t, cond)
    assert torch.isfinite(out).all()
    err = rel_l2(out, ref)
    report("full-width 1+1 dit forward", err, TOL["dit_forward_tiny"])
    assert err <= TOL["dit_forward_tiny"]


def test_full_depth_dit_forward():
    """hunyuan3d-dit-v2-0 at full width AND full depth (16 double + 32 single blocks, 4442 tokens), one velocity
    evaluation: every block's branch contribution against the oracle block on the same input, and the final velocity
    against the oracle's own forward.  Batch 1 (the CFG batch is covered at depth 1+1 above and by flow_sample)."""
    import torch
    from oracle import hy3d_torch as H
    from parity_support import dit_inputs
    s = Setup(H.wide_config(depth=16, depth_single=32, vae_layers=1, cond_layers=1), 17)
    x, t, cond = dit_inputs(s.cfg, 3, batch=1)
    worst = _block_deltas(s, x, t, cond, "full-depth")
    assert worst <= TOL["block_delta"]
    with torch.no_grad():
        ref = s.oracle.model(x, t, cond)
    out = s.gpu.dit_forward(x, t, cond)
    err = rel_l2(out, ref)
    report("full-depth 16+32 dit forward", err, TOL["dit_forward_full_depth"])
    assert torch.isfinite(out).all() and err <= TOL["dit_forward_full_depth"]


def test_full_depth_conditioner_and_vae():
    """DINOv2-giant at full width AND full depth (40 layers, 1370 tokens) against the real transformers.Dinov2Model the
    oracle wraps, and the ShapeVAE transformer at its full 16 layers: the depths the 1-layer tests above do not reach."""
    import torch
    from oracle import hy3d_torch as H
    s = Setup(H.wide_config(depth=1, depth_single=1, vae_layers=16, cond_layers=40), 23)
    g = torch.Generator().manual_seed(5)
    img = torch.randn(3, 518, 518, generator=g)
    with torch.no_grad():
        ref = s.oracle.conditioner.main_image_encoder.model(img[None]).last_hidden_state[0]
    err = rel_l2(s.gpu.cond_encode(img).float(), ref)
    report("full-depth conditioner (40 layers, real Dinov2Model)", err, TOL["conditioner"])
    assert err <= TOL["conditioner"]
    lat = torch.randn(3072, 64, generator=g)
    with torch.no_grad():
        z_ref = s.oracle.vae(lat[None] / s.oracle.vae.scale_factor)
    err = rel_l2(s.gpu.vae_decode(lat, return_z=True), z_ref[0])
    report("full-depth vae latents (16 layers)", err, TOL["vae_latents"])
    assert err <= TOL["vae_latents"]


def test_full_width_conditioner_vae_and_grid_points(wide):
    import torch
    g = torch.Generator().manual_seed(3)
    img = torch.randn(3, 518, 518, generator=g)
    with torch.no_grad():
        ref = wide.oracle.conditioner.main_image_encoder.model(img[None]).last_hidden_state[0]
    err = rel_l2(wide.gpu.cond_encode(img).float(), ref)
    report("full-width conditioner (1 layer)", err, TOL["conditioner"])
    assert err <= TOL["conditioner"]
    lat = torch.randn(3072, 64, generator=g)
    with torch.no_grad():
        z_ref = wide.oracle.vae(lat[None] / wide.oracle.vae.scale_factor)
    z = wide.gpu.vae_decode(lat, return_z=True)
    err = rel_l2(z, z_ref[0])
    report("full-width vae latents (1 layer)", err, TOL["vae_latents"])
    assert err <= TOL["vae_latents"]
    # a slice of the real 257^3 grid (reference octree_resolution_hy: 256)
    R, start, count = 256, 257 * 257 * 100 + 12345, 3000
    pts = torch.from_numpy(wide.H.dense_grid_points(1.01, R)[start:start + count])
    with torch.no_grad():
        ref = wide.oracle.vae.geo_decoder(queries=pts[None], latents=z_ref)[0, :, 0]
    out = torch.zeros(257 ** 3, device="cuda")
    wide.gpu.grid_query(1.01, R, out=out, start=start, count=count)
    got = out[start:start + count].cpu()
    d = (got - ref).abs().max().item() / ref.abs().max().item()
    report("full-width grid logits (257^3 slice)", d, TOL["grid_logits"])
    assert d <= TOL["grid_logits"]


def test_layernorm_instantiations_are_bit_identical(wide):
    """The row kernels (LayerNorm, ln_dot) exist with a compile-time or a run-time row length and with 1 or 4 rows per
    wave (options ln_fixed / ln_rows; the automatic choice takes 4 rows from 65 536 rows per launch, option ln_rows4_min).  Same element -> lane
    map, same order of every sum: conditioner (C = 1536), VAE (C = 1024, fp32 rows), geo decoder (bf16 rows, ln_dot, a
    row count that is not a multiple of 16) and a DiT step (modulated rows) must not change a bit."""
    import torch
    from r3g import ffi
    L = ffi.lib()
    g = torch.Generator().manual_seed(9)
    img = torch.randn(3, 518, 518, generator=g)
    lat = torch.randn(3072, 64, generator=g)
    x, _, cond = _inputs(wide, 23)
    R, start, count = 256, 257 * 257 * 77 + 4321, 3001

    def run():
        c = wide.gpu.cond_encode(img).clone()
        z = wide.gpu.vae_decode(lat, return_z=True).clone()
        out = torch.zeros(257 ** 3, device="cuda")
        wide.gpu.grid_query(1.01, R, out=out, start=start, count=count)
        f = wide.gpu.flow_sample(x[0].clone(), cond, 1, 5.0).clone()
        return c, z, out[start:start + count].clone(), f
    outs = []
    try:
        # (round 6: + the MODE instantiations -- the affine-only / modulation-only launches with their optional terms known at
        # compile time, option ln_modes -- against the run-time form)
        for fixed, rows, modes in ((1, 4, 1), (1, 1, 1), (0, 1, 1), (0, 4, 1), (1, 4, 0), (1, 1, 0)):
            ffi.check(L.r3g_set_option(b"ln_fixed", fixed))
            ffi.check(L.r3g_set_option(b"ln_rows", rows))
            ffi.check(L.r3g_set_option(b"ln_modes", modes))
            outs.append(run())
    finally:
        ffi.check(L.r3g_set_option(b"ln_fixed", 1))
        ffi.check(L.r3g_set_option(b"ln_rows", 0))
        ffi.check(L.r3g_set_option(b"ln_modes", 1))
    names = ("conditioner", "vae z", "grid logits", "flow_sample")
    bad = []
    for (fixed, rows), o in zip(((1, 1), (0, 1), (0, 4), (14, 4), (11, 1)), outs[1:]):
        for name, a, b in zip(names, outs[0], o):
            if not torch.equal(a, b):
                bad.append("%s: ln_fixed=%d ln_rows=%d differs from (1, 4) in %d elements, max |d| %.3e"
                           % (name, fixed, rows, int((a != b).sum()), float((a.float() - b.float()).abs().max())))
    assert not bad, "; ".join(bad)
    assert all(torch.isfinite(t.float()).all() for t in outs[0])


def test_ln_post_and_output_proj_inside_the_last_residual_gemm(wide):
    """Round 6, option geo_lnd_fused (default): the geo decoder's last residual GEMM writes per-row statistics of its 64-column chunks
    (sum, squared deviations from the chunk mean, dot with gamma * w) instead of the stream, and a small kernel merges them (Chan's
    formula) into the logits -- the same function as the ln_dot launch over the stored stream, another summation order."""
    import torch
    from r3g import ffi
    L = ffi.lib()
    lat = torch.randn(3072, 64, generator=torch.Generator().manual_seed(5))
    wide.gpu.vae_decode(lat, return_z=True)
    R = 256
    outs = {}
    try:
        for fused in (1, 0):
            ffi.check(L.r3g_set_option(b"geo_lnd_fused", fused))
            for start, count in ((257 * 257 * 100 + 12345, 3000), (0, 2 * 131072 + 777)):     # a ragged slice; two canonical passes + a tail
                out = torch.zeros(257 ** 3, device="cuda")
                wide.gpu.grid_query(1.01, R, out=out, start=start, count=count)
                outs[(fused, start)] = out[start:start + count].cpu().clone()
    finally:
        ffi.check(L.r3g_set_option(b"geo_lnd_fused", 1))
    for start in (257 * 257 * 100 + 12345, 0):
        a, b = outs[(1, start)], outs[(0, start)]
        assert torch.isfinite(a).all()
        d = float((a - b).abs().max() / b.abs().max())
        report("geo decoder: ln_post + output_proj fused into the last GEMM vs the ln_dot launch (start %d)" % start, d, 1e-5)
        assert d <= 1e-5


def test_ln_3_folded_into_the_gemms_around_it(wide):
    """Round 6, option geo_ln3_fold (default): LN(x) W^T = rstd (x W'^T - mean c1) + c2 with W' = bf16(W gamma) -- c_proj's epilogue writes
    the row statistics of the stream it stores, c_fc runs on the raw stream.  Against the fp32 oracle at the grid-logit tolerance, and
    against the unfolded path (which rounds the normalised operand to bf16: a difference of that size is expected)."""
    import torch
    from r3g import ffi
    L = ffi.lib()
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(3072, 64, generator=g)
    with torch.no_grad():
        z_ref = wide.oracle.vae(lat[None] / wide.oracle.vae.scale_factor)
    wide.gpu.vae_decode(lat, return_z=True)
    R, start, count = 256, 257 * 257 * 100 + 12345, 3000
    pts = torch.from_numpy(wide.H.dense_grid_points(1.01, R)[start:start + count])
    with torch.no_grad():
        ref = wide.oracle.vae.geo_decoder(queries=pts[None], latents=z_ref)[0, :, 0]
    got = {}
    try:
        for fold in (1, 0):
            ffi.check(L.r3g_set_option(b"geo_ln3_fold", fold))
            out = torch.zeros(257 ** 3, device="cuda")
            wide.gpu.grid_query(1.01, R, out=out, start=start, count=count)
            got[fold] = out[start:start + count].cpu().clone()
            # two canonical passes through the query-side cache as well (the statistics ride on c_proj's cached-x0 form)
            out2 = torch.zeros(257 ** 3, device="cuda")
            wide.gpu.grid_query(1.01, R, out=out2, start=0, count=2 * 131072)
            got[(fold, "pass")] = out2[:2 * 131072].cpu().clone()
    finally:
        ffi.check(L.r3g_set_option(b"geo_ln3_fold", 1))
    scale = ref.abs().max().item()
    for fold in (1, 0):
        d = (got[fold] - ref).abs().max().item() / scale
        report("full-width grid logits, ln_3 %s (257^3 slice)" % ("folded into c_proj / c_fc" if fold else "as its own launch"), d, TOL["grid_logits"])
        assert torch.isfinite(got[fold]).all() and d <= TOL["grid_logits"]
    d = (got[1] - got[0]).abs().max().item() / scale
    report("  folded against unfolded", d, 1e-2)
    assert d <= 1e-2             # (two bf16-level approximations of the same function: measured 4-6e-3, each within 6e-3 of the fp32 oracle)
    dp = (got[(1, "pass")] - got[(0, "pass")]).abs().max().item() / got[(0, "pass")].abs().max().item()
    report("  folded against unfolded, two canonical passes", dp, 1e-2)
    assert dp <= 1e-2 and torch.isfinite(got[(1, "pass")]).all()


def test_geo_decoder_fp8_mode(wide):
    """option geo_fp8 (BASELINE.json configs[3]): the geo decoder's c_q / MLP GEMMs on e4m3 operands (LayerNorm quantises with
    row scales, the MLP hidden with a static scale) -- grid logits against the fp32 oracle, and against the bf16 path"""
    import torch
    from r3g import ffi
    L = ffi.lib()
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(3072, 64, generator=g)
    with torch.no_grad():
        z_ref = wide.oracle.vae(lat[None] / wide.oracle.vae.scale_factor)
    wide.gpu.vae_decode(lat, return_z=True)
    R, start, count = 256, 257 * 257 * 100 + 12345, 3000
    pts = torch.from_numpy(wide.H.dense_grid_points(1.01, R)[start:start + count])
    with torch.no_grad():
        ref = wide.oracle.vae.geo_decoder(queries=pts[None], latents=z_ref)[0, :, 0]
    out = torch.zeros(257 ** 3, device="cuda")
    wide.gpu.grid_query(1.01, R, out=out, start=start, count=count)
    bf16 = out[start:start + count].cpu().clone()
    modes = {}
    try:
        for mode in (3, 2, 1):          # c_q only, MLP only, both
            ffi.check(L.r3g_set_option(b"geo_fp8", mode))
            out.zero_()
            wide.gpu.grid_query(1.01, R, out=out, start=start, count=count)
            modes[mode] = out[start:start + count].cpu().clone()
    finally:
        ffi.check(L.r3g_set_option(b"geo_fp8", 0))
    for mode, name in ((3, "c_q only"), (2, "MLP only")):
        report("  fp8 %s" % name, (modes[mode] - ref).abs().max().item() / ref.abs().max().item(), TOL["grid_logits_fp8"])
    fp8 = modes[1]
    d = (fp8 - ref).abs().max().item() / ref.abs().max().item()
    report("full-width grid logits, geo decoder in fp8 mode (257^3 slice)", d, TOL["grid_logits_fp8"])
    report("  fp8 mode against the bf16 path", (fp8 - bf16).abs().max().item() / bf16.abs().max().item(), TOL["grid_logits_fp8"])
    assert torch.isfinite(fp8).all() and d <= TOL["grid_logits_fp8"]
    assert not torch.equal(fp8, bf16)                      # the mode really took the other path


def test_two_pipelines_with_private_contexts_run_concurrently():
    """jobs_per_gpu: two pipelines on one GPU, each with its own r3g_ctx and stream, driven by two host threads at the same
    time, give bit-identical grids to a sequential run (one context is not thread-safe; two are independent)"""
    import threading
    import torch
    from PIL import Image
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    from oracle import hy3d_torch as H
    cfg = H.tiny_config()
    sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=5))
    pipes = [Hunyuan3DDiTFlowMatchingPipeline(cfg, sd, "cuda:0", grid_chunk=2048, private_ctx=True) for _ in range(2)]
    rng = np.random.default_rng(0)
    imgs = []
    for k in range(2):
        arr = np.zeros((80, 80, 4), np.uint8)
        arr[20:60, 15:65, :3] = rng.integers(0, 255, (40, 50, 3))
        arr[20:60, 15:65, 3] = 255
        imgs.append(Image.fromarray(arr, "RGBA"))

    def one(k, out):
        with torch.cuda.stream(torch.cuda.Stream()):
            for _ in range(3):
                pipes[k](image=imgs[k], num_inference_steps=3, octree_resolution=16, generator=torch.Generator().manual_seed(7))
                torch.cuda.current_stream().synchronize()
                out.append(pipes[k].last_grid.clone())
    seq = [[], []]
    one(0, seq[0])
    one(1, seq[1])
    con = [[], []]
    th = [threading.Thread(target=one, args=(k, con[k])) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    for k in range(2):
        assert len(con[k]) == 3
        for a, b in zip(seq[k], con[k]):
            assert torch.equal(a, b)
    assert not torch.equal(seq[0][0], seq[1][0])


def test_fused_and_unfused_paths_agree(tiny):
    """A/B switches: the QKV epilogue fusion and the batched modulation GEMV must reproduce the separate kernels."""
    import torch
    from r3g import ffi
    L = ffi.lib()
    x, t, cond = _inputs(tiny, 9)
    a = tiny.gpu.dit_forward(x, t, cond).clone()
    try:
        ffi.check(L.r3g_set_option(b"fuse_qkv", 0))
        ffi.check(L.r3g_set_option(b"batch_mods", 0))
        b = tiny.gpu.dit_forward(x, t, cond).clone()
    finally:
        ffi.check(L.r3g_set_option(b"fuse_qkv", 1))
        ffi.check(L.r3g_set_option(b"batch_mods", 1))
    # the unfused path rounds the projection to bf16 before the q/k norm; the fused one normalises in fp32
    report("fused vs unfused qkv/mods", rel_l2(a, b), TOL["dit_forward_tiny"])
    assert rel_l2(a, b) <= TOL["dit_forward_tiny"]
    with torch.no_grad():
        ref = tiny.oracle.model(x, t, cond)
    assert rel_l2(a, ref) <= TOL["dit_forward_tiny"] and rel_l2(b, ref) <= TOL["dit_forward_tiny"]


def test_documented_attention_options_run_the_model(tiny):
    """r3g_set_option("attn_pipelined", 1) and attn_generation 1 select first-generation kernels that scale the scores
    themselves: the producers of Q must then leave it plain (attn_q_scale) -- every model attention used to fail with
    hipErrorInvalidValue under the documented option"""
    import torch
    from r3g import ffi
    L = ffi.lib()
    x, t, cond = _inputs(tiny, 14)
    with torch.no_grad():
        ref = tiny.oracle.model(x, t, cond)
    lat0 = x[0]
    ref_s = tiny.oracle.sample(cond, lat0[None].clone(), 3, 5.0)[0]
    for name, val, back in ((b"attn_pipelined", 1, 0), (b"attn_generation", 1, 7)):
        try:
            ffi.check(L.r3g_set_option(name, val))
            out = tiny.gpu.dit_forward(x, t, cond).clone()
            smp = tiny.gpu.flow_sample(lat0.clone(), cond, 3, 5.0).clone()      # the ragged (de-duplicated) launch too
        finally:
            ffi.check(L.r3g_set_option(name, back))
        assert rel_l2(out, ref) <= TOL["dit_forward_tiny"], name
        assert rel_l2(smp, ref_s) <= TOL["flow_sample"], name


def test_cfg_dedup_is_the_same_function(tiny):
    """The unconditional context (zeros) carried as one weighted token must reproduce the plain CFG batch."""
    import torch
    from r3g import ffi
    L = ffi.lib()
    x, _, cond = _inputs(tiny, 12)
    lat0 = x[0]
    a = tiny.gpu.flow_sample(lat0.clone(), cond, 5, 5.0).clone()          # cond[1] == 0 -> de-duplicated path
    try:
        ffi.check(L.r3g_set_option(b"cfg_dedup", 0))
        b = tiny.gpu.flow_sample(lat0.clone(), cond, 5, 5.0).clone()
    finally:
        ffi.check(L.r3g_set_option(b"cfg_dedup", 1))
    report("cfg dedup vs plain batch (5 steps)", rel_l2(a, b), TOL["same_function"])
    assert rel_l2(a, b) <= TOL["same_function"]
    ref = tiny.oracle.sample(cond, lat0[None].clone(), 5, 5.0)[0]
    assert rel_l2(a, ref) <= TOL["flow_sample"] and rel_l2(b, ref) <= TOL["flow_sample"]
    # a non-uniform "unconditional" context must take the general path (auto-detected) and still match the oracle
    cond_nu = cond.clone()
    cond_nu[1] = torch.randn_like(cond_nu[1]).to(torch.bfloat16).float()
    c = tiny.gpu.flow_sample(lat0.clone(), cond_nu, 3, 2.0)
    ref = tiny.oracle.sample(cond_nu, lat0[None].clone(), 3, 2.0)[0]
    assert rel_l2(c, ref) <= TOL["flow_sample"]


def test_fp16_stream_overflow_runs_the_group_again_on_the_fp32_stream():
    """The DiT's residual stream is fp16 by default (max 65504).  A checkpoint whose activations outgrow that -- here: the input
    projection scaled by 1e5 on a 256-wide model (the 16-bit stream exists from 256 columns on) -- gives non-finite latents on
    the fp16 stream; the guard (round 5) notices and runs the launch group again on the fp32 stream: the result IS the
    fp32 stream's, bit for bit, and finite.  With the guard off the fp16 stream's overflow is what comes back (so this input
    does force the branch)."""
    import torch
    from oracle import hy3d_torch as H
    from r3g import ffi
    from r3g import model as M
    L = ffi.lib()
    cfg = H.tiny_config()
    cfg["dit"].update(hidden_size=256, num_heads=4, depth=1, depth_single_blocks=1)
    sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=9))
    sd["model.latent_in.weight"] = sd["model.latent_in.weight"] * 1e5
    gpu = M.ShapeModel(cfg, sd, 0, grid_chunk=4096)
    from parity_support import dit_inputs
    x, _, cond = dit_inputs(cfg, 3)
    lat0 = x[0]
    guarded = gpu.flow_sample(lat0.clone(), cond, 3, 5.0).clone()
    try:
        ffi.check(L.r3g_set_option(b"dit_resid_f16", 0))
        f32 = gpu.flow_sample(lat0.clone(), cond, 3, 5.0).clone()
    finally:
        ffi.check(L.r3g_set_option(b"dit_resid_f16", 1))
    try:
        ffi.check(L.r3g_set_option(b"dit_f16_guard", 0))
        raw = gpu.flow_sample(lat0.clone(), cond, 3, 5.0).clone()
    finally:
        ffi.check(L.r3g_set_option(b"dit_f16_guard", 1))
    assert torch.isfinite(f32).all() and torch.equal(guarded, f32)
    assert not torch.isfinite(raw).all()
    # an ordinary checkpoint never takes the branch: guard on and off give the same bits
    sd2 = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=9))
    gpu2 = M.ShapeModel(cfg, sd2, 0, grid_chunk=4096)
    a = gpu2.flow_sample(lat0.clone(), cond, 3, 5.0).clone()
    try:
        ffi.check(L.r3g_set_option(b"dit_f16_guard", 0))
        b = gpu2.flow_sample(lat0.clone(), cond, 3, 5.0).clone()
    finally:
        ffi.check(L.r3g_set_option(b"dit_f16_guard", 1))
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_cfg_dedup_full_width(wide):
    import torch
    x, _, cond = _inputs(wide, 5)
    lat0 = x[0]
    out = wide.gpu.flow_sample(lat0.clone(), cond, 2, 5.0)
    ref = wide.oracle.sample(cond, lat0[None].clone(), 2, 5.0)[0]
    err = rel_l2(out, ref)
    report("full-width cfg dedup flow_sample 2 steps", err, TOL["flow_sample"])
    assert err <= TOL["flow_sample"]


@pytest.mark.parametrize("which", ["tiny", "wide"])
def test_grouped_stream_launches_are_bit_identical(which, tiny, wide):
    """The two streams of a double block share one GEMM launch (gemm_launch2); packing two problems into one grid
    must not change a single bit with respect to separate launches."""
    import torch
    from r3g import ffi
    L = ffi.lib()
    st = tiny if which == "tiny" else wide
    x, _, cond = _inputs(st, 21)
    lat0 = x[0]
    a = st.gpu.flow_sample(lat0.clone(), cond, 2, 5.0).clone()
    try:
        ffi.check(L.r3g_set_option(b"group_streams", 0))
        b = st.gpu.flow_sample(lat0.clone(), cond, 2, 5.0).clone()
    finally:
        ffi.check(L.r3g_set_option(b"group_streams", 1))
    assert torch.equal(a, b)
    # the MLP half of linear1 on a second stream beside the attention kernel (optional, off by default): scheduling only
    try:
        ffi.check(L.r3g_set_option(b"overlap_mlp", 1))
        c = st.gpu.flow_sample(lat0.clone(), cond, 2, 5.0).clone()
    finally:
        ffi.check(L.r3g_set_option(b"overlap_mlp", 0))
    assert torch.equal(a, c)
    for _ in range(3):                                   # and it is stable from run to run
        assert torch.equal(a, st.gpu.flow_sample(lat0.clone(), cond, 2, 5.0))


def test_from_pretrained_snapshot_directory(tmp_path):
    """the reference's entry point (src/2d_to_3d_models/run.py:122-124) on a local snapshot directory:
    <dir>/<subfolder>/config.yaml + model.fp16.safetensors -> same mesh as the pipeline built from the same tensors"""
    import torch
    import yaml
    from PIL import Image
    from safetensors.torch import save_file
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    from oracle import hy3d_torch as H
    from test_host_cpu import _snapshot_doc
    cfg = H.tiny_config()
    sd = {k: v.contiguous() for k, v in bf16_round_matrices(H.synthetic_state_dict(cfg, seed=5)).items()}
    sub = tmp_path / "hunyuan3d-dit-v2-0"
    sub.mkdir()
    (sub / "config.yaml").write_text(yaml.safe_dump(_snapshot_doc(cfg)))
    save_file(sd, str(sub / "model.fp16.safetensors"))
    a = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained(str(tmp_path), subfolder="hunyuan3d-dit-v2-0", variant="fp16")
    rng = np.random.default_rng(2)
    img = np.zeros((96, 80, 4), np.uint8)
    img[20:70, 15:60, :3] = rng.integers(0, 255, (50, 45, 3))
    img[20:70, 15:60, 3] = 255
    pil = Image.fromarray(img, "RGBA")
    kw = dict(image=pil, num_inference_steps=3, octree_resolution=24, num_chunks=999, output_type="trimesh")
    ma = a(generator=torch.manual_seed(7), **kw)[0]
    ga = a.last_grid.clone()
    b = Hunyuan3DDiTFlowMatchingPipeline(cfg, sd, "cuda:0")
    mb = b(generator=torch.manual_seed(7), **kw)[0]
    assert torch.equal(ga, b.last_grid)
    assert np.array_equal(ma.faces, mb.faces) and np.array_equal(ma.vertices, mb.vertices)
    with pytest.raises(FileNotFoundError):
        Hunyuan3DDiTFlowMatchingPipeline.from_pretrained(str(tmp_path / "missing"))
