"""Option attn_interleave 2 (csrc/attn.hip VAR bit 3, profiles/attention_skew.md): the 64-query kernel's fast pass with its softmax
skewed ACROSS key blocks in steady state, and the K half of the staging ring one tile ahead of the V^T half.  It changes the order in
which a wave issues its instructions and where the workgroup meets its barrier, not one operation: every output must equal the
clustered body's (attn_interleave 3) bit for bit, with either form of the LDS-DMA (attn_async_stage)."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

SKEWED, CLUSTERED = 2, 3
OPTION_DEFAULTS = {b"attn_interleave": 0, b"attn_async_stage": 1, b"attn_wide_min": 2048, b"attn_generation": 7}     # csrc/attn.hip


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    ffi.context(0)
    return torch, ffi.lib(), ffi


def _restore(env):
    _, L, ffi = env
    for name, val in OPTION_DEFAULTS.items():
        ffi.check(L.r3g_set_option(name, val))


def _operands(torch, B, H, Lq, Lk, shared, seed):
    """random Q / K / V^T in the kernels' layouts, junk in the padded query rows and in the padded keys of K and V^T"""
    from r3g.layout import make_vt, vt_key_positions
    g = torch.Generator(device="cuda").manual_seed(seed)
    Bk = 1 if shared else B
    lqp, lkp = (Lq + 127) // 128 * 128, (Lk + 63) // 64 * 64
    Q = torch.full((B, H, lqp, 64), 3.0, device="cuda", dtype=torch.bfloat16)
    K = torch.full((Bk, H, lkp, 64), 7.0, device="cuda", dtype=torch.bfloat16)
    Q[:, :, :Lq] = torch.randn(B, H, Lq, 64, device="cuda", generator=g).to(torch.bfloat16)
    K[:, :, :Lk] = torch.randn(Bk, H, Lk, 64, device="cuda", generator=g).to(torch.bfloat16)
    Vt = make_vt(torch.randn(Bk, H, Lk, 64, device="cuda", generator=g), lkp)
    pad = torch.ones(lkp, dtype=torch.bool, device="cuda")
    pad[vt_key_positions(Lk, Vt.device)] = False
    Vt[..., pad] = -5.0
    return Q, K, Vt, lqp, lkp


def _run(env, ops, B, H, Lq, Lk, shared, interleave, async_stage):
    torch, L, ffi = env
    Q, K, Vt, lqp, lkp = ops
    o = torch.zeros(B, Lq, H * 64, device="cuda", dtype=torch.bfloat16)
    try:
        ffi.check(L.r3g_set_option(b"attn_generation", 6))
        ffi.check(L.r3g_set_option(b"attn_interleave", interleave))
        ffi.check(L.r3g_set_option(b"attn_async_stage", async_stage))
        ffi.check(L.r3g_op_attention(Q.data_ptr(), K.data_ptr(), Vt.data_ptr(), o.data_ptr(), B, H, Lq, lqp, Lk, lkp, shared, 1,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    finally:
        _restore(env)
    return o


def _skewed_equals_clustered(env, ops, B, H, Lq, Lk, shared, async_stage):
    torch = env[0]
    want = _run(env, ops, B, H, Lq, Lk, shared, CLUSTERED, async_stage)
    assert torch.isfinite(want.float()).all()
    got = _run(env, ops, B, H, Lq, Lk, shared, SKEWED, async_stage)
    assert torch.equal(got, want), "attn_interleave 2 against 3, attn_async_stage=%d on %s: %d values differ, max |d| %.3e" % (
        async_stage, (B, H, Lq, Lk), int((got != want).sum()), float((got.float() - want.float()).abs().max()))
    return want


def test_the_option_takes_its_four_values(env):
    _, L, ffi = env
    v = ctypes.c_int(-1)
    try:
        for val in (1, 2, 3, 0):
            ffi.check(L.r3g_set_option(b"attn_interleave", val))
            ffi.check(L.r3g_get_option(b"attn_interleave", ctypes.byref(v)))
            assert v.value == val
    finally:
        _restore(env)


# 1 to 9 key tiles, odd and even counts, full and padded last tiles, a last tile with one valid key: fill (block 1), the steady
# state with its moved barrier (from 3 unmasked blocks on), drain, and the masked last tile behind it
@pytest.mark.parametrize("async_stage", [0, 1])
@pytest.mark.parametrize("Lk", [64, 65, 96, 128, 129, 160, 192, 193, 256, 257, 320, 321, 513])
def test_skewed_is_bit_identical_on_small_shapes(env, Lk, async_stage):
    # one valid lane, a partial second query block, partial waves, a second workgroup with one valid query
    for Lq in (1, 33, 64, 255, 256, 257, 300):
        ops = _operands(env[0], 1, 2, Lq, Lk, 0, 1000 * Lk + Lq)
        _skewed_equals_clustered(env, ops, 1, 2, Lq, Lk, 0, async_stage)


@pytest.mark.parametrize("B,H,Lq,Lk,shared", [
    (1, 16, 131072, 3072, 1),      # one pass of the geo decoder's cross-attention: 8192 workgroups, two per CU throughout
    (2, 16, 4442, 4442, 0),        # the DiT's conditional entries (padded last tile)
])
def test_skewed_is_bit_identical_at_full_occupancy(env, B, H, Lq, Lk, shared):
    """the race check: every CU holds two workgroups whose waves meet the moved barrier at their own pace"""
    torch = env[0]
    ops = _operands(torch, B, H, Lq, Lk, shared, Lq + 3 * Lk)
    want = _skewed_equals_clustered(env, ops, B, H, Lq, Lk, shared, 1)
    assert torch.equal(_run(env, ops, B, H, Lq, Lk, shared, 0, 1), want), "attn_interleave 0 (automatic) differs"


@pytest.mark.parametrize("key", [40, 400, 430, 500])
def test_safe_pass_behind_a_skewed_fast_pass(env, key):
    """one key whose score exceeds the first block's by far more than the sum test's bound (2^16): in block 1 (made by the fill),
    in an even and an odd block of the steady state, and in the last block (finished by the drain).  The sticky flag sends the
    query tile through the safe pass; nothing of the skewed fast pass may survive."""
    torch = env[0]
    from r3g.layout import read_vt
    B, H, Lq, Lk = 1, 1, 128, 512
    ops = _operands(torch, B, H, Lq, Lk, 0, 11)
    Q, K, Vt, lqp, lkp = ops
    K[0, 0, key] = (Q[0, 0, 5].float() * 4.0).to(torch.bfloat16)
    for async_stage in (0, 1):
        want = _skewed_equals_clustered(env, ops, B, H, Lq, Lk, 0, async_stage)
        assert torch.allclose(want.float()[0, 5], read_vt(Vt, Lk).float()[0, 0, key], atol=3e-2)


def test_stale_rows_past_lq_change_no_bit(env):
    """rows past Lq hold whatever the producer left (here values whose scores overflow, and NaN): they set no sticky flag and
    change no valid row"""
    torch = env[0]
    B, H, Lq, Lk = 1, 2, 200, 300
    ops = _operands(torch, B, H, Lq, Lk, 0, 5)
    outs = []
    for junk in (0.0, 40.0, -40.0, float("nan")):
        ops[0][:, :, Lq:] = junk
        outs.append(_skewed_equals_clustered(env, ops, B, H, Lq, Lk, 0, 1))
    for o in outs[1:]:
        assert torch.equal(outs[0], o)


def test_small_shape_against_the_fp32_reference(env):
    """(the bit comparisons above would not notice an error shared by both forms)"""
    torch = env[0]
    from r3g.layout import read_vt
    B, H, Lq, Lk = 1, 4, 700, 1030
    ops = _operands(torch, B, H, Lq, Lk, 0, 17)
    Q, K, Vt, lqp, lkp = ops
    got = _run(env, ops, B, H, Lq, Lk, 0, SKEWED, 1)
    ref = torch.nn.functional.scaled_dot_product_attention(Q[:, :, :Lq].float(), K[:, :, :Lk].float(), read_vt(Vt, Lk).float())
    ref = ref.permute(0, 2, 1, 3).reshape(B, Lq, H * 64)
    err = float(torch.linalg.norm(got.double() - ref.double()) / torch.linalg.norm(ref.double()))
    assert err <= 1e-2, err


@pytest.fixture(scope="module")
def mini():
    """hunyuan3d-dit-v2-mini's widths and token counts at depth 1 + 1"""
    from oracle import hy3d_torch as H
    from test_model_gpu import Setup
    cfg = H.mini_config()
    cfg["dit"].update(depth=1, depth_single_blocks=1)
    cfg["vae"].update(num_decoder_layers=1)
    cfg["cond"].update(num_hidden_layers=1)
    return Setup(cfg, 41)


def _both_forms(env, compute):
    """compute() under attn_interleave 2 and 3, every attention launch on the 64-query kernel (attn_wide_min 1)"""
    _, L, ffi = env
    outs = {}
    try:
        ffi.check(L.r3g_set_option(b"attn_wide_min", 1))
        for il in (CLUSTERED, SKEWED):
            ffi.check(L.r3g_set_option(b"attn_interleave", il))
            outs[il] = compute()
    finally:
        _restore(env)
    return outs[SKEWED], outs[CLUSTERED]


@pytest.mark.parametrize("n", [1, 4])
def test_latents_do_not_depend_on_the_form(env, mini, n):
    """the DiT's ragged joint-attention launch (per object a conditional entry and the de-duplicated unconditional one with its
    weighted key in a masked last tile) through r3g_flow_sample"""
    torch = env[0]
    from test_model_gpu import _batch_inputs
    lat, cond = _batch_inputs(mini, n, 500)

    def sample():
        if n == 1:
            return mini.gpu.flow_sample(lat[0].clone(), cond[0], 2, 5.0).clone()
        return mini.gpu.flow_sample_batch(lat.clone(), cond, 2, 5.0).clone()
    got, want = _both_forms(env, sample)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), "max |d| %.3e" % float((got - want).abs().max())


def test_full_width_ragged_launch_does_not_depend_on_the_form(env):
    """the DiT's launch of four objects at full width (per object entries of 4442 and 3073 tokens x 16 heads: 1984 work items of 256
    queries), once: the race check on the ragged shape -- and the launch class that the automatic rule moves from the 32-query
    kernel to the skewed 64-query one.  Object 1 of these inputs sets the sticky flag, and the two passes round P at different
    scales at the weighted key: the moved launch must vote on its safe pass per 128 queries to keep the 32-query kernel's bits."""
    torch, L, ffi = env
    from oracle import hy3d_torch as H
    from test_model_gpu import Setup, _batch_inputs
    wide = Setup(H.wide_config(depth=1, depth_single=1, vae_layers=1, cond_layers=1), 11)
    lat, cond = _batch_inputs(wide, 4, 500)

    def sample():
        return wide.gpu.flow_sample_batch(lat.clone(), cond, 2, 5.0).clone()
    got, want = _both_forms(env, sample)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), "max |d| %.3e" % float((got - want).abs().max())
    try:
        automatic = sample()                                     # the 64-query kernel, skewed, by the automatic rule
        ffi.check(L.r3g_set_option(b"attn_interleave", CLUSTERED))
        gen2 = sample()                                          # a forced body leaves the launch on the 32-query kernel
    finally:
        _restore(env)
    assert torch.equal(automatic, gen2), "the moved launch differs from generation 2: max |d| %.3e" % float((automatic - gen2).abs().max())


def test_grid_logits_do_not_depend_on_the_form(env, mini):
    """r3g_grid_query on the mini model's 512 latent tokens (eight unmasked key tiles): a slice inside the grid and the grid's
    tail, whose last pass is a partial one"""
    torch = env[0]
    lat = torch.randn(512, 64, generator=torch.Generator().manual_seed(5))
    mini.gpu.vae_decode(lat, return_z=True)
    n3 = 65 ** 3

    def query():
        res = []
        for start, count in ((65 * 65 * 20 + 123, 3000), (n3 - 2 * 4096 - 777, 2 * 4096 + 777)):
            out = torch.zeros(n3, device="cuda")
            mini.gpu.grid_query(1.01, 64, out=out, start=start, count=count)
            res.append(out[start:start + count].clone())
        return torch.cat(res)
    got, want = _both_forms(env, query)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), "max |d| %.3e" % float((got - want).abs().max())
