"""Options attn_interleave and attn_async_stage (csrc/attn.hip, profiles/attention_interleave.md) change the ORDER in which the
attention kernels issue their instructions and where they wait for the LDS-DMA prefetch, not one operation: every output must
equal the kernels with both options off -- generation 6 / generation 2 as they were -- bit for bit."""
import ctypes
import itertools

import pytest

pytestmark = pytest.mark.gpu

OPTION_DEFAULTS = {b"attn_interleave": 0, b"attn_async_stage": 1}     # the library's defaults (csrc/attn.hip); the tests restore them


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    ffi.context(0)
    return torch, ffi.lib(), ffi


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _operands(torch, B, H, Lq, Lk, shared, seed):
    """random Q / K / V^T in the kernels' layouts; junk in the padded rows and keys (as tests/test_ops_gpu.py)"""
    from r3g.layout import make_vt
    g = torch.Generator(device="cuda").manual_seed(seed)
    Bk = 1 if shared else B
    lqp, lkp = (Lq + 127) // 128 * 128, (Lk + 63) // 64 * 64
    Q = torch.full((B, H, lqp, 64), 3.0, device="cuda", dtype=torch.bfloat16)
    K = torch.full((Bk, H, lkp, 64), 7.0, device="cuda", dtype=torch.bfloat16)
    Q[:, :, :Lq] = torch.randn(B, H, Lq, 64, device="cuda", generator=g).to(torch.bfloat16)
    K[:, :, :Lk] = torch.randn(Bk, H, Lk, 64, device="cuda", generator=g).to(torch.bfloat16)
    Vt = make_vt(torch.randn(Bk, H, Lk, 64, device="cuda", generator=g), lkp)
    return Q, K, Vt, lqp, lkp


def _run(env, ops, B, H, Lq, Lk, shared, gen, interleave, async_stage):
    torch, L, ffi = env
    Q, K, Vt, lqp, lkp = ops
    o = torch.zeros(B, Lq, H * 64, device="cuda", dtype=torch.bfloat16)
    ffi.check(L.r3g_set_option(b"attn_generation", gen))
    ffi.check(L.r3g_set_option(b"attn_interleave", interleave))
    ffi.check(L.r3g_set_option(b"attn_async_stage", async_stage))
    try:
        ffi.check(L.r3g_op_attention(Q.data_ptr(), K.data_ptr(), Vt.data_ptr(), o.data_ptr(), B, H, Lq, lqp, Lk, lkp, shared, 1,
                                     _stream(torch)))
        torch.cuda.synchronize()
    finally:
        ffi.check(L.r3g_set_option(b"attn_generation", 7))
        for name, val in OPTION_DEFAULTS.items():
            ffi.check(L.r3g_set_option(name, val))
    return o


def _all_forms_equal(env, ops, B, H, Lq, Lk, shared):
    """generation 6 in its four forms and generation 2 in its two against generation 6 with both options off"""
    torch = env[0]
    want = _run(env, ops, B, H, Lq, Lk, shared, 6, 0, 0)
    assert torch.isfinite(want.float()).all()
    for gen, il, asy in [(6, 1, 0), (6, 0, 1), (6, 1, 1), (2, 0, 0), (2, 0, 1)]:
        got = _run(env, ops, B, H, Lq, Lk, shared, gen, il, asy)
        assert torch.equal(got, want), "generation %d attn_interleave=%d attn_async_stage=%d on %s: %d values differ" % (
            gen, il, asy, (B, H, Lq, Lk), int((got != want).sum()))
    return want


@pytest.mark.parametrize("B,H,Lq,Lk,shared", [
    (1, 16, 131072, 3072, 1),      # one pass of the geo decoder's cross-attention
    (1, 16, 66305, 3072, 1),       # the 257^3 grid's last pass (66305 = 259 x 256 + 1: a query tile with one valid query)
    (1, 16, 3072, 3072, 0),        # VAE self-attention
    (1, 24, 1370, 1370, 0),        # DINOv2
    (2, 16, 4442, 4442, 0),        # the DiT's conditional entries
    (1, 2, 300, 64, 0), (1, 2, 300, 65, 0), (1, 2, 300, 96, 0), (1, 2, 300, 127, 0),   # one tile: full, one valid key in the
    (1, 2, 300, 129, 0), (1, 1, 700, 513, 0), (1, 3, 26, 26, 0),                      # second block, padded second block, ...
])
def test_interleaved_and_async_forms_are_bit_identical(env, B, H, Lq, Lk, shared):
    ops = _operands(env[0], B, H, Lq, Lk, shared, Lq + 3 * Lk)
    _all_forms_equal(env, ops, B, H, Lq, Lk, shared)


def test_small_shape_against_the_fp32_reference(env):
    """(the bit comparisons above would not notice an error shared by every form)"""
    torch = env[0]
    from r3g.layout import read_vt
    B, H, Lq, Lk = 1, 4, 700, 1030
    ops = _operands(torch, B, H, Lq, Lk, 0, 17)
    Q, K, Vt, lqp, lkp = ops
    got = _run(env, ops, B, H, Lq, Lk, 0, 6, 1, 1)
    ref = torch.nn.functional.scaled_dot_product_attention(Q[:, :, :Lq].float(), K[:, :, :Lk].float(), read_vt(Vt, Lk).float())
    ref = ref.permute(0, 2, 1, 3).reshape(B, Lq, H * 64)
    err = float(torch.linalg.norm(got.double() - ref.double()) / torch.linalg.norm(ref.double()))
    assert err <= 1e-2, err


@pytest.mark.parametrize("factor", [4.0, 1.04])
def test_safe_pass_is_taken_and_bit_identical(env, factor):
    """the inputs of tests/test_ops_gpu.py::test_attention_forced_rescale: one key far above the rest late in the sequence
    (factor 4: the sticky flag sends the query tile through the safe pass; 1.04: it stays on the fast pass)"""
    torch = env[0]
    from r3g.layout import read_vt
    B, H, Lq, Lk = 1, 1, 128, 512
    ops = _operands(torch, B, H, Lq, Lk, 0, 11)
    Q, K, Vt, lqp, lkp = ops
    K[0, 0, 400] = (Q[0, 0, 5].float() * factor).to(torch.bfloat16)
    want = _all_forms_equal(env, ops, B, H, Lq, Lk, 0)
    if factor == 4.0:
        assert torch.allclose(want.float()[0, 5], read_vt(Vt, Lk).float()[0, 0, 400], atol=3e-2)


def test_stale_rows_past_lq_change_no_bit(env):
    """the inputs of tests/test_ops_gpu.py::test_attention_ignores_stale_rows_past_lq"""
    torch = env[0]
    B, H, Lq, Lk = 1, 2, 200, 300
    ops = _operands(torch, B, H, Lq, Lk, 0, 5)
    outs = []
    for junk in (0.0, 40.0, -40.0):
        ops[0][:, :, Lq:] = junk
        outs.append(_all_forms_equal(env, ops, B, H, Lq, Lk, 0))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.fixture(scope="module")
def wide():
    from oracle import hy3d_torch as H
    from test_model_gpu import Setup
    return Setup(H.wide_config(depth=1, depth_single=1, vae_layers=1, cond_layers=1), 11)


@pytest.mark.parametrize("n", [1, 4])
def test_latents_do_not_depend_on_the_options(env, wide, n):
    """r3g_op_attention has no ragged entries and no weighted key: the DiT's joint attention launch (entries (4442, 4442) and
    (3073, 3073 with the weighted key 3072) per object) is checked through r3g_flow_sample at full width."""
    torch, L, ffi = env
    from test_model_gpu import _batch_inputs
    lat, cond = _batch_inputs(wide, n, 500)

    def sample():
        if n == 1:
            return wide.gpu.flow_sample(lat[0].clone(), cond[0], 2, 5.0).clone()
        return wide.gpu.flow_sample_batch(lat.clone(), cond, 2, 5.0).clone()
    outs = {}
    try:
        for il, asy in itertools.product((0, 1), (0, 1)):
            ffi.check(L.r3g_set_option(b"attn_interleave", il))
            ffi.check(L.r3g_set_option(b"attn_async_stage", asy))
            outs[(il, asy)] = sample()
    finally:
        for name, val in OPTION_DEFAULTS.items():
            ffi.check(L.r3g_set_option(name, val))
    assert torch.isfinite(outs[(0, 0)]).all()
    for key, got in outs.items():
        assert torch.equal(got, outs[(0, 0)]), "attn_interleave=%d attn_async_stage=%d: max |d| %.3e" % (
            key + (float((got - outs[(0, 0)]).abs().max()),))


def test_grid_logits_do_not_depend_on_the_options(env, wide):
    """r3g_grid_query on the real 257^3 grid: two canonical 131072-query passes and a tail, and a ragged slice"""
    torch, L, ffi = env
    lat = torch.randn(3072, 64, generator=torch.Generator().manual_seed(5))
    wide.gpu.vae_decode(lat, return_z=True)
    outs = {}
    try:
        for il, asy in itertools.product((0, 1), (0, 1)):
            ffi.check(L.r3g_set_option(b"attn_interleave", il))
            ffi.check(L.r3g_set_option(b"attn_async_stage", asy))
            for start, count in ((257 * 257 * 100 + 12345, 3000), (0, 2 * 131072 + 777)):
                out = torch.zeros(257 ** 3, device="cuda")
                wide.gpu.grid_query(1.01, 256, out=out, start=start, count=count)
                outs[(il, asy, start)] = out[start:start + count].clone()
    finally:
        for name, val in OPTION_DEFAULTS.items():
            ffi.check(L.r3g_set_option(name, val))
    for (il, asy, start), got in outs.items():
        assert torch.isfinite(got).all()
        assert torch.equal(got, outs[(0, 0, start)]), "attn_interleave=%d attn_async_stage=%d start %d" % (il, asy, start)
