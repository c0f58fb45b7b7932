"""Adaptive top-k KV selection in the geo decoder on the GPU (include/r3g.h: options "geo_kv_*", r3g_kv_selection_last,
r3g_op_kv_select, r3g_op_kv_gather; pipeline.kv_selection) against the restatement of DESIGN.md section 4d (tests/kvsel_ref.py).
The selection is checked as a valid top-k of float64 scores up to the fp32 accumulation bound; gather, identity mode and the switch
back to exact attention are equalities of bits."""
import ctypes

import numpy as np
import pytest

import kvsel_ref
from parity_support import TOL, bf16_round_matrices, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    ffi.context(0)
    return torch, ffi.lib(), ffi


def stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_l2(a, b):
    import torch
    return float(torch.linalg.norm(a.double() - b.double()) / (torch.linalg.norm(b.double()) + 1e-30))


def padded(torch, x, rows, fill):
    """x bf16 [H, n, 64] -> [H, rows, 64] on the device with `fill` in the padding rows"""
    out = torch.full((x.shape[0], rows, 64), fill, dtype=torch.bfloat16)
    out[:, :x.shape[1]] = x
    return out.cuda()


def device_select(env, q, k, group, stride, topk):
    """r3g_op_kv_select on bf16 q [H, n, 64], k [H, N, 64] (CPU tensors; junk in the padding rows) -> int64 [groups, H, topk]"""
    torch, L, ffi = env
    H, n, N = q.shape[0], q.shape[1], k.shape[1]
    lqp, lkp = (n + 127) // 128 * 128, (N + 63) // 64 * 64
    Q, K = padded(torch, q, lqp, 3.0), padded(torch, k, lkp, 7.0)
    groups = len(kvsel_ref.groups(n, group))
    idx = torch.full((groups, H, topk), -1, dtype=torch.int32, device="cuda")
    ffi.check(L.r3g_op_kv_select(Q.data_ptr(), n, lqp, K.data_ptr(), N, lkp, H, group, stride, topk, idx.data_ptr(), stream(torch)))
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64)


# ---- 1. the selection is a valid top-k ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,N,k,G,n", [(2, 256, 85, 1024, 2500), (4, 512, 256, 2048, 4096), (16, 3072, 1024, 8192, 8320)])
def test_selection_is_a_valid_topk(env, H, N, k, G, n):
    """random bf16 Q, K, stride 64.  With float64 scores s, the k-th largest t and eps = (S + 66) 2^-24 sum_d mean_s|q_sd| |k_d| (the
    fp32 accumulation bound of the mean over S samples and of the 64-term dot): selected keys have s >= t - 2 eps, the others
    s <= t + 2 eps, indices ascending and distinct; keys within 2 eps of t are unconstrained and at most 1 % of N per (group, head)
    (on these shapes: at most 6 of 3072)."""
    torch = env[0]
    g = torch.Generator().manual_seed(1000 * H + n)
    q = torch.randn(H, n, 64, generator=g).to(torch.bfloat16)
    kk = torch.randn(H, N, 64, generator=g).to(torch.bfloat16)
    idx = device_select(env, q, kk, G, 64, k)
    s, a, S = kvsel_ref.scores(q, kk, G, 64)
    assert S.tolist() == [len(kvsel_ref.sample_rows(r, 64)) for _, r in kvsel_ref.groups(n, G)]
    free = kvsel_ref.check_selection(idx, s, kvsel_ref.accumulation_eps(a, S), k, cap=0.01)
    report("kvsel: H=%d N=%d k=%d G=%d n=%d: largest share of keys within 2 eps of the threshold (cap 1e-2)" % (H, N, k, G, n), free, 1e-2)


# ---- 2. exact cases -----------------------------------------------------------------------------------------------------
def separated_case(torch, H, N, n, seed):
    """queries = one offset per head + small noise: q-bar is the offset up to the noise, so the scores spread over O(|offset|)"""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(H, 1, 64, generator=g) + 0.02 * torch.randn(H, n, 64, generator=g)).to(torch.bfloat16)
    k = torch.randn(H, N, 64, generator=g).to(torch.bfloat16)
    return q, k


def assert_separated(s, eps, k):
    """precondition on the test's own data: the k-th and (k+1)-th largest scores differ by more than 4 eps in every (group, head)"""
    N = s.shape[-1]
    if k >= N:
        return
    srt = np.sort(s, axis=-1)
    assert ((srt[..., N - k] - srt[..., N - k - 1]) > 4 * eps.max(-1)).all(), "test data: the threshold is not separated"


@pytest.mark.parametrize("H,N,G,n,k", [(2, 512, 1024, 2500, 171), (2, 512, 1024, 2500, 1), (2, 512, 1024, 2500, 512),
                                       (3, 256, 256, 256 + 30, 85)])
def test_separated_scores_give_exactly_the_reference_set(env, H, N, G, n, k):
    """scores separated far beyond eps at the threshold: the set is the restatement's.  k = 1, k = N (the identity), and (last case)
    a tail group of 30 rows: a single sample, row 0."""
    torch = env[0]
    q, kk = separated_case(torch, H, N, n, 77 + k)
    s, a, S = kvsel_ref.scores(q, kk, G, 64)
    if n == 256 + 30:
        assert S.tolist() == [4, 1]
    assert_separated(s, kvsel_ref.accumulation_eps(a, S), k)
    want = kvsel_ref.select(s, k)
    got = device_select(env, q, kk, G, 64, k)
    assert np.array_equal(got, want)
    if k == N:
        assert np.array_equal(got, np.broadcast_to(np.arange(N), got.shape))


@pytest.mark.parametrize("above", [0, 1])
def test_duplicated_keys_at_the_threshold_go_to_the_lower_index(env, above):
    """four identical key rows tie at the threshold (identical rows give identical fp32 scores), k - 1 - `above` keys score higher:
    the first 1 + `above` of the four by index are kept"""
    torch = env[0]
    H, N, G, k = 2, 512, 1024, 171
    q, kk = separated_case(torch, H, N, G, 5)
    s, a, S = kvsel_ref.scores(q, kk, G, 64)
    order = np.argsort(-s[0], axis=-1)                       # per head: keys by descending score
    dups = []
    for h in range(H):
        src = order[h, k - 1 - above]                        # the key at the threshold
        low = np.sort(order[h, N - 40:])[[3, 17, 31]]        # three keys far below it
        kk[h, torch.as_tensor(low)] = kk[h, int(src)].clone()
        dups.append(np.sort(np.concatenate([[src], low])))
    s, a, S = kvsel_ref.scores(q, kk, G, 64)
    eps = kvsel_ref.accumulation_eps(a, S)
    for h in range(H):
        row, t = s[0, h], s[0, h, dups[h][0]]
        assert len(set(row[dups[h]].tolist())) == 1 and (row > t).sum() == k - 1 - above
        # (precondition on the test's own data: nothing else comes near the tie)
        assert row[row > t].min() - t > 4 * eps[0, h].max() and t - row[row < t].max() > 4 * eps[0, h].max()
    got = device_select(env, q, kk, G, 64, k)
    assert np.array_equal(got, kvsel_ref.select(s, k))
    for h in range(H):
        kept = [int(j) for j in dups[h] if j in set(got[0, h].tolist())]
        assert kept == dups[h][:1 + above].tolist()


def test_a_nan_key_is_never_selected_while_finite_keys_remain(env):
    torch = env[0]
    H, N, G, k = 2, 512, 1024, 171
    q, kk = separated_case(torch, H, N, G, 9)
    s, a, S = kvsel_ref.scores(q, kk, G, 64)
    best = np.argmax(s[0], axis=-1)
    other = [1 if best[h] == 0 else 0 for h in range(H)]
    for h in range(H):
        kk[h, int(best[h])] = float("nan")                   # the key that would have ranked first: the whole row
        kk[h, other[h], 5] = float("nan")                    # a key of low index: one element
    s, a, S = kvsel_ref.scores(q, kk, G, 64)
    assert np.isnan(s).sum() == 2 * H
    want = kvsel_ref.select(s, k)
    fin = np.where(np.isnan(s), -np.inf, s)
    assert_separated(fin, kvsel_ref.accumulation_eps(np.nan_to_num(a), S), k)
    got = device_select(env, q, kk, G, 64, k)
    assert np.array_equal(got, want)
    for h in range(H):
        assert int(best[h]) not in got[0, h].tolist() and other[h] not in got[0, h].tolist()
    # with k = N - 1 one NaN key has to be taken: the one of lower index; with k = N all of them
    got = device_select(env, q, kk, G, 64, N - 1)
    assert np.array_equal(got, kvsel_ref.select(s, N - 1))
    for h in range(H):
        lo, hi = sorted((int(best[h]), other[h]))
        assert lo in got[0, h].tolist() and hi not in got[0, h].tolist()
    assert np.array_equal(device_select(env, q, kk, G, 64, N), np.broadcast_to(np.arange(N), (1, H, N)))


# ---- 3. gather ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,N,k,groups", [(2, 256, 85, 3), (4, 3072, 1024, 2)])
def test_gather_builds_the_attention_operands_of_the_selected_keys(env, H, N, k, groups):
    """compact K = K[idx] and compact V^T = make_vt(V[idx]) bit for bit, padding columns (k = 85: 43 of 128) zero; r3g_op_attention
    on them (batch = groups, own K / V) equals the same op on operands built here from K[idx], V[idx] bit for bit and is within the
    attention op's tolerance (1e-2, tests/test_ops_gpu.py) of fp32 SDPA over the gathered keys"""
    torch, L, ffi = env
    from r3g.layout import make_vt
    g = torch.Generator().manual_seed(N + k)
    kk = torch.randn(H, N, 64, generator=g).to(torch.bfloat16).cuda()
    v = torch.randn(H, N, 64, generator=g).to(torch.bfloat16).cuda()
    idx = torch.stack([torch.sort(torch.randperm(N, generator=g)[:k]).values for _ in range(groups * H)]).reshape(groups, H, k)
    idx_d = idx.to(torch.int32).cuda()
    kpad = (k + 63) // 64 * 64
    kc = torch.full((groups, H, kpad, 64), 5.0, dtype=torch.bfloat16, device="cuda")
    vtc = torch.full((groups, H, 64, kpad), 5.0, dtype=torch.bfloat16, device="cuda")
    ffi.check(L.r3g_op_kv_gather(kk.data_ptr(), make_vt(v, N).data_ptr(), N, N, H, idx_d.data_ptr(), groups, k, kc.data_ptr(),
                                 vtc.data_ptr(), stream(torch)))
    torch.cuda.synchronize()
    sel = idx.cuda()[..., None].expand(-1, -1, -1, 64)
    k_sel = kk[None].expand(groups, -1, -1, -1).gather(2, sel)           # [groups, H, k, 64]
    v_sel = v[None].expand(groups, -1, -1, -1).gather(2, sel)
    k_own = torch.zeros_like(kc)
    k_own[:, :, :k] = k_sel
    vt_own = make_vt(v_sel, kpad)
    assert torch.equal(kc.view(torch.int16), k_own.view(torch.int16))
    assert torch.equal(vtc.view(torch.int16), vt_own.view(torch.int16))
    if kpad > k:
        from r3g.layout import vt_key_positions
        used = torch.zeros(kpad, dtype=torch.bool)
        used[vt_key_positions(k)] = True
        assert float(vtc[..., (~used).cuda()].abs().max()) == 0.0 and float(kc[:, :, k:].abs().max()) == 0.0
    Lq = 256
    q = torch.randn(groups, H, Lq, 64, generator=g).to(torch.bfloat16).cuda()
    outs = []
    for K_, Vt_ in ((kc, vtc), (k_own, vt_own)):
        o = torch.zeros(groups, Lq, H * 64, dtype=torch.bfloat16, device="cuda")
        ffi.check(L.r3g_op_attention(q.data_ptr(), K_.data_ptr(), Vt_.data_ptr(), o.data_ptr(), groups, H, Lq, Lq, k, kpad, 0, 1,
                                     stream(torch)))
        torch.cuda.synchronize()
        outs.append(o)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    ref = torch.nn.functional.scaled_dot_product_attention(q.float(), k_sel.float(), v_sel.float())
    assert rel_l2(outs[0].float(), ref.permute(0, 2, 1, 3).reshape(groups, Lq, H * 64)) <= 1e-2


# ---- 4. / 5. the model ----------------------------------------------------------------------------------------------------
class Setup:
    def __init__(self, cfg, seed, grid_chunk=4096):
        from oracle import hy3d_torch as H
        from r3g import model as M
        self.cfg, self.H = cfg, H
        self.sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=seed))
        self.gpu = M.ShapeModel(cfg, self.sd, 0, grid_chunk=grid_chunk)
        self.N, self.heads = cfg["vae"]["num_latents"], cfg["vae"]["heads"]

    def latents(self, seed):
        import torch
        return torch.randn(self.N, self.cfg["vae"]["embed_dim"], generator=torch.Generator().manual_seed(seed))

    def oracle_vae(self):
        vae = self.H.ShapeVAE(**self.cfg["vae"]).eval()
        vae.load_state_dict({k[4:]: v for k, v in self.sd.items() if k.startswith("vae.")}, strict=True)
        return vae


def _cfg(which):
    from oracle import hy3d_torch as H
    if which == "tiny":
        return H.tiny_config(), 3            # W = 128: fp32 residual stream, no query-side cache
    cfg = H.wide_config(depth=1, depth_single=1, vae_layers=1, cond_layers=1)
    cfg["vae"].update(num_latents=512)       # W = 1024: bf16 stream, query-side cache; 512 latents
    return cfg, 11


@pytest.fixture(scope="module", params=["tiny", "wide"])
def model(request):
    cfg, seed = _cfg(request.param)
    s = Setup(cfg, seed)
    s.tag = request.param
    yield s
    s.gpu.set_kv_selection(0, 8192, 64)


def test_identity_selection_equals_the_exact_path_bit_for_bit(model):
    """geo_kv_topk = N_lat, groups of 1024: every key is kept in its own order, the path is taken with no shortcut, and the logits of
    the dense grid (R = 40: 17 passes of 4096, the last one 3 groups + a tail of 313) and of a ragged ascending list equal the exact
    path's.  The query-side cache is not allocated again by the switch."""
    import torch
    from r3g import ffi
    s, R = model, 40
    total = (R + 1) ** 3
    lst = torch.sort(torch.randperm(total, generator=torch.Generator().manual_seed(4))[:2 * 4096 + 777]).values.to(torch.int32).cuda()
    s.gpu.vae_decode(s.latents(7))
    try:
        s.gpu.set_kv_selection(0, 1024, 64)
        dense0 = s.gpu.grid_query(1.01, R).clone()
        list0 = s.gpu.grid_query_points(1.01, R, lst).clone()
        builds = ffi.counter("geo_q_cache_builds")
        sel0 = ffi.counter("geo_kv_groups")
        assert s.gpu.set_kv_selection(s.N, 1024, 64) == s.N
        dense1 = s.gpu.grid_query(1.01, R).clone()
        n_sel = ffi.counter("geo_kv_groups") - sel0
        assert n_sel == s.heads * (16 * 4 + 4)                   # 16 passes of 4 groups, one of 3 + a tail
        list1 = s.gpu.grid_query_points(1.01, R, lst).clone()
        assert ffi.counter("geo_kv_groups") - sel0 == n_sel + s.heads * (2 * 4 + 1)
        table = s.gpu.kv_selection_last()                        # the list's last pass: 777 points, one tail group
        assert tuple(table.shape) == (1, s.heads, s.N)
        assert torch.equal(table.cpu(), torch.arange(s.N, dtype=torch.int32).expand(1, s.heads, s.N))
        s.gpu.set_kv_selection(0)
        dense2 = s.gpu.grid_query(1.01, R).clone()
        assert ffi.counter("geo_q_cache_builds") == builds
    finally:
        s.gpu.set_kv_selection(0, 8192, 64)
    for name, a, b in (("dense grid", dense1, dense0), ("listed points", list1, list0), ("dense grid after the switch back", dense2, dense0)):
        diff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
        assert diff == 0, "%s, %s: %d of %d logits differ from the exact path's" % (s.tag, name, diff, a.numel())


def test_topk_logits_follow_the_restatement_fed_with_the_device_table(model):
    """the -1 rule (85 of 256, 256 of 512) on one pass (R = 14: 3375 points, groups of 1024 + a tail of 303).  The device's table is
    (a) what r3g_op_kv_select gives on the device's own Q / K and a valid top-k of their float64 scores (as in the op test, with its
    cap), (b) where a bf16 allowance on the oracle's fp32 q, k leaves the cap reachable, also a valid top-k of those; fed to the
    restated decoder it reproduces the device's logits within the grid-logit tolerance (1e-2 of the logits' scale).
    The distance to the exact decoder is reported, not bounded: it is a property of the checkpoint."""
    import torch
    from r3g import ffi
    s, R, G = model, 14, 1024
    n = (R + 1) ** 3
    lat = s.latents(12)
    k = kvsel_ref.upstream_topk(s.N)
    assert k == {256: 85, 512: 256}[s.N]
    s.gpu.vae_decode(lat)
    try:
        s.gpu.set_kv_selection(0, G, 64)
        exact = s.gpu.grid_query(1.01, R).reshape(-1).cpu()
        assert s.gpu.set_kv_selection(-1, G, 64) == k
        got = s.gpu.grid_query(1.01, R).reshape(-1).cpu()
        table = s.gpu.kv_selection_last()
        dq, dk = s.gpu.kv_selection_operands()
        torch.cuda.synchronize()
    finally:
        s.gpu.set_kv_selection(0, 8192, 64)
    groups = len(kvsel_ref.groups(n, G))
    assert tuple(table.shape) == (groups, s.heads, k) and tuple(dq.shape) == (s.heads, n, 64) and tuple(dk.shape) == (s.heads, s.N, 64)
    idx = table.cpu().numpy().astype(np.int64)
    # (a) the device's own operands
    again = device_select((torch, ffi.lib(), ffi), dq.cpu(), dk.cpu(), G, 64, k)
    assert np.array_equal(again, idx)
    sc, a, S = kvsel_ref.scores(dq, dk, G, 64)
    free = kvsel_ref.check_selection(idx, sc, kvsel_ref.accumulation_eps(a, S), k, cap=0.01)
    report("kvsel: %s model table: largest share of keys within 2 eps of the threshold (cap 1e-2)" % s.tag, free, 1e-2)
    # (b) the oracle's fp32 q, k.  Allowance: q and k reach the kernel rounded to bf16 (2^-9 relative each) and are themselves
    # projections of bf16-rounded operands (another 2^-9 each): 2^-7 of sum_d mean_s|q_sd| |k_d| on top of the accumulation bound.
    vae = s.oracle_vae()
    pts = torch.from_numpy(s.H.dense_grid_points(1.01, R))
    with torch.no_grad():
        z = vae(lat[None] / vae.scale_factor)
    oq, ok = kvsel_ref.oracle_qk(vae.geo_decoder, pts, z)
    so, ao, So = kvsel_ref.scores(oq, ok, G, 64)
    eps_o = kvsel_ref.accumulation_eps(ao, So) + 2.0 ** -7 * ao
    t = np.sort(so, axis=-1)[..., s.N - k][..., None]
    reachable = float(((np.abs(so - t) <= 2 * eps_o).sum(-1) / s.N).max()) <= 0.01
    print("kvsel %s: oracle-side validation %s" % (s.tag, "runs" if reachable else "skipped: the bf16 allowance leaves more than 1 % "
                                                   "of the keys unconstrained; the device's own operands were validated instead"))
    if reachable:
        kvsel_ref.check_selection(idx, so, eps_o, k, cap=0.01)
    # the restatement with the device's table
    with torch.no_grad():
        want = kvsel_ref.topk_geo_decoder(vae.geo_decoder, idx, G)(queries=pts[None], latents=z)[0, :, 0]
        want_exact = vae.geo_decoder(queries=pts[None], latents=z)[0, :, 0]
    scale = float(want.abs().max())
    d = float((got - want).abs().max()) / scale
    report("kvsel: %s grid logits, top-k %d of %d, against the restatement with the device's table" % (s.tag, k, s.N), d, TOL["grid_logits"])
    assert torch.isfinite(got).all() and d <= TOL["grid_logits"]
    report("kvsel: %s |top-k - exact| / scale on the device, max (reported)" % s.tag, float((got - exact).abs().max()) / scale, 1e18)
    report("kvsel: %s |top-k - exact| / scale on the device, mean (reported)" % s.tag, float((got - exact).abs().mean()) / scale, 1e18)
    report("kvsel: %s |top-k - exact| / scale in the oracle, max (reported)" % s.tag, float((want - want_exact).abs().max()) / scale, 1e18)


# ---- 6. refusals and the pipeline ------------------------------------------------------------------------------------------
def test_refusals(env):
    torch, L, ffi = env
    cfg, seed = _cfg("tiny")
    s = Setup(cfg, seed)
    s.gpu.vae_decode(s.latents(1))
    with pytest.raises(ffi.R3GError) as e:
        s.gpu.kv_selection_last()                                 # no top-k pass yet
    assert e.value.code == -4
    with pytest.raises(ffi.R3GError) as e:
        s.gpu.kv_selection_operands()
    assert e.value.code == -4
    try:
        for bad in (dict(group=1000), dict(group=128), dict(stride=0)):
            with pytest.raises(ffi.R3GError) as e:
                s.gpu.set_kv_selection(-1, **bad)
            assert e.value.code == -1
        s.gpu.set_kv_selection(-1)
        ffi.check(L.r3g_set_option(b"geo_fp8", 1))
        idx = torch.arange(10, dtype=torch.int32).cuda()
        for call in (lambda: s.gpu.grid_query(1.01, 8), lambda: s.gpu.grid_query_points(1.01, 8, idx)):
            with pytest.raises(ffi.R3GError) as e:
                call()
            assert e.value.code == -1
        ffi.check(L.r3g_set_option(b"geo_fp8", 0))
        assert torch.isfinite(s.gpu.grid_query(1.01, 8)).all()
        assert tuple(s.gpu.kv_selection_last().shape) == (1, s.heads, 85)
    finally:
        ffi.check(L.r3g_set_option(b"geo_fp8", 0))
        s.gpu.set_kv_selection(0, 8192, 64)


def test_pipeline_kv_selection(monkeypatch):
    import torch
    from PIL import Image
    from hy3dgen.shapegen import Hunyuan3DDiTFlowMatchingPipeline
    from r3g import ffi
    monkeypatch.delenv("R3G_VOLUME_DECODER", raising=False)
    monkeypatch.delenv("R3G_KV_SELECTION", raising=False)
    pipe = Hunyuan3DDiTFlowMatchingPipeline.from_pretrained("synthetic:mini:0", device="cuda:0")
    rng = np.random.default_rng(0)
    img = np.zeros((96, 80, 4), np.uint8)
    img[20:70, 15:60, :3] = rng.integers(0, 255, (50, 45, 3))
    img[20:70, 15:60, 3] = 255
    pil = Image.fromarray(img, "RGBA")
    R = 64

    def run(**kw):
        mesh = pipe(image=pil, num_inference_steps=3, octree_resolution=R, generator=torch.manual_seed(1234567), **kw)[0]
        assert mesh is not None and len(mesh.faces) > 0
        return pipe.last_grid.clone()
    try:
        g0 = run()
        assert pipe.kv_selection == "exact" and pipe.timings["kv_selection"] == "exact"
        sel0 = ffi.counter("geo_kv_groups")
        pipe.kv_selection = "topk"
        g1 = run()                                                # marching cubes
        assert pipe.timings["kv_selection"] == "topk:256"         # upstream's rule on 512 latents
        assert ffi.counter("geo_kv_groups") > sel0 and not torch.equal(g1, g0)
        run(mc_algo="dmc")                                        # dual marching cubes
        pipe.hier_min_resolution = 32                             # levels 32, 64: listed points as well
        pipe.enable_flashvdm()
        sel1 = ffi.counter("geo_kv_groups")
        run()
        assert pipe.last_hier_stats["levels"] == [32, 64] and pipe.timings["kv_selection"] == "topk:256"
        assert ffi.counter("geo_kv_groups") > sel1 and pipe.kv_selection == "topk"
        pipe.enable_flashvdm(False)
        pipe.kv_selection = "exact"
        sel2 = ffi.counter("geo_kv_groups")
        g4 = run()
        assert pipe.timings["kv_selection"] == "exact" and ffi.counter("geo_kv_groups") == sel2
        assert torch.equal(g4.view(torch.int32), g0.view(torch.int32))
    finally:
        pipe.model.set_kv_selection(0, 8192, 64)
