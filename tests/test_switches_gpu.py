"""Every public kernel switch end to end (tests/switch_table.py): under each non-default value the affected stages of a full-width,
depth-1 model -- and the op-level GEMM / attention, a resnet block of the texture UNet and a marching-cubes volume -- still compute
what include/r3g.h promises for that switch ("bits": equal to the default-switch result; "tol": the stage's existing tolerance
against the fp32 oracle), and the kernel-choice counters of r3g_get_counter show that the switch was obeyed rather than ignored.

Setup as tests/test_model_gpu.py's `wide` fixture; the fp32 oracle outputs and the default-switch baselines are computed once per module.
"""
import ctypes

import numpy as np
import pytest

import switch_table as T
from parity_support import TOL, bf16_round_matrices, rel_l2, report

pytestmark = pytest.mark.gpu

R = 256
SLICE = (257 * 257 * 100 + 12345, 3000)          # a ragged slice of the 257^3 grid
PASSES = (0, 2 * 131072)                         # canonical passes of the query-side cache, from the grid's start
PASS_SAMPLE = 89                                 # the oracle evaluates every 89th point of PASSES (2946 points)
TOL_GEMM, TOL_ATTN, TOL_UNET = 5e-3, 1e-2, 1e-2  # tests/test_ops_gpu.py's and tests/test_unet_gpu.py's


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class World:
    """the model, its oracle, the inputs of every stage, the oracle's outputs, and the stages themselves"""

    def __init__(self):
        import torch
        from oracle import hy3d_torch as H
        from oracle import unet_torch as U
        from r3g import ffi
        from r3g import model as M
        from r3g import unet as RU
        self.torch, self.ffi, self.L, self.H = torch, ffi, ffi.lib(), H
        torch.manual_seed(0)
        cfg = H.wide_config(depth=1, depth_single=1, vae_layers=1, cond_layers=1)
        sd = bf16_round_matrices(H.synthetic_state_dict(cfg, seed=11))
        self.oracle = H.load_state_dict(H.ShapePipeline(cfg), sd)
        self.gpu = M.ShapeModel(cfg, sd, 0, grid_chunk=4096)
        g = torch.Generator().manual_seed(3)
        self.img = torch.randn(3, 518, 518, generator=g)
        self.lat = torch.randn(3072, 64, generator=g)
        from parity_support import dit_inputs
        self.x, self.t, self.cond = dit_inputs(cfg, 1)
        self.grid = torch.zeros(257 ** 3, device="cuda")
        # the texture UNet's smallest resnet block case (tests/test_unet_gpu.py: 8 x 8, 64 channels)
        ucfg = U.small_config()
        usd = {k: (v.to(torch.bfloat16).float() if v.ndim >= 2 else v.clone()) for k, v in U.synthetic_state_dict(ucfg, seed=3).items()}
        self.unet_oracle = U.load(ucfg, usd)
        self.unet = RU.UnetBlocks(usd, max_hw=8 * 8, max_channels=max(ucfg["block_out_channels"]), temb_dim=ucfg["temb_dim"],
                                  ctx_dim=ucfg["cross_attention_dim"], ctx_tokens=ucfg["ctx_tokens"], groups=ucfg["groups"])
        gu = torch.Generator().manual_seed(18)
        self.ux = torch.randn(1, 64, 8, 8, generator=gu)
        self.utemb = torch.randn(1, ucfg["temb_dim"], generator=gu)
        # marching cubes: the row-marching kernel (the one "mc_rows" / "mc_deferred" act in) runs on rows of 256 cells
        rng = np.random.default_rng(7)
        vol = rng.standard_normal((5, 19, 257)).astype(np.float32)
        for _ in range(3):
            for ax in range(3):
                vol = (np.roll(vol, 1, ax) + 2 * vol + np.roll(vol, -1, ax)) / 4
        self.vol = torch.from_numpy(vol.astype(np.float32)).cuda()
        self.ops = {}
        self._oracle_outputs()

    def _oracle_outputs(self):
        torch, o = self.torch, self.oracle
        with torch.no_grad():
            self.ref = {"cond": o.conditioner.main_image_encoder.model(self.img[None]).last_hidden_state[0],
                        "dit": o.model(self.x, self.t, self.cond),
                        "flow": o.sample(self.cond, self.x[0][None].clone(), 2, 5.0)[0]}
            z_ref = o.vae(self.lat[None] / o.vae.scale_factor)
            self.ref["vae"] = z_ref[0]
            pts = self.H.dense_grid_points(1.01, R)
            self.pass_idx = torch.arange(PASSES[0], PASSES[0] + PASSES[1], PASS_SAMPLE)
            for key, sel in (("slice", slice(SLICE[0], SLICE[0] + SLICE[1])), ("passes", self.pass_idx.numpy())):
                self.ref[key] = o.vae.geo_decoder(queries=torch.from_numpy(pts[sel])[None], latents=z_ref)[0, :, 0]
            self.ref["unet"] = self.unet_oracle.down_blocks[0].resnets[0](self.ux, self.utemb)

    # ---- stages: each returns {output name: tensor} --------------------------------------------------------------------------------
    def cond_stage(self, row):
        return {"cond": self.gpu.cond_encode(self.img).float().cpu()}

    def dit_stage(self, row):
        out = self.gpu.dit_forward(self.x, self.t, self.cond).cpu()
        # one evaluated step: a 2-entry schedule is sigma 0 -> 1 and upstream's trailing step with d_sigma = 0
        flow = self.gpu.flow_sample(self.x[0].clone(), self.cond, 2, 5.0).cpu()
        return {"dit": out, "flow": flow}

    def vae_stage(self, row):
        return {"vae": self.gpu.vae_decode(self.lat, return_z=True).cpu()}

    def drop_geo_cache(self):
        """a canonical pass at another resolution: the query-side cache of the 257^3 grid is freed and the next query there allocates it"""
        small = self.torch.zeros(17 ** 3, device="cuda")
        self.gpu.grid_query(1.01, 16, out=small, start=0, count=4096)

    def geo_stage(self, row):
        self.gpu.vae_decode(self.lat, return_z=True)
        if row.get("drop_geo_cache"):
            self.drop_geo_cache()
        out = {}
        for key, (start, count) in (("slice", SLICE), ("passes", PASSES)):
            self.grid.zero_()
            self.gpu.grid_query(1.01, R, out=self.grid, start=start, count=count)
            out[key] = self.grid[start:start + count].cpu()
        return out

    def mc_stage(self, row):
        from r3g import mc as gpu_mc
        v, f = gpu_mc.marching_cubes(self.vol, 0.0)
        return {"mc_verts": v.cpu().view(self.torch.int32), "mc_faces": f.cpu()}

    def unet_stage(self, row):
        return {"unet": self.unet.resnet("down_blocks.0.resnets.0", self.ux, self.utemb, 64).cpu()}

    def _gemm_case(self, M, N, K):
        torch = self.torch
        if ("gemm", M, N, K) not in self.ops:
            g = torch.Generator(device="cuda").manual_seed(M * 7 + N)
            a = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
            w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
            bias = torch.randn(N, device="cuda", generator=g)
            gate = torch.randn(N, device="cuda", generator=g)
            c0 = torch.randn(M, N, device="cuda", generator=g)
            prod = (a.double() @ w.double().t() + bias.double())
            self.ops[("gemm", M, N, K)] = (a, w, bias, gate, c0, prod)
        return self.ops[("gemm", M, N, K)]

    def gemm_stage(self, row):
        """r3g_op_gemm under the process-wide staging mode; epilogue 0 (bf16), 3 (fp32 residual with gate), 4 (fp32), 6 (bf16 residual)"""
        torch, L, ffi = self.torch, self.L, self.ffi
        M, N, K = row.get("gemm", T.GEMM_DEFAULT)
        a, w, bias, gate, c0, prod = self._gemm_case(M, N, K)
        dma = T.get_option(L, ffi, "lds_dma")
        out = {}
        for epi in row.get("gemm_epis", (0,)):
            dt = torch.bfloat16 if epi in (0, 6) else torch.float32
            c = c0.to(dt).clone() if epi in (3, 6) else torch.full((M, N), float("nan"), device="cuda", dtype=dt)
            gp = gate.data_ptr() if epi in (3, 6) else None
            if row.get("gemm_splitk_ws"):
                ws = torch.empty(16 * M * N, device="cuda")
                ffi.check(L.r3g_op_gemm_splitk(a.data_ptr(), K, w.data_ptr(), K, bias.data_ptr(), c.data_ptr(), N, gp, M, N, K, epi,
                                               ws.data_ptr(), ws.numel(), None, _stream(torch)))
            else:
                ffi.check(L.r3g_op_gemm(a.data_ptr(), K, w.data_ptr(), K, bias.data_ptr(), c.data_ptr(), N, gp, M, N, K, epi, dma,
                                        _stream(torch)))
            torch.cuda.synchronize()
            out["gemm_epi%d" % epi] = c.cpu()
            if ("gemm_ref", M, N, K, epi) not in self.ops:
                ref = prod if epi in (0, 4) else c0.to(dt).double() + gate.double() * prod
                self.ops[("gemm_ref", M, N, K, epi)] = ref.cpu()
            self.ref["gemm_epi%d" % epi, M, N, K] = self.ops[("gemm_ref", M, N, K, epi)]
        return out

    def attn_stage(self, row):
        torch, L, ffi = self.torch, self.L, self.ffi
        B, H, Lq, Lk = row.get("attn", T.ATTN_DEFAULT)
        if ("attn", B, H, Lq, Lk) not in self.ops:
            from test_ops_gpu import _attn_case
            self.ops[("attn", B, H, Lq, Lk)] = _attn_case(torch, B, H, Lq, Lk, 0, Lq + 3 * Lk)
        Q, K, Vt, ref, lqp, lkp = self.ops[("attn", B, H, Lq, Lk)]
        self.ref["attn"] = ref.cpu()
        o = torch.zeros(B, Lq, H * 64, device="cuda", dtype=torch.bfloat16)
        ffi.check(L.r3g_op_attention(Q.data_ptr(), K.data_ptr(), Vt.data_ptr(), o.data_ptr(), B, H, Lq, lqp, Lk, lkp, 0,
                                     T.get_option(L, ffi, "lds_dma"), _stream(torch)))
        torch.cuda.synchronize()
        return {"attn": o.cpu()}

    STAGE = {"cond": "cond_stage", "dit": "dit_stage", "vae": "vae_stage", "geo": "geo_stage", "mc": "mc_stage",
             "attn_op": "attn_stage", "gemm_op": "gemm_stage", "unet": "unet_stage"}

    def run(self, stage, row):
        out = getattr(self, self.STAGE[stage])(row)
        self.torch.cuda.synchronize()
        return out

    # ---- the project's existing metric and tolerance of every output against the fp32 oracle ------------------------------------
    def error(self, key, got, row):
        """-> (measured, tolerance)"""
        if key in ("slice", "passes"):
            ref = self.ref[key]
            g = got if key == "slice" else got[self.pass_idx - PASSES[0]]
            return float((g - ref).abs().max() / ref.abs().max()), TOL[row.get("tol_key", "grid_logits")]
        if key == "cond":
            return rel_l2(got, self.ref["cond"]), TOL["conditioner"]
        if key == "dit":
            return rel_l2(got, self.ref["dit"]), TOL["dit_forward_tiny"]
        if key == "flow":
            return rel_l2(got, self.ref["flow"]), TOL["flow_sample"]
        if key == "vae":
            return rel_l2(got, self.ref["vae"]), TOL["vae_latents"]
        if key == "unet":
            return rel_l2(got - self.ux, self.ref["unet"] - self.ux), TOL_UNET      # the branch contribution, as tests/test_unet_gpu.py
        if key == "attn":
            return rel_l2(got.float(), self.ref["attn"]), TOL_ATTN
        if key.startswith("gemm_epi"):
            M, N, K = row.get("gemm", T.GEMM_DEFAULT)
            return rel_l2(got.float(), self.ref[key, M, N, K]), TOL_GEMM
        raise KeyError(key)


@pytest.fixture(scope="module")
def world():
    import torch
    from r3g import ffi
    L = ffi.lib()
    assert T.not_at_default(L, ffi) == {}, "switches left off their defaults by an earlier test (current, default)"
    w = World()
    w.baselines = {}
    yield w
    torch.cuda.synchronize()
    # after everything this module (and, in a whole-suite run, every module before it) did: all switches are at their defaults
    assert T.not_at_default(L, ffi) == {}, "switches left off their defaults (current, default)"


def _baseline(w, stage, row):
    """the stage under default switches, or under the row's `with_` switches alone (a lowered threshold): computed once per setting"""
    key = (stage, tuple(sorted(row.get("with_", {}).items())), row.get("gemm"), row.get("gemm_epis"), row.get("attn"),
           bool(row.get("gemm_splitk_ws")), bool(row.get("drop_geo_cache")))
    if key not in w.baselines:
        with T.switched(w.L, w.ffi, **row.get("with_", {})):
            w.baselines[key] = w.run(stage, row)
        if row.get("drop_geo_cache"):
            w.drop_geo_cache()
    return w.baselines[key]


def _counters(w, names):
    return {n: T.get_counter(w.L, w.ffi, n) for n in names}


def _assert_counters(row, alt, stage, before, after, what):
    for name, expect in T.counter_checks(row, alt, stage):
        d = after[name] - before[name]
        if expect == "moves":
            assert d > 0, "%s: counter %s did not move on stage %s: the switch was not obeyed" % (what, name, stage)
        elif expect == "stays":
            assert d == 0, "%s: counter %s moved by %d on stage %s: the switch was not obeyed" % (what, name, d, stage)
        else:
            assert d == expect, "%s: counter %s moved by %d on stage %s, expected %d" % (what, name, d, stage, expect)


def test_default_switches_meet_the_oracle(world):
    """the baselines every other test compares with: each stage on default switches, at the project's tolerance for it"""
    torch = world.torch
    for stage in T.STAGES:
        row = {}
        out = _baseline(world, stage, row)
        for key, got in out.items():
            assert torch.isfinite(got.float()).all(), key
            if key.startswith("mc_"):
                continue
            err, tol = world.error(key, got, row)
            report("switches: default %s" % key, err, tol)
            assert err <= tol, (key, err, tol)
    assert len(world.baselines[("mc", (), None, None, None, False, False)]["mc_faces"]) > 1000


@pytest.mark.parametrize("name,alt", T.cases(), ids=["%s=%d" % c for c in T.cases()])
def test_switch(world, name, alt):
    torch, L, ffi = world.torch, world.L, world.ffi
    row = T.ROWS[name]
    what = "%s=%d" % (name, alt)
    names = sorted({c[0] for c in row.get("counter", ())})
    for stage in T.stages_of(row, alt):
        base = _baseline(world, stage, row)
        values = dict(row.get("with_", {}))
        values[name] = alt
        with T.switched(L, ffi, **values):
            assert T.get_option(L, ffi, name) == alt
            before = _counters(world, names)
            out = world.run(stage, row)
            after = _counters(world, names)
        if row.get("drop_geo_cache"):
            world.drop_geo_cache()                 # (the next query at 257^3 allocates the cache under the default budget again)
        assert T.get_option(L, ffi, name) == row["default"]
        promise = T.promise_of(row, stage, alt)
        differs = False
        for key, got in out.items():
            assert torch.isfinite(got.float()).all(), (what, key)
            same = torch.equal(got, base[key])
            differs = differs or not same
            if promise == "bits":
                assert same, "%s: %s differs from the default-switch result in %d elements, max |d| %.3e" % (
                    what, key, int((got != base[key]).sum()), float((got.float() - base[key].float()).abs().max()))
            elif key.startswith("mc_"):
                assert same, (what, key)
            else:
                err, tol = world.error(key, got, row)
                report("switches: %s %s" % (what, key), err, tol)
                assert err <= tol, (what, key, err, tol)
        if promise == "tol" and stage in T.differs_of(row, alt):
            assert differs, "%s: stage %s equals the default-switch result bit for bit although include/r3g.h says the rounding differs" % (what, stage)
        _assert_counters(row, alt, stage, before, after, what)


STAGING = {"r3g_set_staging(0)": None, "lds_dma=0": {"lds_dma": 0}, "gemm_wide_epilogue=0": {"gemm_wide_epilogue": 0}}


@pytest.mark.parametrize("how", sorted(STAGING))
@pytest.mark.parametrize("fold,lnd", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_staging_and_epilogue_switches_leave_the_geo_decoder_working(world, how, fold, lnd):
    """The folded geo-decoder epilogues exist for LDS-DMA staging and the wide epilogue only.  The model used to pick them from its own
    conditions alone, and r3g_set_staging(0), "lds_dma" 0 or "gemm_wide_epilogue" 0 turned every grid query into
    "gemm_launch(geo c_proj): invalid argument" (hipErrorInvalidValue from gemm_launch2).  Now the launcher's own predicate decides, and
    the unfolded launches run: R3G_OK, logits at the grid tolerance against the oracle, and no pass counted as folded."""
    torch, L, ffi = world.torch, world.L, world.ffi
    names = ("geo_lnf_passes", "geo_lnd_passes", "gemm_register_staged")
    try:
        if STAGING[how] is None:
            ffi.check(L.r3g_set_staging(0))
            assert T.get_option(L, ffi, "lds_dma") == 0
        with T.switched(L, ffi, geo_ln3_fold=fold, geo_lnd_fused=lnd, **(STAGING[how] or {})):
            before = _counters(world, names)
            z = world.gpu.vae_decode(world.lat, return_z=True).cpu()          # (ffi.check inside: anything but R3G_OK raises)
            out = world.geo_stage({})
            after = _counters(world, names)
    finally:
        ffi.check(L.r3g_set_staging(1))
    err = rel_l2(z, world.ref["vae"])
    report("switches: %s vae latents" % how, err, TOL["vae_latents"])
    assert err <= TOL["vae_latents"]
    for key, got in out.items():
        assert torch.isfinite(got).all()
        err, tol = world.error(key, got, {})
        report("switches: %s fold=%d lnd=%d geo %s" % (how, fold, lnd, key), err, tol)
        assert err <= tol, (how, fold, lnd, key, err)
    assert after["geo_lnf_passes"] == before["geo_lnf_passes"] and after["geo_lnd_passes"] == before["geo_lnd_passes"]
    if how != "gemm_wide_epilogue=0":
        assert after["gemm_register_staged"] > before["gemm_register_staged"]
    assert T.not_at_default(L, ffi) == {}


@pytest.mark.parametrize("how", sorted(STAGING))
def test_staging_and_epilogue_switches_leave_the_dit_and_the_conditioner_working(world, how):
    torch, L, ffi = world.torch, world.L, world.ffi
    try:
        if STAGING[how] is None:
            ffi.check(L.r3g_set_staging(0))
        with T.switched(L, ffi, **(STAGING[how] or {})):
            out = world.gpu.dit_forward(world.x, world.t, world.cond).cpu()
            tok = world.gpu.cond_encode(world.img).float().cpu()
    finally:
        ffi.check(L.r3g_set_staging(1))
    for key, got in (("dit", out), ("cond", tok)):
        assert torch.isfinite(got).all()
        err, tol = world.error(key, got, {})
        report("switches: %s %s" % (how, key), err, tol)
        assert err <= tol, (how, key, err)


def test_the_op_entry_points_put_the_staging_mode_back(world):
    """r3g_op_gemm / r3g_op_attention take the staging mode of THEIR launch as an argument; they used to leave LDS-DMA switched on
    behind them, whatever r3g_set_staging had selected"""
    torch, L, ffi = world.torch, world.L, world.ffi
    names = ("gemm_register_staged", "attn_register_staged")
    try:
        for mode in (0, 1):
            ffi.check(L.r3g_set_staging(mode))
            for dma in (1, 0):
                before = _counters(world, names)
                a, w, bias, gate, c0, prod = world._gemm_case(*T.GEMM_DEFAULT)
                M, N, K = T.GEMM_DEFAULT
                c = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
                ffi.check(L.r3g_op_gemm(a.data_ptr(), K, w.data_ptr(), K, bias.data_ptr(), c.data_ptr(), N, None, M, N, K, 0, dma,
                                        _stream(torch)))
                from test_ops_gpu import _attn_case
                B, H, Lq, Lk = T.ATTN_DEFAULT
                Q, Kk, Vt, ref, lqp, lkp = _attn_case(torch, B, H, Lq, Lk, 0, 5)
                o = torch.zeros(B, Lq, H * 64, device="cuda", dtype=torch.bfloat16)
                ffi.check(L.r3g_op_attention(Q.data_ptr(), Kk.data_ptr(), Vt.data_ptr(), o.data_ptr(), B, H, Lq, lqp, Lk, lkp, 0, dma,
                                             _stream(torch)))
                torch.cuda.synchronize()
                after = _counters(world, names)
                assert T.get_option(L, ffi, "lds_dma") == mode, (mode, dma)
                for n in names:                    # the launch itself obeyed its argument
                    assert after[n] - before[n] == (1 if dma == 0 else 0), (n, mode, dma)
                assert rel_l2(c.float().cpu(), prod.cpu()) <= TOL_GEMM and rel_l2(o.float(), ref) <= TOL_ATTN
    finally:
        ffi.check(L.r3g_set_staging(1))


def test_register_staging_differs_from_the_default_only_by_the_attention_variant(world):
    """"lds_dma" 0 keeps every bit of the DiT except through its attention, whose register-staged kernel is the "attn_variant" 0 body:
    the DiT stage under "lds_dma" 0 equals the DiT stage under "attn_variant" 0 bit for bit (and the plain-batch forward, which
    never meets that variant's corner, equals the default)"""
    torch, L, ffi = world.torch, world.L, world.ffi
    base = _baseline(world, "dit", {})
    with T.switched(L, ffi, attn_variant=0):
        v0 = world.run("dit", {})
    with T.switched(L, ffi, lds_dma=0):
        regs = world.run("dit", {})
    for key in v0:
        assert torch.equal(regs[key], v0[key]), key
    assert torch.equal(regs["dit"], base["dit"])
    assert not torch.equal(v0["flow"], base["flow"])          # (variant 0 does meet its corner on the de-duplicated context)


def test_phased_off_with_the_persistent_form_on(world):
    """launch_epi special-cases the pair: with "gemm_phased" 0 the automatic rule takes the two-stage 256 x 256 kernel (waves 9), which
    has no persistent form, so "gemm_persistent" 1 must be inert -- on the DiT workload with 8 CUs assumed, where every 256 x 256 grid
    would otherwise be persistent.  Same tiles, same k order: the default bits."""
    torch, L, ffi = world.torch, world.L, world.ffi
    base = _baseline(world, "dit", {})
    names = ("gemm_two_stage_256", "gemm_phased", "gemm_phased_persistent", "gemm_mixed")
    with T.switched(L, ffi, gemm_num_cu=8, gemm_phased=0, gemm_persistent=1):
        before = _counters(world, names)
        out = world.run("dit", {})
        after = _counters(world, names)
    for key in out:
        assert torch.equal(out[key], base[key]), key
    assert after["gemm_two_stage_256"] > before["gemm_two_stage_256"]
    for n in ("gemm_phased", "gemm_phased_persistent", "gemm_mixed"):
        assert after[n] == before[n], n


def test_every_switch_is_back_at_its_default(world):
    """the last test of the module (and, in a single-process run of the whole suite, nearly of the suite: the module sorts late)"""
    assert T.not_at_default(world.L, world.ffi) == {}
