"""One table of the library's process-wide switches (r3g_set_option), shared by tests/test_switch_table_cpu.py,
tests/test_abi.py and tests/test_switches_gpu.py, and the `switched` context manager the new tests set them with.

A row:
  default     the value a fresh process has (what r3g_get_option reports before anything was set)
  alternates  the non-default values worth running
  stages      which workloads of tests/test_switches_gpu.py the switch can affect: cond | dit | vae | geo | mc | attn_op | gemm_op | unet
  promise     "bits" (include/r3g.h: "changes no result bit") or "tol" (same function, other rounding: the stage's existing tolerance
              against the fp32 oracle applies); a dict {stage: promise, "*": promise} where the header distinguishes stages
  differs     stages whose output the header says DOES change under the alternate ("tol" rows: asserted not bit-equal there)
  promise_by_alt / differs_by_alt   the same for one alternate that the header treats differently from the others
  counter     what proves that the switch was obeyed: a list of (counter name, expectation, stage or None = every stage), expectation
              "moves" | "stays" | an exact increment, or a dict {alternate: expectation}; read across the run under the alternate
  with_       further switches set for the baseline AND the alternate run: thresholded switches act only from a size the small
              workloads do not reach, so the threshold comes down (gemm_num_cu, attn_wide_min) instead of the workload going up
  gemm / attn shape and epilogues of the op-level workload where the default one cannot reach the switch (the rule is written beside it)
  refused     a value r3g_set_option refuses or ignores: the old value stays in force
  excluded    a written reason: the row is only checked for set / get / restore
"""
import contextlib

GEMM_DEFAULT = (515, 768, 1024)        # tests/test_ops_gpu.py's ragged residual shape
# launch_epi takes 256 x 256 tiles under the automatic rule only from t256 >= 128 tiles: M = 8192, N = 1024 are 32 x 4 = 128 of them.
# With gemm_num_cu = 128 they are exactly one full round (fills, and 128 * 100 >= 128 * 85: rule 2's "wide enough"), K = 256 < 2048.
GEMM_T256 = (8192, 1024, 256)
ATTN_DEFAULT = (1, 2, 300, 129)        # tests/test_ops_gpu.py's ragged attention shape: (B, H, Lq, Lk)

ROWS = {
    # ---- model-side forms ------------------------------------------------------------------------------------------------------------
    "fuse_qkv": dict(default=1, alternates=(0,), stages=("cond", "dit", "vae", "geo"), promise="tol", differs=("dit",)),
    # (batch_mods, group_streams and overlap_mlp regroup launches of kernels that have no launch counter (GEMV, streams): their cases hold
    #  the results to the promise, but nothing observable would tell an ignored switch from an obeyed one)
    "batch_mods": dict(default=1, alternates=(0,), stages=("dit",), promise="tol"),
    "cfg_dedup": dict(default=1, alternates=(0,), stages=("dit",), promise="tol", differs=("dit",)),
    # the dit stage's flow_sample is a 2-entry schedule: one evaluated step and upstream's trailing step with d_sigma = 0
    "skip_zero_step": dict(default=1, alternates=(0,), stages=("dit",), promise="bits", counter=[("dit_evals", 2, "dit")]),
    "geo_q_cache": dict(default=1, alternates=(0,), stages=("geo",), promise="bits", counter=[("geo_q_cache_builds", "stays", "geo")]),
    # the budget is read when the cache is allocated: the geo stage drops the cache first (a query at another resolution), so that the
    # two canonical-pass workloads allocate it again under 1 GiB = 64 passes of 4096 x 1024 x 2 x 2 bytes
    "geo_q_cache_gb": dict(default=-1, alternates=(1,), stages=("geo",), promise="bits", drop_geo_cache=True,
                           counter=[("geo_q_cache_builds", "moves", "geo")]),
    "geo_resid_bf16": dict(default=1, alternates=(0,), stages=("geo",), promise="tol", differs=("geo",),
                           counter=[("geo_lnf_passes", "stays", "geo"), ("geo_lnd_passes", "stays", "geo")]),
    "dit_resid_f16": dict(default=1, alternates=(0,), stages=("dit",), promise="tol", differs=("dit",)),
    "dit_f16_guard": dict(default=1, alternates=(0,), stages=("dit",), promise="bits", counter=[("dit_f16_fallbacks", "stays", "dit")]),
    "gelu_pk": dict(default=1, alternates=(0,), stages=("cond", "dit", "vae", "geo"), promise="tol", differs=("dit", "geo")),
    "geo_fp8": dict(default=0, alternates=(1, 2, 3), stages=("geo",), promise="tol", differs=("geo",), tol_key="grid_logits_fp8",
                    counter=[("geo_lnd_passes", {1: "stays", 2: "stays", 3: "moves"}, "geo")]),
    "group_streams": dict(default=1, alternates=(0,), stages=("dit",), promise="bits"),
    "overlap_mlp": dict(default=0, alternates=(1,), stages=("dit",), promise="bits"),
    "geo_lnd_fused": dict(default=1, alternates=(0,), stages=("geo",), promise="tol", differs=("geo",),
                          counter=[("geo_lnd_passes", "stays", "geo"), ("geo_lnf_passes", "moves", "geo")]),
    "geo_ln3_fold": dict(default=1, alternates=(0,), stages=("geo",), promise="tol", differs=("geo",),
                         counter=[("geo_lnf_passes", "stays", "geo"), ("geo_lnd_passes", "moves", "geo")]),
    # only a narrow geo decoder (width 256) is affected; this fixture's is 1024 wide: nothing may change, no pass may take the fused tail
    "geo_narrow_fused": dict(default=0, alternates=(1,), stages=("geo",), promise="tol", counter=[("geo_narrow_passes", "stays", "geo")]),
    # ---- GEMM ------------------------------------------------------------------------------------------------------------------------
    # (13 = split-K over two workgroups: shape_ok of launch_epi holds for 515 x 768 x 1024 -- K % 256 == 0, N % 256 == 0, 9 tiles.
    #  32 = the deep-ring kernel: one problem with K % 32 == 0, which the op-level GEMM is; a double block's two-problem launches
    #  would leave it for the 8-wave kernel, so it runs at the op level only, like 13)
    "gemm_waves": dict(default=0, alternates=(4, 8, 9, 10, 11, 12, 16, 13, 32), stages=("dit", "gemm_op"), promise="bits",
                       stages_by_alt={13: ("gemm_op",), 32: ("gemm_op",)}, refused=(7,), promise_by_alt={13: "tol"},
                       differs_by_alt={13: ("gemm_op",)},
                       counter=[("gemm_w4_128", {4: "moves"}, None), ("gemm_w8_128", {8: "moves"}, None),
                                ("gemm_two_stage_256", {9: "moves"}, None), ("gemm_256x128", {10: "moves"}, None),
                                ("gemm_phased", {11: "moves"}, None), ("gemm_phased_persistent", {12: "moves"}, None),
                                ("gemm_w16_256", {16: "moves"}, None), ("gemm_splitk2", {13: "moves"}, "gemm_op"),
                                ("gemm_deep_ring", {32: "moves"}, "gemm_op")]),
    # (the group width travels in the kernel's arguments: no host observable tells 0 from 2.  The counter only shows that the kernel the
    #  switch acts in -- the phased one, which rasterises in groups -- was launched; it would move the same way if the switch were dropped)
    "gemm_raster": dict(default=-1, alternates=(0, 2), stages=("dit", "gemm_op"), promise="bits", gemm=GEMM_T256,
                        with_={"gemm_num_cu": 128}, counter=[("gemm_phased", "moves", "gemm_op")]),
    # rule 2 differs from rules 1 and 0 only in "wide enough": GEMM_T256 under gemm_num_cu = 128 takes the phased kernel by rule 2 alone
    "gemm_auto_rule": dict(default=2, alternates=(1, 0), stages=("gemm_op",), promise="bits", gemm=GEMM_T256, with_={"gemm_num_cu": 128},
                           counter=[("gemm_phased", "stays", None), ("gemm_w8_128", "moves", None)]),
    # 8 CUs: every 256 x 256 grid of the DiT has more tiles than CUs -> the persistent forms, and the single block's mixed launch
    "gemm_num_cu": dict(default=256, alternates=(8,), stages=("dit", "geo", "gemm_op"), promise="bits", refused=(0,),
                        counter=[("gemm_phased_persistent", "moves", "dit"), ("gemm_mixed", "moves", "dit")]),
    # stores only -- but the folded geo epilogues exist in the wide form alone: the geo decoder then runs rounds 1-5's launches; and the
    # narrow fp32 read-modify-write epilogue forms old + gate * (acc + bias) with one fused multiply-add where the wide one rounds the
    # product on its way through LDS: every stage with an fp32 residual stream (conditioner, plain-batch DiT forward, VAE) moves by
    # an fp32 rounding per residual GEMM; the bf16-output op-level GEMM keeps its bits
    "gemm_wide_epilogue": dict(default=1, alternates=(0,), stages=("cond", "dit", "vae", "geo", "gemm_op"),
                               promise={"gemm_op": "bits", "*": "tol"}, differs=("geo", "cond", "dit"),
                               counter=[("geo_lnf_passes", "stays", "geo"), ("geo_lnd_passes", "stays", "geo")]),
    "gemm_phased": dict(default=1, alternates=(0,), stages=("gemm_op",), promise="bits", gemm=GEMM_T256, with_={"gemm_num_cu": 128},
                        counter=[("gemm_phased", "stays", None), ("gemm_two_stage_256", "moves", None)]),
    # 128 tiles on 8 CUs: 16 full rounds (fills), bf16 output, K >= 256 -> the persistent form unless the switch forbids it
    "gemm_persistent": dict(default=1, alternates=(0,), stages=("dit", "gemm_op"), promise="bits", gemm=GEMM_T256, with_={"gemm_num_cu": 8},
                            counter=[("gemm_phased_persistent", "stays", None), ("gemm_phased", "moves", None), ("gemm_mixed", "stays", "dit")]),
    # the read-modify-write epilogues on the persistent form: bit 0 admits the fp32 one (epilogue 3), bit 1 the bf16 one (epilogue 6);
    # the op workload runs both epilogues, so the persistent counter moves by the number of admitted ones
    "gemm_persistent_resid": dict(default=0, alternates=(1, 2, 3), stages=("gemm_op",), promise="bits", gemm=GEMM_T256, gemm_epis=(3, 6),
                                  with_={"gemm_num_cu": 8}, counter=[("gemm_phased_persistent", {1: 1, 2: 1, 3: 2}, None)]),
    "gemm_xcd_walk": dict(default=1, alternates=(0,), stages=("dit", "gemm_op"), promise="bits", gemm=GEMM_T256, with_={"gemm_num_cu": 8},
                          counter=[("gemm_phased_persistent", "moves", None)]),
    # launch_epi: fp32 residual epilogue, K >= 2048, K % 256 == 0, N % 256 == 0 and num_cu / 2 < 2 * tiles <= num_cu: 512 x 512 are 4
    # tiles of 256 x 256, with gemm_num_cu = 8.  Two workgroups per tile each sum half of K: another order of the fp32 additions
    "gemm_splitk": dict(default=0, alternates=(1,), stages=("gemm_op",), promise="tol", differs=("gemm_op",), gemm=(512, 512, 2048),
                        gemm_epis=(3,), with_={"gemm_num_cu": 8}, counter=[("gemm_splitk2", "moves", None)]),
    # r3g_op_gemm_splitk's rule: <= 256 tiles of 128 x 128, K >= 2048 -> 256 x 256 x 2048 runs as 4 slices of 8 k-steps.  The smallest
    # resnet block's convolutions have K = 576: no split either way, so nothing may change there
    "gemm_splitk128": dict(default=1, alternates=(0,), stages=("gemm_op", "unet"), promise="tol", differs=("gemm_op",), gemm=(256, 256, 2048),
                           gemm_epis=(4,), gemm_splitk_ws=True, counter=[("gemm_splitk128", "stays", None)]),
    "conv_implicit": dict(default=1, alternates=(0,), stages=("unet",), promise="bits", counter=[("gemm_conv_implicit", "stays", None)]),
    "gemm_epi_slices": dict(default=1, alternates=(0,), stages=("dit",), promise="bits", with_={"gemm_num_cu": 8},
                            counter=[("gemm_phased_persistent", "moves", None), ("gemm_mixed", "moves", None)]),
    "gemm_mixed": dict(default=1, alternates=(0,), stages=("dit",), promise="bits", with_={"gemm_num_cu": 8},
                       counter=[("gemm_mixed", "stays", None), ("gemm_phased_persistent", "moves", None)]),
    "gemm_persistent_qkv": dict(default=1, alternates=(0,), stages=("dit",), promise="bits", with_={"gemm_num_cu": 8},
                                counter=[("gemm_mixed", "stays", None), ("gemm_phased", "moves", None)]),
    # ---- staging ---------------------------------------------------------------------------------------------------------------------
    # the tile kernels and the attention stage through registers; the phased GEMM kernels have no such form (and with it no folded geo
    # epilogues: the geo decoder runs rounds 1-5's launches) and the 3 x 3 convolutions fall back to im2col + GEMM
    # The register-staged attention kernel is the "attn_variant" 0 body: that switch's stated corner (the weighted key of the
    # de-duplicated CFG context moves variant 0's stabiliser) comes with it -- tests/test_switches_gpu.py holds the two equal bit for bit
    "lds_dma": dict(default=1, alternates=(0,), stages=("cond", "dit", "vae", "geo", "attn_op", "gemm_op", "unet"),
                    promise={"geo": "tol", "dit": "tol", "*": "bits"}, differs=("geo",),
                    counter=[("gemm_register_staged", "moves", "dit"), ("gemm_register_staged", "moves", "gemm_op"),
                             ("attn_register_staged", "moves", "attn_op"), ("attn_register_staged", "moves", "dit"),
                             ("gemm_conv_implicit", "stays", "unet"), ("geo_lnf_passes", "stays", "geo"), ("geo_lnd_passes", "stays", "geo")]),
    # ---- attention -------------------------------------------------------------------------------------------------------------------
    # the stated corner is met on the DiT stage: the weighted key of the de-duplicated unconditional context (+log2(1370) on its score)
    # moves variant 0's stabiliser where the fast pass keeps its own, so flow_sample's latents differ there (and only there)
    "attn_variant": dict(default=1, alternates=(0,), stages=("dit", "vae", "geo", "attn_op"), promise="tol", differs=("dit",), refused=(2,)),
    # (attn_interleave acts in the 64-query kernel = generation 6: 300 queries x 2 heads are 4 work items of 256 queries, attn_wide_min 1)
    "attn_interleave": dict(default=0, alternates=(1,), stages=("attn_op", "geo"), promise="bits", with_={"attn_wide_min": 1},
                            counter=[("attn_gen6", "moves", None)]),
    "attn_async_stage": dict(default=1, alternates=(0,), stages=("dit", "attn_op"), promise="bits", counter=[("attn_gen2", "moves", None)]),
    "attn_pipelined": dict(default=0, alternates=(1,), stages=("dit", "attn_op"), promise="tol", differs=("attn_op",),
                           counter=[("attn_pipelined", "moves", None), ("attn_gen2", "stays", None)]),
    "attn_generation": dict(default=7, alternates=(1, 2, 3, 4, 5, 6, 9), stages=("dit", "attn_op"), promise="tol", refused=(8,),
                            stages_by_alt={3: ("attn_op",), 4: ("attn_op",), 5: ("attn_op",)},
                            counter=[("attn_gen1", {1: "moves"}, None), ("attn_gen2", {2: "moves", 6: "stays"}, None),
                                     ("attn_gen3", {3: "moves"}, None), ("attn_gen4", {4: "moves"}, None), ("attn_gen5", {5: "moves"}, None),
                                     ("attn_gen6", {6: "moves"}, None), ("attn_gen9", {9: "moves"}, None)]),
    # (the priority picks one of three instantiations of ONE kernel: the counter shows that generation 9, where the switch acts, was
    #  launched, not which instantiation -- it would move the same way if the switch were dropped)
    "attn_prio": dict(default=1, alternates=(0, 2), stages=("attn_op",), promise="bits", with_={"attn_generation": 9}, refused=(3,),
                      counter=[("attn_gen9", "moves", None)]),
    # generation 7 takes generation 6 from attn_wide_min work items of 256 queries on: the threshold comes down to the ragged shape's 4
    "attn_wide_min": dict(default=2048, alternates=(1,), stages=("attn_op", "dit"), promise="bits", refused=(0,),
                          counter=[("attn_gen6", "moves", None), ("attn_gen2", "stays", "attn_op")]),
    # ---- row kernels -----------------------------------------------------------------------------------------------------------------
    "ln_modes": dict(default=1, alternates=(0,), stages=("cond", "dit", "vae", "geo"), promise="bits", counter=[("ln_mode_inst", "stays", None)]),
    "ln_rows": dict(default=0, alternates=(1, 4), stages=("cond", "dit", "vae", "geo"), promise="bits",
                    counter=[("ln_rows1", {1: "moves", 4: "stays"}, None), ("ln_rows4", {1: "stays", 4: "moves"}, None)]),
    # 4 rows per wave from 1024 rows on: the conditioner's 1370-row, the VAE's 3072-row, the DiT's 4442-row launches and the geo decoder's
    # 3000-row slice take them (none of them reaches the default 65536)
    "ln_rows4_min": dict(default=65536, alternates=(1024,), stages=("cond", "dit", "vae", "geo"), promise="bits",
                         counter=[("ln_rows4", "moves", None)]),
    "ln_fixed": dict(default=1, alternates=(0,), stages=("cond", "dit", "vae", "geo"), promise="bits", counter=[("ln_fixed_count", "stays", None)]),
    # the row-marching kernel runs where the row length is a multiple of 256 (+ 1 node).  tests/mc_volumes.py's only such volume is the
    # 257^3 sphere "D"; the mc stage takes tests/test_mc_gpu.py's row-kernel shape 5 x 19 x 257 instead (19 rows: more than one group of
    # 4, 8 or 16 rows and a partial one), and the counters show that the row kernel ran with the rows asked for
    "mc_rows": dict(default=16, alternates=(4, 8, 32), stages=("mc",), promise="bits",
                    counter=[("mc_rows4", {4: "moves"}, None), ("mc_rows8", {8: "moves"}, None), ("mc_rows32", {32: "moves"}, None),
                             ("mc_rows16", "stays", None)]),
    "mc_deferred": dict(default=1, alternates=(0,), stages=("mc",), promise="bits",
                        counter=[("mc_deferred_rows", "stays", None), ("mc_rows16", "moves", None)]),
    # ---- set / get / restore only ----------------------------------------------------------------------------------------------------
    "attn_ablate": dict(default=0, alternates=(1,), stages=(), promise="bits", excluded="timing-only masks: the results are garbage by design"),
    "attn_stamps": dict(default=0, alternates=(1,), stages=(), promise="bits", excluded="prints per-phase ticks to stderr and makes the launch synchronous"),
    "flow_first_step": dict(default=0, alternates=(1,), stages=(), promise="bits", excluded="covered by tests/test_cfg1_golden_gpu.py"),
    "flow_last_step": dict(default=-1, alternates=(1,), stages=(), promise="bits", excluded="covered by tests/test_cfg1_golden_gpu.py"),
    "geo_kv_topk": dict(default=0, alternates=(512, -1), stages=(), promise="tol", refused=(-2,), excluded="covered by tests/test_kvsel_gpu.py"),
    "geo_kv_group": dict(default=8192, alternates=(256,), stages=(), promise="tol", refused=(100, 0), excluded="covered by tests/test_kvsel_gpu.py"),
    "geo_kv_stride": dict(default=64, alternates=(1,), stages=(), promise="tol", refused=(0,), excluded="covered by tests/test_kvsel_gpu.py"),
    "floater_by_vertex": dict(default=0, alternates=(1,), stages=(), promise="tol",
                              excluded="another definition of a connected component (rounds 1-2), not another kernel for the same function: "
                                       "tests/test_mesh_gpu.py compares both with their oracles"),
}

STAGES = ("cond", "dit", "vae", "geo", "mc", "attn_op", "gemm_op", "unet")


def promise_of(row, stage, alt=None):
    p = row.get("promise_by_alt", {}).get(alt, row["promise"])
    return p if isinstance(p, str) else p.get(stage, p["*"])


def differs_of(row, alt=None):
    """stages whose output must NOT equal the default-switch result under this alternate"""
    return row.get("differs_by_alt", {}).get(alt, row.get("differs", ()))


def stages_of(row, alt):
    return row.get("stages_by_alt", {}).get(alt, row["stages"])


def counter_checks(row, alt, stage):
    """[(counter name, "moves" | "stays" | exact increment)] that apply to this alternate on this stage"""
    out = []
    for name, expect, where in row.get("counter", ()):
        if where is not None and where != stage:
            continue
        if isinstance(expect, dict):
            if alt not in expect:
                continue
            expect = expect[alt]
        out.append((name, expect))
    return out


def cases():
    """every (name, alternate) of the rows that are run on the GPU"""
    return [(n, a) for n, r in ROWS.items() if not r.get("excluded") for a in r["alternates"]]


def get_option(L, ffi, name):
    return ffi.option(name)


def get_counter(L, ffi, name):
    return ffi.counter(name)


def set_option(L, ffi, name, value):
    ffi.check(L.r3g_set_option(name.encode(), int(value)))


def not_at_default(L, ffi):
    """{name: (current, default)} of every switch that is not at its default"""
    return {n: (get_option(L, ffi, n), r["default"]) for n, r in ROWS.items() if get_option(L, ffi, n) != r["default"]}


def restore_defaults(L, ffi):
    for n, r in ROWS.items():
        set_option(L, ffi, n, r["default"])


@contextlib.contextmanager
def switched(L, ffi, **values):
    """set the given switches, yield, and put back what r3g_get_option reported before -- also when the body raises"""
    old = {n: get_option(L, ffi, n) for n in values}
    try:
        for n, v in values.items():
            set_option(L, ffi, n, v)
        yield
    finally:
        for n, v in reversed(list(old.items())):
            set_option(L, ffi, n, v)
