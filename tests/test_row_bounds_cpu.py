"""The element-wise bounds of tests/row_bounds.py are neither vacuous nor unreachable -- shown without a GPU and without the library.

REACHABLE: for every row kernel an emulation written here in float32 torch -- the same operations in the kernel's order, the lane -> element
map of the kernel, the wave tree as a pairwise sum (xor 32, 16, ... 1), fused multiply-adds where the kernel spells them out -- stays inside
the bound at EVERY element of every shape and operand set the GPU tests launch.  No element is excluded from any comparison.
NOT VACUOUS: each mutant below, applied to the emulation, breaks the bound at at least one element wherever it applies.

Where a mutant applies, and what is out of reach:
  * eps_outside (1 / (sqrt(var) + eps)) moves rstd by eps / sqrt(var) ~ 1e-6 relative on a row of variance ~1: far inside a bf16 ulp.  It
    is visible where eps matters -- the row of variance 1e-6 and the constant row, which every operand set of five rows or more holds.
  * drop_last_chunk needs a second chunk (C >= 512 on the row-in-registers kernel, C >= 128 on the scalar one): the statistics skip the
    last 256 (64) columns.
  * scale_not_1p needs a scale, affine_after_mod both pairs, seg2_end and stale_mod their row configurations; stale_mod also needs a
    per-batch vector (the first row of a batch then takes the previous batch's).
  * truncate: an element shows a truncating store with probability about one half; rows * C >= 64 everywhere, so draw 0 shows it.
  * softmax, unscaled_max (the maximum subtracted without the scale): a common factor of every exponential, which CANCELS in p unless an
    exponential leaves the float32 range.  With scores of standard deviation 3 / scale it does from n = 1020 on (the maximum is ~ 3.3
    deviations out: every exponential underflows), not at n = 4, and never on a row of equal scores: asserted from n = 1020 on.
  * GEGLU with the tanh form of GELU in place of erf: the two differ by up to 4.7e-4 around |x| = 2, a quarter of a bf16 half-ulp there --
    unlike the GEMM's packed-GELU case (tests/test_mutation_cpu.py) it IS visible from 72 columns on (an element shows it when the shift
    crosses a rounding boundary); at F = 8 (8 or 24 outputs) it is a property of the draw and is pooled over 16 operand sets.
  * GroupNorm, unbiased variance needs more than one value per group ((1, 32, 32) has one: n - 1 = 0).  group_first_channel needs
    channels-per-group % 4 != 0.
"""
import pytest
import torch

import row_bounds as RB


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def tree(v):
    """wave_sum: the xor butterfly over the last (64-lane) dimension, every level one float32 addition"""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def truncate_bf16(y32):
    return (y32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def to_e4m3(x):
    """float32 -> e4m3 code, round to nearest even, saturating (v_cvt_pk_fp8_f32)"""
    pos = RB.E4M3[:127].float()                       # codes 0 .. 126 ascending, 126 = 448
    a = x.abs().clamp_max(448.0)
    hi = torch.searchsorted(pos, a.contiguous()).clamp(1, 126)
    lo = hi - 1
    dl, dh = a - pos[lo], pos[hi] - a
    code = torch.where((dl < dh) | ((dl == dh) & (lo % 2 == 0)), lo, hi)
    return (code + 128 * (x < 0)).to(torch.uint8)


# ---- LayerNorm / ln_dot -----------------------------------------------------------------------------------------------------------------
def emu_row_stats(x, C, eps, vec, mutant=None):
    """(mean, rstd) float32 [rows][1] as layernorm_kernel (vec) / layernorm_small_kernel compute them"""
    rows = x.shape[0]
    if vec:
        v = x.view(rows, C // 256, 64, 4)
        ng = v.shape[1] - (1 if mutant == "drop_last_chunk" else 0)
        s = torch.zeros(rows, 64)
        for i in range(ng):
            s = s + (((v[:, i, :, 0] + v[:, i, :, 1]) + v[:, i, :, 2]) + v[:, i, :, 3])
        mean = (tree(s) / C)[:, None]
        ss = torch.zeros(rows, 64)
        for i in range(ng):
            for e in range(4):
                d = v[:, i, :, e] - mean
                ss = fma(d, d, ss)
    else:
        v = x.view(rows, C // 64, 64)
        ng = v.shape[1] - (1 if mutant == "drop_last_chunk" else 0)
        s = torch.zeros(rows, 64)
        for i in range(ng):
            s = s + v[:, i]
        mean = (tree(s) / C)[:, None]
        ss = torch.zeros(rows, 64)
        for i in range(ng):
            d = v[:, i] - mean
            ss = ss + d * d
    var = tree(ss) / (C - 1 if mutant == "var_cm1" else C)
    eps = torch.tensor(eps, dtype=torch.float32)
    rstd = 1.0 / (torch.sqrt(var) + eps) if mutant == "eps_outside" else torch.rsqrt(var + eps)
    return mean, rstd[:, None]


def emu_layernorm(case, mutant=None, fp8=False):
    C, rows, rpb = case["C"], case["rows"], case["rpb"]
    x = case["x"]
    mean, rstd = emu_row_stats(x, C, case["eps"], C % 256 == 0, mutant)
    o = (x - mean) * rstd
    sc_rows, sh_rows, has_sc, has_sh = case["sc_rows"].clone(), case["sh_rows"].clone(), case["has_sc"].clone(), case["has_sh"].clone()
    if mutant == "seg2_end":
        r1 = case["seg2"][1]
        sc_rows[r1], sh_rows[r1], has_sc[r1], has_sh[r1] = case["scale2"], case["shift2"], True, True
    if mutant == "stale_mod":
        for r in range(rpb, rows, rpb):             # the first row of every batch but the first keeps the previous batch's vectors
            sc_rows[r], sh_rows[r] = sc_rows[r - 1], sh_rows[r - 1]

    def affine(o):
        if case["w"] is not None:
            o = o * case["w"]
        if case["b"] is not None:
            o = o + case["b"]
        return o

    def modulate(o):
        o = torch.where(has_sc[:, None], o * (sc_rows if mutant == "scale_not_1p" else (1.0 + sc_rows)), o)
        return torch.where(has_sh[:, None], o + sh_rows, o)

    o = affine(modulate(o)) if mutant == "affine_after_mod" else modulate(affine(o))
    if not fp8:
        return truncate_bf16(o) if mutant == "truncate" else o.to(torch.bfloat16)
    amax = o.abs().amax(-1)
    k = torch.tensor(1.0 / (240.0 if mutant == "fp8_amax240" else 448.0), dtype=torch.float32)
    qs = torch.where(amax > 0, amax * k, torch.ones_like(amax))
    inv = 1.0 / qs
    return to_e4m3(o * inv[:, None]), qs


def ln_applies(mutant, C, rowcfg, combo):
    name, rows, rpb, seg2 = rowcfg
    return {"var_cm1": True, "eps_outside": rows >= 5, "scale_not_1p": combo in ("mod", "affine_mod", "scale_only") or bool(seg2),
            "affine_after_mod": combo == "affine_mod", "seg2_end": bool(seg2), "stale_mod": rpb < rows and combo in ("mod", "affine_mod", "scale_only"),
            "drop_last_chunk": C >= 512 if C % 256 == 0 else C >= 128, "truncate": True}[mutant]


LN_MUTANTS = ("var_cm1", "eps_outside", "scale_not_1p", "affine_after_mod", "seg2_end", "stale_mod", "drop_last_chunk", "truncate")


@pytest.mark.parametrize("C", RB.LN_C)
def test_layernorm_emulation_is_inside_the_bound_everywhere(C):
    worst = 0.0
    for xf in RB.ln_formats(C):
        for rc in RB.LN_ROWCFGS:
            for combo in RB.LN_COMBOS:
                case = RB.ln_case(C, xf, rc, combo)
                ref, bound = RB.ln_ref_bound(case)
                r = RB.worst_ratio(emu_layernorm(case), ref, bound)
                worst = max(worst, r)
                assert r <= 1.0, "C %d format %d %s %s: error / bound %.3f" % (C, xf, rc[0], combo, r)
    print("layernorm C %d: largest error / bound of the emulation %.3f" % (C, worst))
    assert worst > 0.5          # a rounding tie is near: the bf16 bound is met tightly


@pytest.mark.parametrize("mutant", LN_MUTANTS)
def test_layernorm_mutants_break_the_bound(mutant):
    ran = 0
    for C in RB.LN_C:
        for xf in (RB.ln_formats(C) if C == 256 else (0,)):
            for rc in RB.LN_ROWCFGS:
                for combo in RB.LN_COMBOS:
                    if not ln_applies(mutant, C, rc, combo):
                        continue
                    case = RB.ln_case(C, xf, rc, combo)
                    ref, bound = RB.ln_ref_bound(case)
                    r = RB.worst_ratio(emu_layernorm(case, mutant), ref, bound)
                    assert r > 1.0, "%s is invisible at C %d format %d %s %s: error / bound %.3f" % (mutant, C, xf, rc[0], combo, r)
                    ran += 1
    assert ran >= 7


FP8_CASES = [(C, xf, rc, combo) for C in (256, 1024) for xf in (0, 1, 2) for rc in RB.LN_ROWCFGS[1:3] for combo in ("none", "affine_mod")]


def test_layernorm_e4m3_emulation_is_inside_and_amax_240_is_not():
    for C, xf, rc, combo in FP8_CASES:
        case = RB.ln_case(C, xf, rc, combo, zero_row=2)
        re = RB.ln_ref_err(case)
        codes, qs = emu_layernorm(case, fp8=True)
        rs, rc_, zeros_ok = RB.ln_fp8_check(case, codes, qs, re)
        assert rs <= 1.0 and rc_ <= 1.0 and zeros_ok, (C, xf, rc[0], combo, rs, rc_, zeros_ok)
        if combo == "none":
            assert float(qs[2]) == 1.0 and int(codes[2].max()) == 0          # the all-zero row
        codes, qs = emu_layernorm(case, "fp8_amax240", fp8=True)
        rs, rc_, _ = RB.ln_fp8_check(case, codes, qs, re)
        assert rs > 1.0, "a scale of amax / 240 is invisible at %s" % ((C, xf, rc[0], combo),)
        codes, qs = emu_layernorm(case, "var_cm1", fp8=True)
        rs, rc_, _ = RB.ln_fp8_check(case, codes, qs, re)
        assert max(rs, rc_) > 1.0


def emu_ln_dot(case, mutant=None):
    C, rows = case["C"], case["rows"]
    x, w = case["x"], case["w"]
    vec = C % 256 == 0
    if case["do_ln"]:
        mean, rstd = emu_row_stats(x, C, case["eps"], vec, mutant)
        o = (x - mean) * rstd
        if case["affine"]:
            o = fma(o, case["lnw"].expand_as(o), case["lnb"].expand_as(o)) if vec else o * case["lnw"] + case["lnb"]
    else:
        o = x
    acc = torch.zeros(rows, 64)
    if vec:
        ov, wv = o.view(rows, C // 256, 64, 4), w.view(C // 256, 64, 4).expand(rows, -1, -1, -1)
        for i in range(C // 256):
            t = ov[:, i, :, 0] * wv[:, i, :, 0]
            for e in (1, 2, 3):
                t = fma(ov[:, i, :, e], wv[:, i, :, e], t)
            acc = acc + t
    else:
        ov, wv = o.view(rows, C // 64, 64), w.view(C // 64, 64)
        for i in range(C // 64):
            acc = acc + ov[:, i] * wv[i]
    return tree(acc) + torch.tensor(case["b"], dtype=torch.float32)


def lnd_cases():
    for C in RB.LND_C:
        for xb in ((0, 1) if C % 256 == 0 else (0,)):
            for rows in RB.LND_ROWS:
                for do_ln in (0, 1):
                    for affine in ((0, 1) if do_ln else (0,)):
                        yield C, xb, rows, do_ln, affine


def test_ln_dot_emulation_is_inside_and_its_mutants_are_not():
    """A launch has `rows` outputs (17 at most), and a mutant that rescales a row moves its output by that factor times the dot product
    itself, which is small wherever the terms happen to cancel while the bound is in absolute values: every shape is pooled over eight operand sets."""
    worst, ran = 0.0, 0
    for C, xb, rows, do_ln, affine in lnd_cases():
        seen = {"var_cm1": 0.0, "eps_outside": 0.0, "drop_last_chunk": 0.0}
        for draw in range(8):
            case = RB.lnd_case(C, xb, rows, do_ln, affine, draw=draw)
            ref, bound = RB.lnd_ref_bound(case)
            r = RB.worst_ratio(emu_ln_dot(case), ref, bound)
            worst = max(worst, r)
            assert r <= 1.0, (C, xb, rows, do_ln, affine, draw, r)
            if do_ln:
                for mutant in seen:
                    seen[mutant] = max(seen[mutant], RB.worst_ratio(emu_ln_dot(case, mutant), ref, bound))
        if not do_ln:
            continue
        for mutant, rm in seen.items():
            if (mutant == "eps_outside" and rows < 5) or (mutant == "drop_last_chunk" and not (C >= 512 if C % 256 == 0 else C >= 128)):
                continue
            assert rm > 1.0, "%s is invisible at %s: error / bound %.3f" % (mutant, (C, xb, rows, do_ln, affine), rm)
            ran += 1
    print("ln_dot: largest error / bound of the emulation %.4f" % worst)
    assert ran >= 20 and worst > 1e-3


# ---- qkv_split ----------------------------------------------------------------------------------------------------------------------------
def emu_qkv(case, mutant=None):
    """{"q": bf16 [B][H][L][64], "k": ..., "vt": bf16 [B][H][64][n]} of the operands present"""
    eps = torch.tensor(case["eps"], dtype=torch.float32)
    out = {}

    def norm(x, wt, bs, kind):
        if kind == 1:
            r = torch.rsqrt(tree(x * x) * (1.0 / 64.0) + eps)[..., None]
            return x * r * (wt if wt is not None else 1.0)
        mean = (tree(x) * (1.0 / 64.0))[..., None]
        d = x - mean
        r = torch.rsqrt(tree(d * d) * (1.0 / 64.0) + eps)[..., None]
        return d * r * (wt if wt is not None else 1.0) + (bs if bs is not None else 0.0)

    kind = 1 if (mutant == "rms_for_ln" and case["norm"] == 2) else case["norm"]
    for which, off, wt, bs in (("q", case["q_off"], case["qw"], case["qb"]), ("k", case["k_off"], case["kw"], case["kb"])):
        if off < 0:
            continue
        x = RB.qkv_heads(case, off).float()
        qs = torch.tensor(case["q_scale"], dtype=torch.float32)
        scaled = which == "q" and case["q_scale"] != 0.0
        if scaled and mutant == "qscale_before_norm":
            x = x * qs
        if kind:
            x = norm(x, wt, bs if kind == 2 else None, kind)
        if scaled and mutant != "qscale_before_norm":
            x = x * qs
        out[which] = x.to(torch.bfloat16)
    if case["v_off"] >= 0:
        _, vt = RB.qkv_vt_expected(case, 0)
        L, n = case["L"], vt.shape[-1]
        if mutant == "no_vt_key_pos":
            vt = torch.zeros_like(vt)
            vt[..., :L] = RB.qkv_heads(case, case["v_off"]).to(torch.bfloat16).transpose(-1, -2)
        if mutant == "pad_not_zeroed" and L < n:
            vt = vt.clone()
            vt[..., RB.vt_positions(n)[L:]] = RB.qkv_heads(case, case["v_off"]).to(torch.bfloat16)[:, :, 0, :, None]      # token 0 where zeros belong
        out["vt"] = vt
    return out


def qkv_cases():
    for L in RB.QKV_L:
        for B, H in RB.QKV_BH:
            for layout in RB.QKV_LAYOUTS:
                for norm, weights in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
                    for q_scale in RB.QKV_QSCALE:
                        yield L, B, H, layout, norm, weights, q_scale


def qkv_ratio(case, got):
    """(worst error / bound over Q and K, V^T equal to the bit)"""
    r = 0.0
    for which in ("q", "k"):
        if which in got:
            ref, bound = RB.qkv_norm_ref_bound(case, which)
            r = max(r, RB.worst_ratio(got[which], ref, bound))
    vt_ok = True
    if "vt" in got:
        vt_ok = torch.equal(got["vt"].view(torch.int16), RB.qkv_vt_expected(case, 0)[1].view(torch.int16))
    return r, vt_ok


def test_qkv_split_emulation_is_inside_and_its_mutants_are_not():
    worst, ran = 0.0, {m: 0 for m in ("rms_for_ln", "qscale_before_norm", "no_vt_key_pos", "pad_not_zeroed")}
    for L, B, H, layout, norm, weights, q_scale in qkv_cases():
        case = RB.qkv_case(L, B, H, layout, norm, weights, q_scale)
        r, vt_ok = qkv_ratio(case, emu_qkv(case))
        worst = max(worst, r)
        assert r <= 1.0 and vt_ok, (L, B, H, layout, norm, weights, q_scale, r, vt_ok)
        has_q, has_v = case["q_off"] >= 0, case["v_off"] >= 0
        applies = {"rms_for_ln": norm == 2, "qscale_before_norm": has_q and norm != 0 and q_scale != 0.0,
                   "no_vt_key_pos": has_v and L > 4, "pad_not_zeroed": has_v and L % 64 != 0}
        for mutant, ok in applies.items():
            if not ok:
                continue
            rm, vm = qkv_ratio(case, emu_qkv(case, mutant))
            assert rm > 1.0 or not vm, "%s is invisible at %s" % (mutant, (L, B, H, layout, norm, weights, q_scale))
            ran[mutant] += 1
    print("qkv_split: largest error / bound of the emulation %.3f" % worst)
    assert min(ran.values()) >= 8 and worst > 0.5


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------------
def emu_group_norm(case, silu, mutant=None):
    rows, C, G, nb = case["rows"], case["C"], case["groups"], case["nb"]
    geo = RB.gn_geometry(rows, C)
    nblk, rpb, P, m = geo["nblk"], geo["rpb"], geo["P"], geo["m"]
    cpg = C // G
    x = case["x"]
    z = x + case["addv"][:, None, :C] if case["addv"] is not None else x
    zs = x if mutant == "addv_not_in_stats" else z
    # pass 1: float32 sums per (block, row lane, channel), rows ascending; a missing row adds an exact zero
    b_, p_, t_ = torch.meshgrid(torch.arange(nblk), torch.arange(P), torch.arange(m), indexing="ij")
    local = p_ + t_ * P
    row = b_ * rpb + local
    valid = (local < rpb) & (row < rows)
    zp = torch.cat([zs, torch.zeros(nb, 1, C)], 1)[:, torch.where(valid, row, torch.full_like(row, rows))]      # [nb][nblk][P][m][C]
    acc, acc2 = torch.zeros(nb, nblk, P, C), torch.zeros(nb, nblk, P, C)
    for t in range(m):
        acc = acc + zp[:, :, :, t]
        acc2 = fma(zp[:, :, :, t], zp[:, :, :, t], acc2)
    s = acc.double().sum((1, 2)).view(nb, G, cpg).sum(-1)
    ss = acc2.double().sum((1, 2)).view(nb, G, cpg).sum(-1)
    n = float(rows * cpg)
    mean = s / n
    var = (ss / n - mean * mean).clamp_min(0.0)
    if mutant == "unbiased":
        var = var * n / (n - 1.0)
    mu = mean.float()
    rs = (1.0 / torch.sqrt(var + case["eps"])).float()
    grp = torch.arange(C) // cpg
    if mutant == "group_first_channel":
        grp = (torch.arange(C) // 4 * 4) // cpg
    o = (z - mu[:, grp][:, None]) * rs[:, grp][:, None] * case["gamma"] + case["beta"]
    if silu and mutant != "silu_missing":
        o = o / (1.0 + torch.exp(-o))
    return o.to(torch.bfloat16)


def test_group_norm_emulation_is_inside_and_its_mutants_are_not():
    worst, ran = 0.0, {m: 0 for m in ("group_first_channel", "unbiased", "addv_not_in_stats", "silu_missing")}
    for rows, C, G, _ in RB.GN_SHAPES:
        for nb in (1, 3):
            for addv in (0, 1):
                case = RB.gn_case(rows, C, G, nb, addv)
                for silu in (0, 1):
                    ref, bound = RB.gn_ref_bound(case, silu)
                    r = RB.worst_ratio(emu_group_norm(case, silu), ref, bound)
                    worst = max(worst, r)
                    assert r <= 1.0, (rows, C, G, nb, addv, silu, r)
                    applies = {"group_first_channel": (C // G) % 4 != 0, "unbiased": rows * (C // G) > 1, "addv_not_in_stats": bool(addv),
                               "silu_missing": bool(silu)}
                    for mutant, ok in applies.items():
                        if ok:
                            rm = RB.worst_ratio(emu_group_norm(case, silu, mutant), ref, bound)
                            assert rm > 1.0, "%s is invisible at %s: error / bound %.3f" % (mutant, (rows, C, G, nb, addv, silu), rm)
                            ran[mutant] += 1
    print("group_norm: largest error / bound of the emulation %.3f" % worst)
    assert min(ran.values()) >= 6 and worst > 0.5


def test_group_norm_geometry_covers_every_regime():
    geos = [RB.gn_geometry(rows, C) for rows, C, G, _ in RB.GN_SHAPES]
    assert {g_["cols_per_thread"] for g_ in geos} == {1, 2, 3}
    assert any(g_["P"] > 1 for g_ in geos) and any(g_["P"] == 1 for g_ in geos)
    assert any(g_["capped"] and g_["empty_blocks"] > 0 for g_ in geos)
    assert RB.gn_geometry(4100, 32) == dict(nblk=256, rpb=17, P=32, cols_per_thread=1, m=1, capped=True, empty_blocks=14)


# ---- softmax rows ---------------------------------------------------------------------------------------------------------------------------
def emu_softmax(case, mutant=None):
    rows, n = case["rows"], case["n"]
    s = case["s"]
    sl = torch.tensor(case["scale"], dtype=torch.float32) * torch.tensor(RB.LOG2E32, dtype=torch.float32)
    mx = s.max(-1, keepdim=True).values
    mx = mx if mutant == "unscaled_max" else mx * sl
    e = torch.exp2(fma(s, sl.expand_as(s), -mx.expand_as(s)))
    e = torch.where(e < RB.FLUSH, torch.zeros_like(e), e)          # v_exp_f32 has no denormal results
    npad = (n + 1023) // 1024 * 1024
    ep = torch.zeros(rows, npad)
    ep[:, :(n - 4 if mutant == "sum_n_minus_4" else n)] = e[:, :(n - 4 if mutant == "sum_n_minus_4" else n)]
    ep = ep.view(rows, npad // 1024, 256, 4)
    acc = torch.zeros(rows, 256)
    for k in range(npad // 1024):
        acc = acc + (((ep[:, k, :, 0] + ep[:, k, :, 1]) + ep[:, k, :, 2]) + ep[:, k, :, 3])
    red = tree(acc.view(rows, 4, 64))
    tot = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    return (e * (1.0 / tot)[:, None]).to(torch.bfloat16)


def test_softmax_rows_emulation_is_inside_and_its_mutants_are_not():
    worst = 0.0
    for n in RB.SM_N:
        for rows in RB.SM_ROWS:
            case = RB.sm_case(rows, n)
            ref, bound, zero = RB.sm_ref_bound(case)
            got = emu_softmax(case)
            r = RB.worst_ratio(got, ref, bound)
            worst = max(worst, r)
            assert r <= 1.0 and bool((got[zero].view(torch.int16) == 0).all()), (rows, n, r)
            if rows == 3:
                assert bool(zero[2].any()) or n == 4          # the 300-unit row really holds probabilities that must be zeros
            rm = RB.worst_ratio(emu_softmax(case, "sum_n_minus_4"), ref, bound)
            assert rm > 1.0, "a sum over n - 4 elements is invisible at %s" % ((rows, n),)
            if n >= 1020:
                rm = RB.worst_ratio(emu_softmax(case, "unscaled_max"), ref, bound)
                assert rm > 1.0, "an unscaled maximum is invisible at %s" % ((rows, n),)
    print("softmax_rows: largest error / bound of the emulation %.3f" % worst)
    assert worst > 0.5


# ---- GEGLU / SwiGLU -------------------------------------------------------------------------------------------------------------------------
def emu_glu(case, kind, mutant=None):
    F = case["F"]
    a, b = case["x"][:, :F].float(), case["x"][:, F:].float()
    if mutant == "halves_swapped":
        a, b = b, a
    if kind == "swiglu":
        return ((a / (1.0 + torch.exp(-a))) * b).to(torch.bfloat16)
    if mutant == "tanh_gelu":
        return (a * torch.nn.functional.gelu(b, approximate="tanh")).to(torch.bfloat16)
    t = 1.0 / fma(b.abs(), torch.full_like(b, 0.3275911 * 0.7071067811865476), torch.ones_like(b))
    e = torch.exp2(b * b * -0.7213475204444817)
    h = t * (0.127414796 + t * (-0.142248368 + t * (0.7107068705 + t * (-0.7265760135 + t * 0.5307027145)))) * e
    return (a * (b * torch.where(b >= 0, 1.0 - h, h))).to(torch.bfloat16)


def test_glu_emulations_are_inside_and_their_mutants_are_not():
    for kind in ("geglu", "swiglu"):
        worst = 0.0
        for rows in RB.GLU_ROWS:
            for F in RB.GLU_F:
                draws = range(16) if rows * F < 64 else range(1)          # module docstring: pooled where a shape has few elements
                seen = {"halves_swapped": 0.0, "tanh_gelu": 0.0}
                for draw in draws:
                    case = RB.glu_case(rows, F, draw=draw)
                    ref, bound = RB.glu_ref_bound(case, kind)
                    r = RB.worst_ratio(emu_glu(case, kind), ref, bound)
                    worst = max(worst, r)
                    assert r <= 1.0, (kind, rows, F, draw, r)
                    for mutant in seen:
                        if mutant == "tanh_gelu" and kind != "geglu":
                            continue
                        seen[mutant] = max(seen[mutant], RB.worst_ratio(emu_glu(case, kind, mutant), ref, bound))
                assert seen["halves_swapped"] > 1.0, (kind, rows, F)
                assert kind != "geglu" or seen["tanh_gelu"] > 1.0, "tanh GELU is invisible at %s" % ((rows, F),)
        print("%s: largest error / bound of the emulation %.3f" % (kind, worst))
        assert worst > 0.5


# ---- the restated launch rules -----------------------------------------------------------------------------------------------------------
def test_layernorm_plan_reaches_every_form():
    reached = set()
    for C, xf, (rpw, fixed, modes), rc, combo in RB.ln_plan():
        f = RB.ln_form(C, xf, C + RB.LN_PAD, C + RB.LN_PAD, RB.combo_has(combo, rc[3]), rc[1], rpw, fixed, modes, seg2=bool(rc[3]))
        assert rc[1] % (4 * f["rpw"]) != 0          # every launch ends in a partial workgroup: a row tail
        reached.add((f["kernel"], f["nv"], f["mode"], f["rpw"], xf))
    assert RB.ln_forms_required() <= reached
    f = RB.ln_form(1024, 0, 1032, 1032, {"scale", "shift", "scale2", "shift2"}, 13, 4, 1, 1, seg2=True)
    assert f["mode"] == 2 and f["counters"] == dict(ln_rows1=0, ln_rows4=1, ln_fixed_count=1, ln_mode_inst=1)
    assert RB.ln_form(1024, 0, 1032, 1032, {"scale"}, 5, 1, 1, 1)["mode"] == -1
    assert RB.ln_form(1024, 0, 1032, 1032, {"w", "b"}, 5, 1, 0, 1)["counters"] == dict(ln_rows1=1, ln_rows4=0, ln_fixed_count=0, ln_mode_inst=0)
    assert RB.ln_form(192, 0, 200, 200, set(), 5)["counters"] == dict(ln_rows1=0, ln_rows4=0, ln_fixed_count=0, ln_mode_inst=0)
    assert RB.ln_dot_form(1024, 1, 1028, 17, 4)["counters"] == dict(ln_rows1=0, ln_rows4=1, ln_fixed_count=1, ln_mode_inst=0)


def test_e4m3_table_and_rounding():
    assert float(RB.E4M3[126]) == 448.0 and float(RB.E4M3[1]) == 2.0 ** -9 and float(RB.E4M3[8]) == 2.0 ** -6
    x = torch.tensor([0.0, 447.0, 500.0, -464.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10])
    assert RB.e4m3_decode(to_e4m3(x)).tolist() == [0.0, 448.0, 448.0, -448.0, 16.0, 20.0, 0.0, 2.0 ** -8]
