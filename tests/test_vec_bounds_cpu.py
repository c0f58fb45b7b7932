"""The element-wise bounds of tests/vec_bounds.py are neither vacuous nor unreachable -- shown without a GPU and without the library.

REACHABLE: for every kernel an emulation written here in float32 torch -- the same operations in the kernel's order: a lane's strides of
512 over K, the wave tree as a pairwise sum (xor 32, 16, ... 1), the float4 body plus scalar tail of the Euler step, lin_coord's float64
expression -- stays inside the bound (or equals the expected bits) at EVERY element of every shape tests/test_vec_kernels_gpu.py launches.
NOT VACUOUS: each mutant below, applied to the emulation, breaks the bound or the bit equality wherever it applies; where it applies is
spelled out next to each loop, and no case is skipped.

One mutant of the list is EQUIVALENT, and the test says so instead of hiding it: "the last coordinate not pinned to bound".  lin_coord
evaluates i * step - bound in float64 and rounds to float32 once; at i = R that value is within a few 2^-53 of `bound`, so the line that
pins the last coordinate changes no bit at any (R, bound) launched here -- nor does it when the whole expression is evaluated in float32
(tried: R * fl(2 bound / R) - bound hits float32(bound) at all four lattices).  No test on these shapes can tell the kernel with the pin
from the kernel without it; what the test does instead is ASSERT the equivalence (the unpinned coordinates equal np.linspace bit for bit),
so that a change which makes the pin live fails here and has to be looked at.
"""
import math

import pytest
import torch

import vec_bounds as VB


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


GUARD_BF16 = torch.tensor([0x7FA5], dtype=torch.int16).view(torch.bfloat16)
F32 = lambda v: torch.tensor(v, dtype=torch.float32)


def silu32(x):
    return x / (1.0 + torch.exp(-x))


def rne_bf16(x):
    """float32 -> bf16 by integer arithmetic: add 0x7FFF plus the lowest kept bit, drop 16 bits (finite values)"""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    r = torch.where(r >= 0x8000, r - 0x10000, r)
    return r.to(torch.int16).view(torch.bfloat16)


# ---- gemv / gemv_multi --------------------------------------------------------------------------------------------------------------
def lanes(t, K):
    """[..., K] -> [..., strides, 64 lanes, 8]: lane l holds k = 8 l + 512 s .. + 7; missing elements are zeros (they add exact zeros)"""
    Kp = (K + 511) // 512 * 512
    out = torch.zeros(*t.shape[:-1], Kp)
    out[..., :K] = t
    return out.view(*t.shape[:-1], Kp // 512, 64, 8)


def emu_gemv(case, mutant=None):
    B, K, N = case["B"], case["K"], case["N"]
    x = case["x"]
    if case["silu_in"] and mutant != "silu_in_skipped":
        x = silu32(x)
    if mutant == "batch_prev":
        x = x.roll(1, 0)
    w = case["w"].float()
    if mutant == "row_prev":
        w = w.roll(1, 0)
    xl, wl = lanes(x, K)[:, None], lanes(w, K)[None]
    acc = torch.zeros(B, N, 64)
    for s in range(xl.shape[2]):
        if mutant == "second_k_stride_skipped" and s == 1:
            continue
        for e in range(8):
            acc = fma(wl[:, :, s, :, e].expand(B, N, 64), xl[:, :, s, :, e].expand(B, N, 64), acc)
    v = tree(acc)
    if case["bias"] is not None and mutant != "bias_dropped":
        v = v + case["bias"]
    if case["silu_out"]:
        v = silu32(v)
    if mutant == "second_n_pass_skipped":
        v[:, 4 * VB.gemv_blocks(N):] = float("nan")          # rows the grid's first pass does not reach are never stored
    return v


def gemv_applies(mutant, B, K, N, silu_in, bias):
    return {"bias_dropped": bool(bias), "silu_in_skipped": bool(silu_in), "row_prev": N > 1, "second_k_stride_skipped": K > 512,
            "second_n_pass_skipped": N > 4 * VB.gemv_blocks(N), "batch_prev": B > 1}[mutant]


GEMV_MUTANTS = ("bias_dropped", "silu_in_skipped", "row_prev", "second_k_stride_skipped", "second_n_pass_skipped", "batch_prev")


def test_gemv_emulation_is_inside_and_its_mutants_are_not():
    worst, ran = 0.0, {m: 0 for m in GEMV_MUTANTS}
    for B, K, N, si, so, bias in VB.gemv_plan():
        case = VB.gemv_case(B, K, N, si, so, bias)
        ref, bound = VB.gemv_ref_bound(case["x"], case["w"], case["bias"], K, si, so)
        r = VB.worst(emu_gemv(case), ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, (B, K, N, si, so, bias, r)
        for mutant in GEMV_MUTANTS:
            if gemv_applies(mutant, B, K, N, si, bias):
                rm = VB.worst(emu_gemv(case, mutant), ref, bound)
                assert rm > 1.0, "%s is invisible at %s: error / bound %.3f" % (mutant, (B, K, N, si, so, bias), rm)
                ran[mutant] += 1
    print("gemv: largest error / bound of the emulation %.4f" % worst)
    assert min(ran.values()) >= 4, ran
    assert worst > 1e-3


def emu_gemv_multi(case, mutant=None):
    B, K = case["B"], case["K"]
    x = silu32(case["x"]) if case["silu_in"] else case["x"]
    xl = lanes(x, K)[:, None]
    y = torch.full((case["total"],), float("nan"))
    for j, job in enumerate(case["jobs"]):
        N = job["N"]
        wl = lanes(job["w"].float(), K)[None]
        acc = torch.zeros(B, N, 64)
        for s in range(xl.shape[2]):
            for e in range(0, 8, 2):
                p0 = wl[:, :, s, :, e].expand(B, N, 64) * xl[:, :, s, :, e].expand(B, N, 64)
                acc = acc + fma(wl[:, :, s, :, e + 1].expand(B, N, 64), xl[:, :, s, :, e + 1].expand(B, N, 64), p0)
        v = tree(acc)
        bias = job["bias"]
        if mutant == "bias_of_job0":
            b0 = case["jobs"][0]["bias"]
            bias = b0[torch.arange(N) % b0.numel()]
        if bias is not None:
            v = v + bias
        off = 0 if mutant == "out_off_ignored" else job["off"]
        y[off + torch.arange(B)[:, None] * N + torch.arange(N)[None]] = v
    return y


def gemvm_ratio(case, y):
    """(worst error / bound over the three jobs, number of unowned elements that were written)"""
    r = 0.0
    owned = torch.zeros(case["total"], dtype=torch.bool)
    for j, job in enumerate(case["jobs"]):
        ref, bound = VB.gemv_ref_bound(case["x"], job["w"], job["bias"], case["K"], case["silu_in"], 0)
        idx = VB.gemvm_owned(case, j)
        assert not bool(owned[idx.reshape(-1)].any())          # the jobs' outputs do not overlap
        owned[idx.reshape(-1)] = True
        r = max(r, VB.worst(y[idx], ref, bound))
    return r, int((~torch.isnan(y[~owned])).sum())


def test_gemv_multi_emulation_is_inside_and_its_mutants_are_not():
    worst = 0.0
    for B in VB.GEMVM_B:
        for K in VB.GEMVM_K:
            for si in (0, 1):
                case = VB.gemvm_case(B, K, si)
                r, stray = gemvm_ratio(case, emu_gemv_multi(case))
                worst = max(worst, r)
                assert r <= 1.0 and stray == 0, (B, K, si, r, stray)
                for mutant in ("out_off_ignored", "bias_of_job0"):
                    rm, _ = gemvm_ratio(case, emu_gemv_multi(case, mutant))
                    assert rm > 1.0, "%s is invisible at %s" % (mutant, (B, K, si))
    print("gemv_multi: largest error / bound of the emulation %.4f" % worst)
    assert worst > 1e-3


def test_gemv_launch_rule_and_plan():
    assert [VB.gemv_blocks(n) for n in (1, 4, 5, 1023, 1024, 1029)] == [1, 1, 2, 256, 256, 256]
    ns = {N for _, _, N, _, _, _ in VB.gemv_plan()}
    assert any(N >= 1024 and N > 4 * VB.gemv_blocks(N) for N in ns) and any(N < 1024 and N % 4 for N in ns)      # a second pass; a row tail
    combos = {(si, so) for _, _, _, si, so, _ in VB.gemv_plan()}
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert sum(1 for c in VB.gemv_plan() if not c[5]) >= 2


# ---- timestep embedding -------------------------------------------------------------------------------------------------------------
def emu_timestep(t, tf, mutant=None):
    j = torch.arange(128, dtype=torch.float32)
    L = torch.log(F32(1000.0 if mutant == "period_1000" else 10000.0))
    freq = torch.exp(-L * j / F32(127.0 if mutant == "j_over_127" else 128.0))
    arg = t[:, None] * freq if mutant == "time_factor_dropped" else t[:, None] * F32(tf) * freq
    c, s = torch.cos(arg), torch.sin(arg)
    return torch.cat([s, c], -1) if mutant == "cos_sin_exchanged" else torch.cat([c, s], -1)


def test_timestep_emulation_is_inside_and_its_mutants_are_not():
    worst, ran = 0.0, {m: 0 for m in ("cos_sin_exchanged", "j_over_127", "time_factor_dropped", "period_1000")}
    for B in VB.TS_B:
        for tv in VB.TS_T:
            for tf in VB.TS_TF:
                t = VB.ts_times(B, tv)
                ref, bound = VB.ts_ref_bound(t, tf)
                got = emu_timestep(t, tf)
                r = VB.worst(got, ref, bound)
                worst = max(worst, r)
                assert r <= 1.0, (B, tv, tf, r)
                if tv == 0.0:
                    assert bool((got[:, :128] == 1.0).all()) and bool((got[:, 128:] == 0.0).all())
                    assert bool((bound[:, 128:] == 0.0).all())          # nothing but an exact zero passes there
                    continue                                            # every mutant but the exchange gives the same at t = 0
                for mutant in ran:
                    if mutant == "time_factor_dropped" and tf == 1.0:
                        continue
                    rm = VB.worst(emu_timestep(t, tf, mutant), ref, bound)
                    assert rm > 1.0, "%s is invisible at %s: error / bound %.3f" % (mutant, (B, tv, tf), rm)
                    ran[mutant] += 1
        t0 = VB.ts_times(B, 0.0)
        assert VB.worst(emu_timestep(t0, 1000.0, "cos_sin_exchanged"), *VB.ts_ref_bound(t0, 1000.0)) > 1.0
    print("timestep_embedding: largest error / bound of the emulation %.4f" % worst)
    assert min(ran.values()) >= 6 and worst > 1e-3
    # the size of the bound where it is largest: t = 1, tf = 1000, j = 0 (module docstring of vec_bounds)
    b = float(VB.ts_ref_bound(VB.ts_times(1, 1.0), 1000.0)[1][0, 0])
    assert 3e-4 < b < 2e-3


# ---- Fourier embeddings -------------------------------------------------------------------------------------------------------------
def emu_coords(R, bound, mutant=None):
    """lin_coord for i = 0 .. R"""
    i = torch.arange(R + 1)
    if mutant == "coord_f32":
        c = i.float() * F32(2.0 * bound / R) - F32(bound)
    else:
        c = (i.double() * ((2.0 * bound) / R) + (-bound)).float()
    if mutant != "unpinned":
        c[R] = F32(bound)
    return c


def emu_fourier(idx, R, bound, nf, pi, mutant=None):
    n = R + 1
    coords = emu_coords(R, bound, mutant)
    ii, jj, kk = idx // (n * n), (idx // n) % n, idx % n
    if mutant == "axes_kji":
        ii, kk = kk, torch.where(ii < n, ii, torch.zeros_like(ii))
        inside = (idx // (n * n) < n)[:, None]
    else:
        inside = (ii < n)[:, None]
    xyz = torch.stack([coords[ii.clamp_max(R)], coords[jj], coords[kk]], -1)
    xyz = torch.where(inside, xyz, torch.zeros_like(xyz))
    out = torch.zeros(idx.numel(), 64, dtype=torch.bfloat16)
    out[:, :3] = xyz.to(torch.bfloat16)
    if nf:
        fr = torch.tensor([float(2 * f if mutant == "two_f" else 1 << f) for f in range(nf)], dtype=torch.float32)
        if pi and mutant != "pi_dropped":
            fr = fr * F32(VB.PI32)
        arg = xyz[:, :, None] * fr[None, None, :]                     # [n][c][f]
        if mutant == "f_major":
            arg = arg.transpose(1, 2)
        s, c = torch.sin(arg).reshape(-1, 3 * nf), torch.cos(arg).reshape(-1, 3 * nf)
        if mutant == "sin_cos_exchanged":
            s, c = c, s
        out[:, 3:3 + 3 * nf] = s.to(torch.bfloat16)
        out[:, 3 + 3 * nf:3 + 6 * nf] = c.to(torch.bfloat16)
    return out


def fourier_configs():
    """(R, bound, idx): the rows the GPU test asks the dense kernel for"""
    for R, bound in VB.FOURIER_GRIDS:
        yield R, bound, torch.arange((R + 1) ** 3 + VB.FOURIER_BEHIND)
    R, bound = VB.FOURIER_BIG
    yield R, bound, torch.cat([torch.arange(s, s + c) for s, c in VB.fourier_big_windows()])


FOURIER_MUTANTS = ("sin_cos_exchanged", "f_major", "pi_dropped", "two_f", "coord_f32", "unpinned", "axes_kji")


def test_fourier_emulation_is_inside_and_its_mutants_are_not():
    worst = 0.0
    applied = {m: 0 for m in FOURIER_MUTANTS}
    killed = {m: 0 for m in FOURIER_MUTANTS}
    for R, bound, idx in fourier_configs():
        coords = VB.lin_coords(R, bound)
        assert VB.bit_mismatches(emu_coords(R, bound), coords) == 0, "lin_coord's expression is not np.linspace at %s" % ((R, bound),)
        assert VB.bit_mismatches(emu_coords(R, bound, "unpinned"), coords) == 0          # the equivalent mutant (module docstring)
        xyz = VB.fourier_xyz(idx, R, coords)
        for nf in VB.FOURIER_NF:
            for pi in (0, 1):
                ref, bnd, exact = VB.fourier_ref_bound(xyz, nf, pi)
                r, bad = VB.fourier_check(emu_fourier(idx, R, bound, nf, pi), ref, bnd, exact)
                worst = max(worst, r)
                assert r <= 1.0 and bad == 0, (R, bound, nf, pi, r, bad)
                applies = {"sin_cos_exchanged": nf >= 1, "f_major": nf >= 2, "pi_dropped": bool(pi) and nf >= 1, "two_f": nf >= 1, "axes_kji": True,
                           "coord_f32": True, "unpinned": True}
                for mutant in FOURIER_MUTANTS:
                    if not applies[mutant]:
                        continue
                    rm, bm = VB.fourier_check(emu_fourier(idx, R, bound, nf, pi, mutant), ref, bnd, exact)
                    applied[mutant] += 1
                    killed[mutant] += int(rm > 1.0 or bm > 0)
    print("fourier: largest error / bound of the emulation %.3f; kills / applications %s" % (worst, {m: (killed[m], applied[m]) for m in FOURIER_MUTANTS}))
    assert worst > 0.5                                            # a rounding tie is near: the bf16 bound is met tightly
    for m in ("sin_cos_exchanged", "f_major", "pi_dropped", "two_f", "axes_kji"):
        assert killed[m] == applied[m] and applied[m] >= 8, (m, killed[m], applied[m])      # wherever they apply
    # float32 coordinates move a coordinate by one float32 step at most: invisible in the bf16 x / y / z channels, visible where the
    # argument's frequency is high and the sine or cosine small -- at one shape at least, as the list demands
    assert killed["coord_f32"] >= 1
    assert killed["unpinned"] == 0                                # the equivalent mutant (module docstring)


def test_fourier_lists_hold_what_the_gpu_test_needs():
    for R, bound in VB.FOURIER_GRIDS + (VB.FOURIER_BIG,):
        n3 = (R + 1) ** 3
        for count in VB.FOURIER_LISTS:
            idx = VB.fourier_list(R, count)
            assert idx.numel() == count and int(idx.min()) >= 0 and int(idx.max()) == n3 - 1
            assert count < 2 or int(idx.min()) == 0
            assert count < 3 or idx.unique().numel() < count          # a repeat
        if R != VB.FOURIER_BIG[0]:
            assert 0 < VB.fourier_split(R) < n3 and VB.fourier_split(R) % 256 and VB.fourier_split(R) % (R + 1)
    assert VB.fourier_big_windows()[-1] == (513 ** 3 - 100, 300)


# ---- Euler steps ------------------------------------------------------------------------------------------------------------------------
def emu_euler(lat, v, ds, form, mutant=None):
    """euler_step_kernel (float4 body, scalar tail in the thread that owns the last partial group) / euler_step_scalar_kernel"""
    ds = F32(ds)
    n = lat.numel()
    out = lat.clone()
    if form == "scalar":
        return lat + ds * v
    n4 = n // 4 * 4
    out[:n4] = (lat[:n4].view(-1, 4) + ds * v[:n4].view(-1, 4)).view(-1)
    if mutant != "tail_skipped":
        out[n4:] = lat[n4:] + ds * v[n4:]
    return out


def emu_cfg(lat, v2, gd, ds, mutant=None):
    n = lat.numel()
    vc, vu = v2[:n], v2[n:]
    if mutant == "halves_exchanged":
        vc, vu = vu, vc
    d = (vu - vc) if mutant == "vu_minus_vc" else (vc - vu)
    return lat + F32(ds) * (vu + F32(gd) * d)


def test_euler_emulations_are_inside_and_their_mutants_are_not():
    worst, ran = 0.0, {"tail_skipped": 0, "halves_exchanged": 0, "vu_minus_vc": 0}
    for n in VB.EULER_N:
        case = VB.euler_case(n)
        for ds in VB.DS:
            ref, bound = VB.euler_ref_bound(case["lat"], case["v"], ds)
            for form in ("vec", "scalar"):
                r = VB.worst(emu_euler(case["lat"], case["v"], ds, form), ref, bound)
                worst = max(worst, r)
                assert r <= 1.0, (n, ds, form, r)
            if n % 4 and ds != 0.0:
                assert VB.worst(emu_euler(case["lat"], case["v"], ds, "vec", "tail_skipped"), ref, bound) > 1.0, n
                ran["tail_skipped"] += 1
    for n in VB.CFG_N:
        case = VB.cfg_case(n)
        for gd in VB.CFG_G:
            for ds in VB.DS:
                ref, bound = VB.cfg_ref_bound(case["lat"], case["v2"], gd, ds)
                r = VB.worst(emu_cfg(case["lat"], case["v2"], gd, ds), ref, bound)
                worst = max(worst, r)
                assert r <= 1.0, (n, gd, ds, r)
                if ds != 0.0:                                   # (at ds = 0 nothing but lat reaches the output)
                    assert VB.worst(emu_cfg(case["lat"], case["v2"], gd, ds, "halves_exchanged"), ref, bound) > 1.0, (n, gd)
                    ran["halves_exchanged"] += 1
                    if gd != 0.0:
                        assert VB.worst(emu_cfg(case["lat"], case["v2"], gd, ds, "vu_minus_vc"), ref, bound) > 1.0, (n, gd)
                        ran["vu_minus_vc"] += 1
    print("euler steps: largest error / bound of the emulations %.4f" % worst)
    assert ran == {"tail_skipped": 5, "halves_exchanged": 12, "vu_minus_vc": 8} and worst > 1e-3


def test_euler_launch_rule():
    assert VB.euler_form(0x1000, 0x2000) == "vec" and VB.euler_form(0x1004, 0x2000) == "scalar" and VB.euler_form(0x1000, 0x2004) == "scalar"
    assert VB.euler_form(0x1010, 0x2020) == "vec" and VB.euler_form(0x1008, 0x2008) == "scalar"


# ---- nonfinite_flag ---------------------------------------------------------------------------------------------------------------------
def emu_nonfinite(x, old, mutant=None):
    if mutant == "last_not_read":
        x = x[:-1]
    bad = torch.isnan(x) if mutant == "only_nans" else ((VB.ibits(x) & 0x7F800000) == 0x7F800000)
    return old | 1 if bool(bad.any()) else old


def test_nonfinite_flag_emulation_and_mutants():
    ran = {"only_nans": 0, "last_not_read": 0}
    for n in VB.NF_N:
        clean = VB.nf_vector(n)
        assert bool(torch.isfinite(clean).all())
        assert n < 5 or (bool((clean.abs() > 3e38).any()) and bool(((clean != 0) & (clean.abs() < 1e-38)).any()))      # max finite, denormals
        for old in VB.NF_OLD:
            assert emu_nonfinite(clean, old) == VB.nf_expected(clean, old) == old
            for bad in VB.NF_BAD:
                for pos in VB.nf_positions(n):
                    x = clean.clone()
                    x[pos] = bad
                    want = VB.nf_expected(x, old)
                    assert want == old | 1 and emu_nonfinite(x, old) == want
                    if not math.isnan(bad):
                        assert emu_nonfinite(x, old, "only_nans") != want
                        ran["only_nans"] += 1
                    if pos == n - 1:
                        assert emu_nonfinite(x, old, "last_not_read") != want
                        ran["last_not_read"] += 1
    assert ran["only_nans"] >= 16 and ran["last_not_read"] >= 24


# ---- bit-exact copies and casts ---------------------------------------------------------------------------------------------------------
def emu_cast_pad(x, Cpad, scale, mutant=None):
    rows, C = x.shape
    out = GUARD_BF16.repeat(rows * Cpad).view(rows, Cpad).clone()
    s = F32(scale)
    if mutant == "scale_after_rounding":
        out[:, :C] = rne_bf16(rne_bf16(x).float() * s)
    elif mutant == "truncate":
        out[:, :C] = truncate_bf16(x * s)
    else:
        out[:, :C] = rne_bf16(x * s)
    if mutant != "pad_not_zeroed":
        out[:, C:] = 0
    return out


def cast_expected_padded(x, Cpad, scale):
    out = torch.zeros(x.shape[0], Cpad, dtype=torch.bfloat16)
    out[:, :x.shape[1]] = VB.cast_expected(x, scale)
    return out


def test_cast_pad_emulation_is_torchs_rounding_and_its_mutants_are_not():
    ran = {"pad_not_zeroed": 0, "scale_after_rounding": 0, "truncate": 0}
    for rows in VB.CAST_ROWS:
        for C, Cpad in VB.CAST_CC:
            x = VB.cast_case(rows, C)
            for scale in VB.CAST_SCALE:
                want = cast_expected_padded(x, Cpad, scale)
                assert VB.bit_mismatches(emu_cast_pad(x, Cpad, scale), want) == 0, (rows, C, Cpad, scale)
                applies = {"pad_not_zeroed": Cpad > C, "scale_after_rounding": scale != 1.0 and rows * C >= 12, "truncate": rows * C >= 12}
                for mutant, ok in applies.items():
                    if ok:
                        assert VB.bit_mismatches(emu_cast_pad(x, Cpad, scale, mutant), want) > 0, "%s is invisible at %s" % (mutant, (rows, C, Cpad, scale))
                        ran[mutant] += 1
    assert ran["pad_not_zeroed"] == 12 and ran["scale_after_rounding"] >= 3 and ran["truncate"] >= 6
    # the tie at element 0 goes to even
    assert float(VB.cast_expected(VB.cast_case(1, 3), 1.0)[0, 0]) == 1.0


def test_f32_to_bf16_specials_and_the_integer_rounding():
    x = VB.F2B_SPECIALS
    want = x.to(torch.bfloat16)
    w = VB.ibits(want).to(torch.int32) & 0xFFFF
    assert w[:4].tolist() == [0x0000, 0x8000, 0x7F80, 0xFF80]
    assert bool(torch.isnan(want[4:6].float()).all())
    assert w[6:13].tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x4000, 0x3F80, 0x3F81]
    assert w[13:].tolist() == [0x7F80, 0xFF80]
    assert VB.f2b_mismatches(want, x) == 0
    fin = ~torch.isnan(x)
    assert VB.bit_mismatches(rne_bf16(x)[fin], want[fin]) == 0
    assert VB.f2b_mismatches(truncate_bf16(x), x) > 0              # truncation: the low-bits NaN becomes an infinity, the ties and the maximum differ
    for n in VB.F2B_N:
        y = VB.f2b_case(n)
        assert VB.f2b_mismatches(rne_bf16(y), y) == 0
    assert VB.f2b_mismatches(truncate_bf16(VB.f2b_case(257)), VB.f2b_case(257)) > 0


def emu_patch_rows(img, S, ps, Kpad):
    """im2col_kernel's index arithmetic, one output element per index"""
    P = S // ps
    i = torch.arange(P * P * Kpad)
    pidx, k = i // Kpad, i % Kpad
    c, r = k // (ps * ps), k % (ps * ps)
    dy, dx, py, px = r // ps, r % ps, pidx // P, pidx % P
    inside = k < 3 * ps * ps
    src = ((c * S + py * ps + dy) * S + px * ps + dx).clamp_max(3 * S * S - 1)
    v = torch.where(inside, img.reshape(-1)[src], torch.zeros(()))
    return rne_bf16(v).view(P * P, Kpad)


def test_copies_and_adds():
    for S, ps, Kpad in VB.PATCH_SHAPES:
        img = VB.patch_case(S)
        want = VB.patch_expected(img, S, ps, Kpad)
        assert VB.bit_mismatches(emu_patch_rows(img, S, ps, Kpad), want) == 0
        assert bool((want[:, 3 * ps * ps:] == 0).all()) and S % ps == 0 and Kpad >= 3 * ps * ps
        if S > ps:
            assert VB.bit_mismatches(emu_patch_rows(img.transpose(1, 2).contiguous(), S, ps, Kpad), want) > 0          # dy and dx exchanged
    for rows in VB.ROWS_ROWS:
        for C in VB.ROWS_C:
            x, pos, vals = VB.rows_case(rows, C)
            assert VB.bit_mismatches((x.double() + pos.double()).float(), x + pos) == 0          # one IEEE sum per element
            assert vals.expand(rows, C).shape == x.shape
    for n in VB.VADD_N:
        a, b = VB.vadd_case(n)
        assert VB.bit_mismatches((a.double() + b.double()).float(), a + b) == 0
        assert bool(((a + b) != a).any())
