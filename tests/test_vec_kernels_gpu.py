"""The small kernels of a sampling step and of input staging -- gemv, gemv_multi, timestep_embedding, fourier_grid, fourier_points,
cfg_euler, both euler_step kernels, nonfinite_flag, cast_pad, fill_rows, add_rows, f32_to_bf16, the patch rows of im2col_kernel and both
vec_add kernels -- each through its own r3g_op_* entry point, one launch at a time.

Per launch:
  * the ELEMENT-WISE bound of tests/vec_bounds.py at every output element, or equality of the bit patterns for the kernels that do one IEEE
    operation or a copy per element (derived there; tests/test_vec_bounds_cpu.py shows that an emulation of each kernel meets it and that
    the listed mutants do not);
  * outputs AND inputs sit in larger buffers filled with a NaN bit pattern (tests/row_guard.py): eight elements in front, the columns
    between the width and the leading dimension, two rows (or eight elements) behind.  Those keep their bits; an owned element that was
    never stored, or a read outside an operand, is a NaN in the result.
One refusals test per entry point: every contract violation of include/r3g.h is R3G_ERR_INVALID with not one bit written, and an admitted
call follows.  The closing test asserts that both Euler kernels and both grid rules of gemv_launch were reached, as computed from the
launch rules restated in vec_bounds.  All shapes are tiny: the file takes a few seconds on an MI355X.
"""
import ctypes

import pytest

import row_guard as G
import vec_bounds as VB
from parity_support import report

pytestmark = pytest.mark.gpu

OFF = G.OFF
ptr = G.ptr
_MEMO = {}
EULER_REACHED, GEMV_REACHED = set(), set()


@pytest.fixture(scope="module")
def env():
    import torch
    from r3g import ffi
    ffi.context(0)
    return torch, ffi.lib(), ffi


def ar(torch, n):
    return torch.arange(n, device="cuda")


def rows_idx(torch, rows, width, ld, off=OFF):
    """flat element indices [rows][width] of rows that are ld apart, the first at element off"""
    return (off + ar(torch, rows) * ld)[:, None] + ar(torch, width)[None]


def placed(torch, dtype, total, idx, values):
    return G.place(torch, G.guarded(torch, dtype, total), idx, values)


def finish(name, worst, failures, bit_exact=False):
    if bit_exact:
        report("vec kernels: %s (elements that differ in a bit)" % name, worst, 0.0)
        print("%s: %d elements differ" % (name, worst))
    else:
        report("vec kernels: %s (error / bound)" % name, worst, 1.0)
        print("%s: worst error / bound %.4f" % (name, worst))
    assert not failures, "%d findings, the first: %s" % (len(failures), "\n".join(failures[:12]))


def guard_finding(torch, failures, tag, flat, owned):
    n, first = G.untouched(torch, flat, owned)
    if n:
        failures.append("%s: %d elements outside the output were written, the first at element %d" % (tag, n, first - OFF))


# ---- gemv ---------------------------------------------------------------------------------------------------------------------------------
def gemv_matrix_bufs(torch, K, N):
    key = ("gemv_w", K, N)
    if key not in _MEMO:
        w, b = VB.gemv_matrix(K, N)
        ldw = K + VB.GEMV_PAD
        _MEMO[key] = dict(ldw=ldw, w=placed(torch, torch.bfloat16, OFF + (N + 2) * ldw, rows_idx(torch, N, K, ldw), w.cuda()),
                          bias=placed(torch, torch.float32, OFF + N + 8, OFF + ar(torch, N), b.cuda()))
    return _MEMO[key]


def gemv_input_buf(torch, B, K):
    key = ("gemv_x", B, K)
    if key not in _MEMO:
        _MEMO[key] = placed(torch, torch.float32, OFF + B * K + 8, OFF + ar(torch, B * K), VB.gemv_input(B, K).cuda())
    return _MEMO[key]


def run_gemv(env):
    if "gemv" in _MEMO:
        return _MEMO["gemv"]
    torch, L, ffi = env
    worst, failures = 0.0, []
    for B, K, N, si, so, bias in VB.gemv_plan():
        case = VB.gemv_case(B, K, N, si, so, bias, "cuda")
        ref, bound = VB.gemv_ref_bound(case["x"], case["w"], case["bias"], K, si, so)
        m, xb = gemv_matrix_bufs(torch, K, N), gemv_input_buf(torch, B, K)
        y = G.guarded(torch, torch.float32, OFF + (B + 2) * N + 8)
        yi = OFF + ar(torch, B * N).view(B, N)
        tag = "gemv b %d k %d n %d silu %d / %d bias %d" % (B, K, N, si, so, bias)
        G.run(torch, ffi, lambda: L.r3g_op_gemv(ptr(xb, OFF), B, K, ptr(m["w"], OFF), m["ldw"], ptr(m["bias"], OFF) if bias else None, ptr(y, OFF),
                                                N, si, so, G.stream(torch)), tag)
        r = VB.worst(y[yi], ref, bound)
        worst = max(worst, r)
        if not r <= 1.0:
            failures.append("%s: error / bound %.3f" % (tag, r))
        else:
            GEMV_REACHED.add(("blocks 256" if VB.gemv_blocks(N) == 256 and N >= 1024 else "blocks n / 4", N > 4 * VB.gemv_blocks(N)))
        guard_finding(torch, failures, tag, y, yi)
    _MEMO["gemv"] = (worst, failures)
    return _MEMO["gemv"]


def test_gemv(env):
    worst, failures = run_gemv(env)
    finish("gemv", worst, failures)


def test_gemv_multi(env):
    torch, L, ffi = env
    worst, failures = 0.0, []
    for B in VB.GEMVM_B:
        for K in VB.GEMVM_K:
            xb = gemv_input_buf(torch, B, K)
            for si in (0, 1):
                case = VB.gemvm_case(B, K, si, "cuda")
                jobs = case["jobs"]
                wb = [placed(torch, torch.bfloat16, OFF + (j["N"] + 2) * j["ldw"], rows_idx(torch, j["N"], K, j["ldw"]), j["w"]) for j in jobs]
                bb = [None if j["bias"] is None else placed(torch, torch.float32, OFF + j["N"] + 8, OFF + ar(torch, j["N"]), j["bias"]) for j in jobs]
                nj = len(jobs)
                w_arr = (ctypes.c_void_p * nj)(*[ptr(b, OFF) for b in wb])
                b_arr = (ctypes.c_void_p * nj)(*[ptr(b, OFF) for b in bb])
                ld_arr = (ctypes.c_int64 * nj)(*[j["ldw"] for j in jobs])
                n_arr = (ctypes.c_int * nj)(*[j["N"] for j in jobs])
                off_arr = (ctypes.c_int64 * nj)(*[j["off"] for j in jobs])
                y = G.guarded(torch, torch.float32, OFF + case["total"] + 8)
                tag = "gemv_multi b %d k %d silu_in %d" % (B, K, si)
                G.run(torch, ffi, lambda: L.r3g_op_gemv_multi(ptr(xb, OFF), B, K, ctypes.addressof(w_arr), ctypes.addressof(b_arr), ctypes.addressof(ld_arr),
                                                              ctypes.addressof(n_arr), ctypes.addressof(off_arr), nj, ptr(y, OFF), si, G.stream(torch)), tag)
                owned = []
                for j, job in enumerate(jobs):
                    ref, bound = VB.gemv_ref_bound(case["x"], job["w"], job["bias"], K, si, 0)
                    idx = OFF + VB.gemvm_owned(case, j)
                    owned.append(idx.reshape(-1))
                    r = VB.worst(y[idx], ref, bound)
                    worst = max(worst, r)
                    if not r <= 1.0:
                        failures.append("%s job %d: error / bound %.3f" % (tag, j, r))
                guard_finding(torch, failures, tag, y, torch.cat(owned))
    finish("gemv_multi", worst, failures)


# ---- timestep embedding -----------------------------------------------------------------------------------------------------------------
def test_timestep_embedding(env):
    torch, L, ffi = env
    worst, failures = 0.0, []
    for B in VB.TS_B:
        oi = OFF + ar(torch, B * 256).view(B, 256)
        for tv in VB.TS_T:
            for tf in VB.TS_TF:
                for by_array in (1, 0):
                    t = VB.ts_times(B, tv) if by_array else VB.ts_times(1, tv).expand(B).contiguous()
                    ref, bound = VB.ts_ref_bound(t.cuda(), tf)
                    tb = placed(torch, torch.float32, OFF + B + 8, OFF + ar(torch, B), t.cuda())
                    out = G.guarded(torch, torch.float32, OFF + (B + 2) * 256)
                    tag = "timestep_embedding b %d t %g time_factor %g %s" % (B, tv, tf, "t array" if by_array else "t scalar")
                    G.run(torch, ffi, lambda: L.r3g_op_timestep_embedding(ptr(tb, OFF) if by_array else None, float(t[0]), B, tf, ptr(out, OFF),
                                                                          G.stream(torch)), tag)
                    got = out[oi]
                    r = VB.worst(got, ref, bound)
                    worst = max(worst, r)
                    if not r <= 1.0:
                        failures.append("%s: error / bound %.3f" % (tag, r))
                    if tv == 0.0 and not (bool((got[:, :128] == 1.0).all()) and bool((got[:, 128:] == 0.0).all())):
                        failures.append("%s: t = 0 must give exactly 1.0 and 0.0" % tag)
                    guard_finding(torch, failures, tag, out, oi)
    finish("timestep_embedding", worst, failures)


# ---- Fourier embeddings -----------------------------------------------------------------------------------------------------------------
def fourier_configs(torch):
    """(R, bound, calls [(start, count)], idx int64 (CPU, ascending): the lattice index of every dense row asked for)"""
    for R, bound in VB.FOURIER_GRIDS:
        n = (R + 1) ** 3 + VB.FOURIER_BEHIND
        yield R, bound, ((0, VB.fourier_split(R)), (VB.fourier_split(R), n - VB.fourier_split(R))), torch.arange(n)
    R, bound = VB.FOURIER_BIG
    yield R, bound, VB.fourier_big_windows(), torch.cat([torch.arange(s, s + c) for s, c in VB.fourier_big_windows()])


def test_fourier_grid_and_points(env):
    torch, L, ffi = env
    worst_g, worst_p, bits, failures = 0.0, 0.0, 0, []
    for R, bound, calls, idx in fourier_configs(torch):
        n3, nrows = (R + 1) ** 3, idx.numel()
        xyz = VB.fourier_xyz(idx, R, VB.lin_coords(R, bound))          # float32, on the CPU: the argument is formed there (vec_bounds)
        lists = {c: VB.fourier_list(R, c) for c in VB.FOURIER_LISTS}
        for nf in VB.FOURIER_NF:
            for pi in (0, 1):
                ref, bnd, exact = (v.cuda() for v in VB.fourier_ref_bound(xyz, nf, pi))
                tag = "fourier r %d bound %g num_freqs %d include_pi %d" % (R, bound, nf, pi)
                dense = G.guarded(torch, torch.bfloat16, OFF + (nrows + 2) * 64)
                row0 = 0
                for start, count in calls:
                    G.run(torch, ffi, lambda: L.r3g_op_fourier_grid(ptr(dense, OFF + row0 * 64), start, count, R, bound, nf, pi, G.stream(torch)),
                          "%s dense start %d count %d" % (tag, start, count))
                    row0 += count
                di = OFF + ar(torch, nrows * 64).view(nrows, 64)
                grid_rows = dense[di]
                r, bad = VB.fourier_check(grid_rows, ref, bnd, exact)
                worst_g, bits = max(worst_g, r), bits + bad
                if not r <= 1.0 or bad:
                    failures.append("%s dense: error / bound %.3f, %d of x / y / z / padding differ in a bit" % (tag, r, bad))
                guard_finding(torch, failures, tag + " dense", dense, di)
                origin = grid_rows[int((idx >= n3).nonzero()[0])]
                for count, lst in lists.items():
                    pos = torch.searchsorted(idx, lst).cuda()          # the dense row that holds each listed point
                    lb = lst.to(torch.int32).cuda()
                    for rows in (count, count + VB.FOURIER_ROWS_EXTRA):
                        out = G.guarded(torch, torch.bfloat16, OFF + (rows + 2) * 64)
                        oi = OFF + ar(torch, rows * 64).view(rows, 64)
                        ptag = "%s listed count %d rows %d" % (tag, count, rows)
                        G.run(torch, ffi, lambda: L.r3g_op_fourier_points(ptr(out, OFF), ptr(lb), count, rows, R, bound, nf, pi, G.stream(torch)), ptag)
                        got = out[oi]
                        r, bad = VB.fourier_check(got[:count], ref[pos], bnd[pos], exact)
                        worst_p, bits = max(worst_p, r), bits + bad
                        same = VB.bit_mismatches(got[:count], grid_rows[pos]) + VB.bit_mismatches(got[count:], origin[None].expand(rows - count, 64))
                        if not r <= 1.0 or bad or same:
                            failures.append("%s: error / bound %.3f, %d exact channels differ, %d elements differ from the dense kernel's rows" % (ptag, r, bad, same))
                        guard_finding(torch, failures, ptag, out, oi)
    report("vec kernels: fourier_grid (error / bound)", worst_g, 1.0)
    report("vec kernels: fourier_points (error / bound)", worst_p, 1.0)
    print("fourier_grid: worst error / bound %.4f; fourier_points: %.4f; coordinate / padding elements that differ in a bit: %d" % (worst_g, worst_p, bits))
    assert not failures, "%d findings, the first: %s" % (len(failures), "\n".join(failures[:12]))


# ---- Euler steps ------------------------------------------------------------------------------------------------------------------------
def run_euler(env):
    if "euler" in _MEMO:
        return _MEMO["euler"]
    torch, L, ffi = env
    worst, failures = 0.0, []
    for n in VB.EULER_N:
        case = VB.euler_case(n, "cuda")
        for align in VB.EULER_ALIGN:
            lo, vo = OFF + (align == "lat_off"), OFF + (align == "v_off")
            vb = placed(torch, torch.float32, vo + n + 8, vo + ar(torch, n), case["v"])
            for ds in VB.DS:
                ref, bound = VB.euler_ref_bound(case["lat"], case["v"], ds)
                li = lo + ar(torch, n)
                lat = placed(torch, torch.float32, lo + n + 8, li, case["lat"])
                form = VB.euler_form(ptr(lat, lo), ptr(vb, vo))
                tag = "euler_step n %d %s ds %g (%s kernel)" % (n, align, ds, form)
                G.run(torch, ffi, lambda: L.r3g_op_euler_step(ptr(lat, lo), ptr(vb, vo), n, ds, G.stream(torch)), tag)
                r = VB.worst(lat[li], ref, bound)
                worst = max(worst, r)
                if not r <= 1.0:
                    failures.append("%s: error / bound %.3f" % (tag, r))
                else:
                    EULER_REACHED.add((form, n % 4 != 0, n >= 4))
                guard_finding(torch, failures, tag, lat, li)
    _MEMO["euler"] = (worst, failures)
    return _MEMO["euler"]


def test_euler_step(env):
    worst, failures = run_euler(env)
    finish("euler_step", worst, failures)


def test_cfg_euler(env):
    torch, L, ffi = env
    worst, failures = 0.0, []
    for n in VB.CFG_N:
        case = VB.cfg_case(n, "cuda")
        vb = placed(torch, torch.float32, OFF + 2 * n + 8, OFF + ar(torch, 2 * n), case["v2"])
        li = OFF + ar(torch, n)
        for gd in VB.CFG_G:
            for ds in VB.DS:
                ref, bound = VB.cfg_ref_bound(case["lat"], case["v2"], gd, ds)
                lat = placed(torch, torch.float32, OFF + n + 8, li, case["lat"])
                tag = "cfg_euler n %d guidance %g ds %g" % (n, gd, ds)
                G.run(torch, ffi, lambda: L.r3g_op_cfg_euler(ptr(lat, OFF), ptr(vb, OFF), n, gd, ds, G.stream(torch)), tag)
                r = VB.worst(lat[li], ref, bound)
                worst = max(worst, r)
                if not r <= 1.0:
                    failures.append("%s: error / bound %.3f" % (tag, r))
                guard_finding(torch, failures, tag, lat, li)
    finish("cfg_euler", worst, failures)


# ---- nonfinite_flag ---------------------------------------------------------------------------------------------------------------------
def test_nonfinite_flag(env):
    """the guard pattern around x is itself a NaN: a read outside [0, n) sets the flag of a clean vector"""
    torch, L, ffi = env
    failures, launches = [], 0
    for n in VB.NF_N:
        clean = VB.nf_vector(n, "cuda")
        xi = OFF + ar(torch, n)
        xb = placed(torch, torch.float32, OFF + n + 8, xi, clean)
        for old in VB.NF_OLD:
            for bad, pos in [(None, None)] + [(b, p) for b in VB.NF_BAD for p in VB.nf_positions(n)]:
                if bad is not None:
                    xb[OFF + pos] = bad
                flag = G.guarded(torch, torch.float32, OFF + 1 + 8)
                flag.view(torch.int32)[OFF] = old
                tag = "nonfinite_flag n %d bad %s at %s flag %d" % (n, bad, pos, old)
                G.run(torch, ffi, lambda: L.r3g_op_nonfinite_flag(ptr(xb, OFF), n, ptr(flag, OFF), G.stream(torch)), tag)
                launches += 1
                want = VB.nf_expected(xb[xi], old)
                if want != (old if bad is None else old | 1):
                    failures.append("%s: the operand is not what the case says" % tag)
                got = int(flag.view(torch.int32)[OFF])
                if got != want:
                    failures.append("%s: flag %d, expected %d" % (tag, got, want))
                guard_finding(torch, failures, tag, flag, torch.tensor([OFF], device="cuda"))
                if bad is not None:
                    xb[OFF + pos] = clean[pos]
    finish("nonfinite_flag, %d launches" % launches, len(failures), failures, bit_exact=True)


# ---- bit-exact copies and casts ---------------------------------------------------------------------------------------------------------
def test_cast_pad(env):
    torch, L, ffi = env
    diff, failures = 0, []
    for rows in VB.CAST_ROWS:
        for C, Cpad in VB.CAST_CC:
            x = VB.cast_case(rows, C, "cuda")
            ldo = Cpad + VB.CAST_LDO_PAD
            oi = rows_idx(torch, rows, Cpad, ldo)
            for pad in VB.CAST_LDI_PAD:
                ldi = C + pad
                xb = placed(torch, torch.float32, OFF + (rows + 2) * ldi, rows_idx(torch, rows, C, ldi), x)
                for scale in VB.CAST_SCALE:
                    want = torch.zeros(rows, Cpad, dtype=torch.bfloat16, device="cuda")
                    want[:, :C] = VB.cast_expected(x, scale)
                    out = G.guarded(torch, torch.bfloat16, OFF + (rows + 2) * ldo)
                    tag = "cast_pad rows %d c %d cpad %d ldi %d scale %g" % (rows, C, Cpad, ldi, scale)
                    G.run(torch, ffi, lambda: L.r3g_op_cast_pad(ptr(xb, OFF), ldi, ptr(out, OFF), ldo, rows, C, Cpad, scale, G.stream(torch)), tag)
                    bad = VB.bit_mismatches(out[oi], want)
                    diff += bad
                    if bad:
                        failures.append("%s: %d elements differ (%d of them in the padding columns)" % (tag, bad, VB.bit_mismatches(out[oi][:, C:], want[:, C:])))
                    guard_finding(torch, failures, tag, out, oi)
    finish("cast_pad", diff, failures, bit_exact=True)


def test_fill_rows_and_add_rows(env):
    torch, L, ffi = env
    diff, failures = 0, []
    for rows in VB.ROWS_ROWS:
        for C in VB.ROWS_C:
            x, pos, vals = VB.rows_case(rows, C, "cuda")
            ld = C + VB.ROWS_PAD
            idx = rows_idx(torch, rows, C, ld)
            vb = placed(torch, torch.float32, OFF + C + 8, OFF + ar(torch, C), vals)
            dst = G.guarded(torch, torch.float32, OFF + (rows + 2) * ld)
            tag = "fill_rows rows %d c %d" % (rows, C)
            G.run(torch, ffi, lambda: L.r3g_op_fill_rows(ptr(dst, OFF), ld, rows, C, ptr(vb, OFF), G.stream(torch)), tag)
            bad = VB.bit_mismatches(dst[idx], vals.expand(rows, C))
            guard_finding(torch, failures, tag, dst, idx)
            xb = placed(torch, torch.float32, OFF + (rows + 2) * ld, idx, x)
            ldp = C + 2 * VB.ROWS_PAD
            pb = placed(torch, torch.float32, OFF + (rows + 2) * ldp, rows_idx(torch, rows, C, ldp), pos)
            tag2 = "add_rows rows %d c %d" % (rows, C)
            G.run(torch, ffi, lambda: L.r3g_op_add_rows(ptr(xb, OFF), ld, ptr(pb, OFF), ldp, rows, C, G.stream(torch)), tag2)
            bad2 = VB.bit_mismatches(xb[idx], x + pos)
            guard_finding(torch, failures, tag2, xb, idx)
            diff += bad + bad2
            if bad or bad2:
                failures.append("%s: %d elements differ; %s: %d" % (tag, bad, tag2, bad2))
    finish("fill_rows, add_rows", diff, failures, bit_exact=True)


def test_vec_add_both_forms(env):
    torch, L, ffi = env
    diff, failures = 0, []
    for n in VB.VADD_N:
        a, b = VB.vadd_case(n, "cuda")
        idx = OFF + ar(torch, n)
        ab, bb = (placed(torch, torch.float32, OFF + n + 8, idx, v) for v in (a, b))
        out = G.guarded(torch, torch.float32, OFF + n + 8)
        G.run(torch, ffi, lambda: L.r3g_op_vec_add(ptr(ab, OFF), ptr(bb, OFF), ptr(out, OFF), n, G.stream(torch)), "vec_add n %d" % n)
        bad = VB.bit_mismatches(out[idx], a + b)
        guard_finding(torch, failures, "vec_add n %d" % n, out, idx)
        for name, pa, pb, want in (("a null", None, ptr(bb, OFF), torch.zeros_like(b) + b), ("b null", ptr(ab, OFF), None, a + torch.zeros_like(a))):
            out = G.guarded(torch, torch.float32, OFF + n + 8)          # a null operand stands for zeros
            G.run(torch, ffi, lambda: L.r3g_op_vec_add(pa, pb, ptr(out, OFF), n, G.stream(torch)), "vec_add n %d, %s" % (n, name))
            bad += VB.bit_mismatches(out[idx], want)
            guard_finding(torch, failures, "vec_add n %d, %s" % (n, name), out, idx)
        G.run(torch, ffi, lambda: L.r3g_op_vec_add_inplace(ptr(ab, OFF), ptr(bb, OFF), n, G.stream(torch)), "vec_add_inplace n %d" % n)
        bad2 = VB.bit_mismatches(ab[idx], a + b)
        guard_finding(torch, failures, "vec_add_inplace n %d" % n, ab, idx)
        diff += bad + bad2
        if bad or bad2:
            failures.append("n %d: vec_add %d elements differ, vec_add_inplace %d" % (n, bad, bad2))
    finish("vec_add, vec_add_inplace", diff, failures, bit_exact=True)


def test_f32_to_bf16(env):
    torch, L, ffi = env
    diff, failures = 0, []
    for name, x in [("n %d" % n, VB.f2b_case(n, "cuda")) for n in VB.F2B_N] + [("specials", VB.F2B_SPECIALS.cuda())]:
        n = x.numel()
        idx = OFF + ar(torch, n)
        xb = placed(torch, torch.float32, OFF + n + 8, idx, x)
        VB.ibits(xb)[idx] = VB.ibits(x)          # (bit patterns: a NaN's payload must arrive as drawn)
        out = G.guarded(torch, torch.bfloat16, OFF + n + 8)
        G.run(torch, ffi, lambda: L.r3g_op_f32_to_bf16(ptr(xb, OFF), ptr(out, OFF), n, G.stream(torch)), "f32_to_bf16 " + name)
        bad = VB.f2b_mismatches(out[idx], x)
        diff += bad
        if bad:
            failures.append("f32_to_bf16 %s: %d elements differ: got %s" % (name, bad, [hex(v & 0xFFFF) for v in VB.ibits(out[idx]).tolist()][:16]))
        guard_finding(torch, failures, "f32_to_bf16 " + name, out, idx)
    finish("f32_to_bf16", diff, failures, bit_exact=True)


def test_patch_rows(env):
    torch, L, ffi = env
    diff, failures = 0, []
    for S, ps, Kpad in VB.PATCH_SHAPES:
        img = VB.patch_case(S, "cuda")
        want = VB.patch_expected(img, S, ps, Kpad)
        ib = placed(torch, torch.float32, OFF + 3 * S * S + 8, OFF + ar(torch, 3 * S * S), img)
        n = want.numel()
        idx = OFF + ar(torch, n).view(want.shape)
        out = G.guarded(torch, torch.bfloat16, OFF + n + 2 * Kpad)
        tag = "patch_rows s %d ps %d kpad %d" % (S, ps, Kpad)
        G.run(torch, ffi, lambda: L.r3g_op_patch_rows(ptr(ib, OFF), S, ps, ptr(out, OFF), Kpad, G.stream(torch)), tag)
        bad = VB.bit_mismatches(out[idx], want)
        diff += bad
        if bad:
            failures.append("%s: %d elements differ" % (tag, bad))
        guard_finding(torch, failures, tag, out, idx)
    finish("patch_rows", diff, failures, bit_exact=True)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def refusals(env, name, fn, order, base, bad, buffers):
    """every entry of bad (what -> the arguments that change) is refused with nothing written; the base call is admitted"""
    torch, L, ffi = env
    call = lambda a: (lambda: fn(*([a[k] for k in order] + [G.stream(torch)])))
    for what, change in bad.items():
        G.refused(torch, L, call(dict(base, **change)), buffers, "%s, %s" % (name, what))
    G.run(torch, ffi, call(base), name + ", an admitted call")


def test_gemv_refusals(env):
    torch, L, ffi = env
    B, K, N = 3, 16, 5
    ldw = K + 8
    x = torch.zeros(B * K, device="cuda")          # (a refused call launches nothing: only the admitted one reads it)
    w = torch.zeros(OFF + (N + 1) * (ldw + 8), device="cuda", dtype=torch.bfloat16)
    bias = torch.zeros(N, device="cuda")
    y = G.guarded(torch, torch.float32, OFF + 8 * N + 8)
    base = dict(x=ptr(x), b=B, k=K, w=ptr(w, OFF), ldw=ldw, bias=ptr(bias), y=ptr(y, OFF), n=N, si=0, so=0)
    bad = {"x null": dict(x=None), "w null": dict(w=None), "y null": dict(y=None), "b 0": dict(b=0), "b 9": dict(b=9), "k 0": dict(k=0), "k % 8": dict(k=12),
           "n 0": dict(n=0), "b * k * 4 > 65536": dict(b=2, k=8200, ldw=8200), "ldw % 8": dict(ldw=K + 4), "ldw < k": dict(ldw=K - 8),
           "w 8 bytes off": dict(w=ptr(w, OFF + 4))}
    refusals(env, "r3g_op_gemv", L.r3g_op_gemv, ("x", "b", "k", "w", "ldw", "bias", "y", "n", "si", "so"), base, bad, (y,))


def test_gemv_multi_refusals(env):
    torch, L, ffi = env
    B, K, Ns = 2, 16, (1, 5)
    x = torch.zeros(B * K, device="cuda")
    ws = [torch.zeros(OFF + (n + 1) * (K + 16), device="cuda", dtype=torch.bfloat16) for n in Ns]
    bias = torch.zeros(8, device="cuda")
    y = G.guarded(torch, torch.float32, OFF + 64)
    keep = []

    def arr(ctype, values):
        a = (ctype * len(values))(*values)
        keep.append(a)
        return ctypes.addressof(a)

    wp = [ptr(t, OFF) for t in ws]
    base = dict(x=ptr(x), b=B, k=K, w=arr(ctypes.c_void_p, wp), bias=arr(ctypes.c_void_p, [ptr(bias), None]), ldw=arr(ctypes.c_int64, [K + 8, K + 16]),
                n=arr(ctypes.c_int, list(Ns)), off=arr(ctypes.c_int64, [20, 3]), nj=2, y=ptr(y, OFF), si=0)
    bad = {"x null": dict(x=None), "y null": dict(y=None), "w array null": dict(w=None), "ldw array null": dict(ldw=None), "n array null": dict(n=None),
           "out_off array null": dict(off=None), "b 0": dict(b=0), "b 3": dict(b=3), "k % 8": dict(k=12), "k 0": dict(k=0), "njobs 0": dict(nj=0),
           "a job's w null": dict(w=arr(ctypes.c_void_p, [wp[0], None])), "a job's w 8 bytes off": dict(w=arr(ctypes.c_void_p, [wp[0], ptr(ws[1], OFF + 4)])),
           "a job's ldw % 8": dict(ldw=arr(ctypes.c_int64, [K + 8, K + 4])), "a job's ldw < k": dict(ldw=arr(ctypes.c_int64, [K - 8, K + 16])),
           "a job's n 0": dict(n=arr(ctypes.c_int, [1, 0])), "a job's out_off < 0": dict(off=arr(ctypes.c_int64, [20, -1])),
           "b * k * 4 > 65536": dict(k=8200, ldw=arr(ctypes.c_int64, [8200, 8200]))}
    refusals(env, "r3g_op_gemv_multi", L.r3g_op_gemv_multi, ("x", "b", "k", "w", "bias", "ldw", "n", "off", "nj", "y", "si"), base, bad, (y,))


def test_timestep_embedding_refusals(env):
    torch, L, ffi = env
    t = torch.zeros(2, device="cuda")
    out = G.guarded(torch, torch.float32, OFF + 2 * 256 + 8)
    base = dict(t=ptr(t), ts=0.5, b=2, tf=1000.0, out=ptr(out, OFF))
    refusals(env, "r3g_op_timestep_embedding", L.r3g_op_timestep_embedding, ("t", "ts", "b", "tf", "out"), base,
             {"out null": dict(out=None), "b 0": dict(b=0), "b -1": dict(b=-1)}, (out,))


def test_fourier_refusals(env):
    torch, L, ffi = env
    out = G.guarded(torch, torch.bfloat16, OFF + 12 * 64)
    lst = torch.zeros(8, device="cuda", dtype=torch.int32)
    base = dict(out=ptr(out, OFF), start=0, count=8, r=1, bound=1.0, nf=8, pi=1)
    bad = {"out null": dict(out=None), "start < 0": dict(start=-1), "count 0": dict(count=0), "r 0": dict(r=0), "num_freqs < 0": dict(nf=-1),
           "3 + 6 num_freqs > 64": dict(nf=11)}
    refusals(env, "r3g_op_fourier_grid", L.r3g_op_fourier_grid, ("out", "start", "count", "r", "bound", "nf", "pi"), base, bad, (out,))
    base = dict(out=ptr(out, OFF), list=ptr(lst), count=8, rows=10, r=1, bound=1.0, nf=8, pi=1)
    bad = {"out null": dict(out=None), "list null": dict(list=None), "count 0": dict(count=0), "rows 0": dict(rows=0, count=0), "count > rows": dict(count=8, rows=7),
           "r 0": dict(r=0), "num_freqs < 0": dict(nf=-1), "3 + 6 num_freqs > 64": dict(nf=11), "out 8 bytes off": dict(out=ptr(out, OFF + 4))}
    refusals(env, "r3g_op_fourier_points", L.r3g_op_fourier_points, ("out", "list", "count", "rows", "r", "bound", "nf", "pi"), base, bad, (out,))


def test_euler_and_flag_refusals(env):
    torch, L, ffi = env
    n = 5
    lat = G.guarded(torch, torch.float32, OFF + n + 8)
    v = torch.zeros(2 * n, device="cuda")
    base = dict(lat=ptr(lat, OFF), v=ptr(v), n=n, g=2.0, ds=-0.02)
    bad = {"lat null": dict(lat=None), "v null": dict(v=None), "n 0": dict(n=0), "n < 0": dict(n=-4)}
    refusals(env, "r3g_op_cfg_euler", L.r3g_op_cfg_euler, ("lat", "v", "n", "g", "ds"), base, bad, (lat,))
    refusals(env, "r3g_op_euler_step", L.r3g_op_euler_step, ("lat", "v", "n", "ds"), base, bad, (lat,))
    flag = G.guarded(torch, torch.float32, OFF + 1 + 8)
    flag.view(torch.int32)[OFF] = 0
    base = dict(x=ptr(v), n=n, flag=ptr(flag, OFF))
    refusals(env, "r3g_op_nonfinite_flag", L.r3g_op_nonfinite_flag, ("x", "n", "flag"), base,
             {"x null": dict(x=None), "flag null": dict(flag=None), "n 0": dict(n=0), "n < 0": dict(n=-1)}, (flag,))


def test_cast_and_copy_refusals(env):
    torch, L, ffi = env
    rows, C, Cpad = 3, 5, 8
    xin = torch.zeros(rows * (C + 3), device="cuda")
    out = G.guarded(torch, torch.bfloat16, OFF + (rows + 2) * (Cpad + 8))
    base = dict(i=ptr(xin), ldi=C + 3, o=ptr(out, OFF), ldo=Cpad + 8, rows=rows, c=C, cpad=Cpad, scale=1.0)
    bad = {"in null": dict(i=None), "out null": dict(o=None), "rows 0": dict(rows=0), "c 0": dict(c=0), "cpad < c": dict(cpad=4), "ldi < c": dict(ldi=4),
           "ldo < cpad": dict(ldo=7)}
    refusals(env, "r3g_op_cast_pad", L.r3g_op_cast_pad, ("i", "ldi", "o", "ldo", "rows", "c", "cpad", "scale"), base, bad, (out,))
    dst = G.guarded(torch, torch.float32, OFF + (rows + 2) * (C + 3))
    vals = torch.zeros(C + 3, device="cuda")
    base = dict(d=ptr(dst, OFF), ld=C + 3, rows=rows, c=C, v=ptr(vals))
    bad = {"dst null": dict(d=None), "vals null": dict(v=None), "rows 0": dict(rows=0), "c 0": dict(c=0), "ld < c": dict(ld=C - 1)}
    refusals(env, "r3g_op_fill_rows", L.r3g_op_fill_rows, ("d", "ld", "rows", "c", "v"), base, bad, (dst,))
    base = dict(x=ptr(dst, OFF), ldx=C + 3, p=ptr(xin), ldp=C + 3, rows=rows, c=C)
    bad = {"x null": dict(x=None), "pos null": dict(p=None), "rows 0": dict(rows=0), "c 0": dict(c=0), "ldx < c": dict(ldx=C - 1), "ldp < c": dict(ldp=C - 1)}
    refusals(env, "r3g_op_add_rows", L.r3g_op_add_rows, ("x", "ldx", "p", "ldp", "rows", "c"), base, bad, (dst,))
    base = dict(i=ptr(xin), o=ptr(out, OFF), n=7)
    refusals(env, "r3g_op_f32_to_bf16", L.r3g_op_f32_to_bf16, ("i", "o", "n"), base, {"in null": dict(i=None), "out null": dict(o=None), "n 0": dict(n=0), "n < 0": dict(n=-7)}, (out,))
    base = dict(y=ptr(dst, OFF), x=ptr(xin), n=7)
    refusals(env, "r3g_op_vec_add_inplace", L.r3g_op_vec_add_inplace, ("y", "x", "n"), base, {"y null": dict(y=None), "x null": dict(x=None), "n 0": dict(n=0), "n < 0": dict(n=-7)}, (dst,))
    base = dict(a=ptr(xin), b=ptr(vals), o=ptr(dst, OFF), n=7)
    refusals(env, "r3g_op_vec_add", L.r3g_op_vec_add, ("a", "b", "o", "n"), base,
             {"out null": dict(o=None), "n 0": dict(n=0), "n < 0": dict(n=-7)}, (dst,))          # (a null a or b is admitted: zeros)


def test_patch_rows_refusals(env):
    torch, L, ffi = env
    S, ps, Kpad = 4, 2, 16
    img = torch.zeros(3 * S * S, device="cuda")
    out = G.guarded(torch, torch.bfloat16, OFF + 4 * Kpad + 16)
    base = dict(img=ptr(img), s=S, ps=ps, o=ptr(out, OFF), kpad=Kpad)
    bad = {"img null": dict(img=None), "out null": dict(o=None), "s 0": dict(s=0), "ps 0": dict(ps=0), "s % ps": dict(ps=3), "ps > s": dict(ps=8, kpad=192),
           "kpad < 3 ps^2": dict(kpad=11)}
    refusals(env, "r3g_op_patch_rows", L.r3g_op_patch_rows, ("img", "s", "ps", "o", "kpad"), base, bad, (out,))


# ---- every kernel form was reached ------------------------------------------------------------------------------------------------------
def test_every_form_was_reached(env):
    """both Euler kernels (the float4 one with and without a tail, and with nothing but a tail) and both grid rules of gemv_launch (the
    capped grid with a second pass over the rows), each by a launch that met its bound -- as the restated launch rules compute it"""
    run_euler(env)
    run_gemv(env)
    assert {("vec", False, True), ("vec", True, True), ("vec", True, False), ("scalar", True, True), ("scalar", False, True)} <= EULER_REACHED, EULER_REACHED
    assert {("blocks 256", True), ("blocks n / 4", False)} <= GEMV_REACHED, GEMV_REACHED
