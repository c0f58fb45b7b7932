"""Normal orientation on the host: the twin of csrc/orient_core.h (tests/emu_orient.py: Boruvka in host
loops, forward and reversed) against an independent restatement (tests/orient_ref.py: Kruskal and a breadth-first walk), exactly;
a sphere on which the outcome is known literally; and the twin as a stand-alone sanitizer build.  No GPU."""
import subprocess

import numpy as np
import pytest

import emu_build
import emu_orient as emu
import orient_ref as R

CLOUDS = R.clouds()


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_twin_equals_the_restatement_in_both_scan_orders(name):
    p, nr, k = CLOUDS[name]
    s_ref, t_ref, rep_ref = R.orient(p, nr, k)
    runs = [emu.orient(p, nr, k, reverse=rev) for rev in (False, True)]
    assert runs[0][2] == runs[1][2]
    for sign, tree, rep in runs:
        assert np.array_equal(sign, s_ref) and np.array_equal(tree, t_ref)
        assert {f: rep[f] for f in rep_ref} == rep_ref


def test_the_cases_are_what_they_claim():
    """heavily frustrated, weights all zero, two trees each led by its own top point, unusable points left out, N = 1 and 2"""
    rep = {name: emu.orient(*CLOUDS[name]) for name in CLOUDS}
    assert rep["random500"][2]["frustrated"] > 100
    assert rep["lattice9x9"][2] == {"usable": 81, "trees": 1, "flipped": 0, "rounds": 2, "frustrated": 0}
    assert rep["two_spheres"][2]["trees"] == 2 and rep["two_spheres"][2]["frustrated"] == 0
    p, nr, _ = CLOUDS["two_spheres"]
    sign, tree, _ = rep["two_spheres"]
    assert sorted(set(tree.tolist())) == [0, 300]
    centre = np.where(tree[:, None] == 0, np.zeros(3, np.float32), np.array([10, 0, 0], np.float32))
    assert (((nr * sign[:, None]) * (p - centre)).sum(1) > 0).all()          # each sphere ends outward: its top point decides
    sign, tree, r = rep["nonfinite"]
    assert r["usable"] == 196 and (sign[[3, 40, 77, 120]] == 0).all() and (tree[[3, 40, 77, 120]] == -1).all()
    assert (sign[np.setdiff1d(np.arange(200), [3, 40, 77, 120])] != 0).all()
    assert rep["one"][0].tolist() == [-1] and rep["one"][1].tolist() == [0]   # n_z < 0: the top member is reversed
    assert rep["two"][0].tolist() == [1, -1] and rep["two"][1].tolist() == [0, 0]
    assert rep["tripled_k1"][2]["trees"] == 60


def test_k_outside_1_to_31_is_refused():
    p, nr, _ = CLOUDS["two"]
    for k in (0, 32, -1):
        with pytest.raises(ValueError):
            emu.orient(p, nr, k)


def test_coin_flipped_sphere_ends_outward_without_exception():
    """4 096 points of a Fibonacci unit sphere, exact normals each reversed by a coin, k = 8: neighbouring normals are a few
    degrees apart (asserted below in float64), so the propagation rule cannot go wrong and EVERY normal must end outward"""
    p, nr = R.fibonacci_sphere(4096)
    flipped = R.coin_flipped(nr, 7)
    ok = np.ones(len(p), bool)
    nb = R.neighbours(p, ok, 8)
    n64 = nr.astype(np.float64)
    worst = min(float(n64[i] @ n64[j]) for i, row in nb.items() for j in row)
    assert worst > np.cos(np.radians(10.0))                                    # measured: about 5.6 degrees at the widest
    sign, tree, rep = emu.orient(p, flipped, 8)
    assert (((flipped * sign[:, None]).astype(np.float64) * p.astype(np.float64)).sum(1) > 0).all()
    assert rep["frustrated"] == 0 and rep["trees"] == 1 and rep["usable"] == 4096 and (tree == 0).all()
    assert rep["flipped"] == int((flipped * p).sum(1).__lt__(0).sum())


def test_twin_as_a_stand_alone_sanitizer_build():
    if not emu_build.sanitizers_link():
        pytest.skip("no sanitizer runtime for g++ on this machine")
    out = subprocess.run([emu.selftest_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
