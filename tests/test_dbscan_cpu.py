"""DBSCAN on the host: the twin of csrc/dbscan_core.h as all-pairs brute force and through the grid walk
(tests/emu_dbscan.py), the numpy restatement written from the definition (tests/dbscan_ref.py), the goldens recorded from
scikit-learn and from the reference's filters (tools/make_dbscan_goldens.py) and, where it imports, live scikit-learn: all
equal, exactly, on every cloud.  Every output is an integer, so there is no tolerance anywhere in this file."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-re-gen_amd"))

import dbscan_ref as R  # noqa: E402
import emu_build  # noqa: E402
import emu_dbscan as E  # noqa: E402

RESOLUTIONS = (1, 3, 16, 0)          # 0: automatic
NAMES = tuple(R.RANDOM) + tuple(R.fixed_clouds())
_REF = {}


def reference(name):
    """the restatement's answer, computed once and left unchanged"""
    if name not in _REF:
        p, eps, ms = R.clouds()[name]
        r = R.dbscan(p, eps, ms)
        for k in ("labels", "counts", "core"):
            r[k].setflags(write=False)
        _REF[name] = r
    return _REF[name]


def same(a, b, counts=True):
    return (np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["core"], b["core"]) and a["report"] == b["report"]
            and (not counts or np.array_equal(a["counts"], b["counts"])))


@pytest.mark.parametrize("name", NAMES)
def test_twin_brute_equals_twin_grid_equals_restatement(name):
    p, eps, ms = R.clouds()[name]
    ref = reference(name)
    assert same(E.brute(p, eps, ms), ref), name
    for res in RESOLUTIONS:
        for rev in (False, True):
            g = E.grid(p, eps, ms, res, rev)
            assert same(g, ref), (name, res, rev)
            if res and ref["report"]["n_usable"]:
                assert g["resolution"] == res


@pytest.mark.parametrize("name", NAMES)
def test_stopping_the_count_at_min_samples_changes_no_flag_and_no_label(name):
    p, eps, ms = R.clouds()[name]
    ref = reference(name)
    assert same(E.brute(p, eps, ms, early=True), ref, counts=False)
    g = E.grid(p, eps, ms, early=True)
    assert same(g, ref, counts=False)
    assert (g["counts"] <= max(ms, 1)).all() and np.array_equal(g["counts"] >= ms, ref["core"])


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_recorded_scikit_learn_labels(name):
    _, expect = R.golden()
    e = expect["clouds"][name]
    p, eps, ms = R.clouds()[name]
    assert (e["eps"], e["min_samples"], e["n"]) == (eps, ms, len(p))
    if "labels" not in e:
        assert len(p) == 0 or not np.isfinite(p).all()           # scikit-learn refuses these
        return
    ref = reference(name)
    assert np.array_equal(ref["labels"], e["labels"]) and np.array_equal(np.nonzero(ref["core"])[0], e["core"])


@pytest.mark.parametrize("name", NAMES)
def test_equals_live_scikit_learn(name):
    cluster = pytest.importorskip("sklearn.cluster")
    p, eps, ms = R.clouds()[name]
    if len(p) == 0 or not np.isfinite(p).all():
        return
    db = cluster.DBSCAN(eps=eps, min_samples=ms).fit(p)
    ref = reference(name)
    assert np.array_equal(ref["labels"], db.labels_) and np.array_equal(np.nonzero(ref["core"])[0], db.core_sample_indices_)


def test_the_clouds_are_what_they_claim():
    c = R.clouds()
    r = reference("chain")["report"]
    assert len(c["chain"][0]) == 4097 and (r["n_clusters"], r["n_noise"], r["n_core"]) == (1, 0, 4097)
    assert np.array_equal(reference("isolated")["labels"], np.arange(len(c["isolated"][0])))
    for name in ("lattice6", "lattice7"):                   # every neighbour of a lattice point is exactly eps away
        ms = c[name][2]
        counts = reference(name)["counts"]
        assert set(np.unique(counts)) == {4, 5, 6, 7} and (reference(name)["core"] == (counts >= ms)).all()
    assert reference("lattice7")["report"]["n_core"] == 343
    dup = reference("duplicates")
    assert (dup["counts"] % 5 == 0).all() and dup["report"]["n_border"] == 0       # a point's copies are distinct neighbours
    for name in ("slabs_ab", "slabs_ba"):                   # the contested point goes to the slab whose core has the lower index
        lab = reference(name)["labels"]
        assert lab[-1] == 0 and lab[1] == 0 and lab[28] == 1 and reference(name)["counts"][-1] == 3
    assert reference("slabs_ab")["labels"][0] == 1 and reference("slabs_ba")["labels"][0] == 0
    big = reference("bigeps")
    assert (big["counts"] == 300).all() and big["report"]["n_clusters"] == 1
    nf = reference("nonfinite")
    bad = ~np.isfinite(c["nonfinite"][0]).all(1)
    assert bad.sum() == 90 and (nf["labels"][bad] == -1).all() and (nf["counts"][bad] == 0).all() and nf["report"]["n_usable"] == 1410
    zero = dict(zip(R.REPORT, (0, 0, 0, 0, 0, -1, 0)))
    assert reference("n0")["report"] == zero and reference("all_nonfinite")["report"] == zero
    far = c["far"]
    assert (far[0].max(0) - far[0].min(0)).max() / far[1] > 1000 and reference("far")["report"]["n_clusters"] == 4


def test_automatic_resolution_rule():
    """floor(longest extent / eps), at least 1, at most 256 and at most the largest r with r^3 <= 8 * usable"""
    def rule(ext, eps, n):
        cap = 1
        while cap < 256 and (cap + 1) ** 3 <= 8 * n:
            cap += 1
        return max(1, min(cap, int(min(ext / eps, 1e9))))
    for ext, eps, n in ((1.0, 0.25, 729), (2.0, 0.25, 729), (1.0, 10.0, 300), (100.0, 0.02, 626), (1024.0, 0.25, 4097), (1.0, 1e-3, 10 ** 7),
                        (1.0, 1e-3, 2 ** 31 - 1), (0.0, 0.1, 5), (3.0, 1.0, 1), (7.9, 1.0, 10 ** 6)):
        lo, hi = np.zeros(3, np.float32), np.array([ext, ext / 2, 0], np.float32)
        assert E.auto_resolution(lo, hi, eps, n) == rule(float(np.float32(ext)), eps, n), (ext, eps, n)
    assert E.grid(R.clouds()["far"][0], 0.02, 5)["resolution"] == 17            # capped by the points, most cells empty
    assert E.grid(R.clouds()["lattice6"][0], 0.25, 6)["resolution"] == 8


@pytest.mark.parametrize("mutant", sorted(E.MUTANTS))
def test_every_mutant_of_the_twin_falls_outside_a_cloud(mutant):
    """`<` for `<=`, a float32 d2, a point that does not count itself, a border point that takes the largest label, and clusters
    numbered by first appearance: each must change the labels of at least one cloud, or the clouds would not test that rule"""
    seen = [name for name in NAMES if not np.array_equal(E.brute(*R.clouds()[name], mutant=mutant)["labels"], reference(name)["labels"])]
    assert seen, mutant
    expected = {"strict_less": "lattice6", "float32_d2": "rounding", "not_itself": "isolated", "border_max": "slabs_ab",
                "first_appearance": "slabs_ab"}[mutant]
    assert expected in seen, (mutant, seen)


def test_refusals_of_the_twin():
    p = R.clouds()["n63"][0]
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(min_samples=0)):
        args = dict(eps=0.2, min_samples=3)
        args.update(kw)
        with pytest.raises(ValueError):
            E.brute(p, **args)
    for res in (-1, 257):
        with pytest.raises(ValueError):
            E.grid(p, 0.2, 3, res)


def test_filters_equal_the_reference_on_the_goldens():
    """filter_dbscan keeps the largest cluster of the labels; filter_points_by_quantile is torch.quantile and a mask, the same
    on any device.  The kept rows are those the reference kept (tools/make_dbscan_goldens.py ran it)."""
    import torch
    from r3g import cloud
    pts, expect = R.golden()
    for name in R.RANDOM:
        e = expect["clouds"][name]
        assert np.array_equal(R.largest_cluster_rows(reference(name)["labels"]), e["dbscan_keep"]), name
        if e["quantile_keep"] is not None:
            kept = cloud.filter_points_by_quantile(torch.from_numpy(pts[name]), e["q"]).numpy()
            assert np.array_equal(kept, pts[name][e["quantile_keep"]]), name
    assert sum(expect["clouds"][name]["quantile_keep"] is not None for name in R.RANDOM) >= 3
    empty = torch.zeros((0, 3))
    assert cloud.filter_points_by_quantile(empty) is empty
    one = torch.tensor([[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [2.0, 2.0, 0.0]])
    assert cloud.filter_points_by_quantile(one, 0.4) is one                      # nothing would remain: the input itself


def test_selftest_program_under_sanitizers():
    """the twin with its own main(), built as a stand-alone program with -fsanitize=address,undefined (runtimes linked
    statically), on the lattice at resolutions 1 to 256; never loaded into Python"""
    if not emu_build.sanitizers_link():
        pytest.skip("no sanitizer runtime for g++ on this machine")
    exe = E.selftest_binary(sanitize=True)      # (a compile error of the twin's program is a failure, not a skip)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr
