"""The plane fit without a GPU: the host twin of csrc/plane_core.h (tests/emu_plane.py) in its two modes against each other and
against the numpy restatement of the definition (tests/plane_ref.py) on the named clouds; the twin's mutants, each exposed by a
named cloud; the reference's recorded fits and yaw losses (tools/make_plane_goldens.py); the sanitised stand-alone twin; the
refusals that the library decides on host state."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import emu_build
import emu_plane as E
import plane_ref as R

NAMES = tuple(R.clouds())
_BRUTE = {}


def brute(name):
    """the twin's plain loops, computed once and left unchanged"""
    if name not in _BRUTE:
        t = E.brute(*R.clouds()[name])
        for k in ("counts", "mask", "plane"):
            t[k].setflags(write=False)
        _BRUTE[name] = t
    return _BRUTE[name]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "plane_expect.json")) as f:
        expect = json.load(f)
    return expect, np.load(os.path.join(golden_dir, "plane_clouds.npz"))


def same(a, b):
    return np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["mask"], b["mask"]) and a["report"] == b["report"]


def rel(a, b):
    """max |a - b| over max |b| (norm-wise: a scatter's off-diagonal entries may be zero)"""
    scale = np.abs(b).max()
    return np.abs(np.asarray(a) - np.asarray(b)).max() / scale if scale else np.abs(a).max()


def test_the_named_clouds_are_what_they_claim():
    c = R.clouds()
    assert len(NAMES) == 7
    assert brute("collinear")["report"]["n_valid"] == 0 and brute("collinear")["report"]["best"] == -1
    tie = brute("planes_tie")
    assert len(set(tie["counts"].tolist())) == 1 and tie["report"]["best"] == 0 and tie["report"]["best_count"] == 100
    assert brute("nonfinite")["report"]["n_usable"] == len(c["nonfinite"][0]) - 4
    p = c["duplicates"][0]
    assert len(np.unique(p, axis=0)) < len(p) and brute("duplicates")["counts"][:5].tolist()[:4] == [0, 0, 0, 0]
    p = c["mirror_slab"][0].astype(np.float64)
    assert np.array_equal(np.sort(p, axis=0), np.sort(-p, axis=0)) and p[:, 0].std() > p[:, 2].std() > p[:, 1].std()


@pytest.mark.parametrize("name", NAMES)
def test_twin_modes_equal_each_other_and_the_restatement(name):
    p, t, thr = R.clouds()[name]
    a, r = brute(name), R.ransac(p, t, thr)
    for splits in (1, 2, 5):
        b = E.blocks(p, t, thr, splits)
        assert same(a, b) and a["plane"].tobytes() == b["plane"].tobytes(), (name, splits)
    assert np.array_equal(a["counts"], r["counts"]) and np.array_equal(a["mask"], r["mask"]) and a["report"] == r["report"], name
    assert np.array_equal(a["plane"][0:3], r["p0"]) and np.array_equal(a["plane"][3:6], r["normal"]), name


@pytest.mark.parametrize("name", NAMES)
def test_moments_against_the_restatement(name):
    """float64 sums of n terms in another order: 8 n 2^-53, relative to the largest entry.  The normal is compared where the two
    smallest eigenvalues are apart (otherwise the direction is not determined: the collinear cloud)"""
    p, t, thr = R.clouds()[name]
    bound = 8 * len(p) * 2.0 ** -53
    for mask in (None, brute(name)["mask"]):
        m, r = E.moments(p, mask), R.moments(p, mask)
        o = m["out"]
        assert m["report"] == {"n": r["n"], "skipped": r["skipped"], "few": r["few"]} and o[0] == r["n"], name
        assert rel(o[1:4], r["centroid"]) <= bound and rel(o[4:10], r["scatter"]) <= bound, name
        val = r["eigenvalues"]
        assert np.all(np.diff(o[10:13]) >= 0) and np.abs(o[10:13] - val).max() <= 64 * bound * max(np.abs(val).max(), 1e-300), name
        if r["n"] >= 3 and val[1] - val[0] > 1e-6 * val[2]:
            assert o[14] >= 0 and abs(np.linalg.norm(o[13:16]) - 1) <= 1e-15 and rel(o[13:16], r["normal"]) <= bound, name
        if r["few"]:
            assert o[13:16].tolist() == [0.0, 1.0, 0.0], name
    # the refinement inside the RANSAC call is the moments of its mask
    assert brute(name)["plane"][6:15].tobytes() == np.concatenate([E.moments(p, brute(name)["mask"])["out"][[1, 2, 3, 13, 14, 15, 10, 11, 12]]]).tobytes()


@pytest.mark.parametrize("mutant", tuple(E.MUTANTS))
def test_every_mutant_is_caught_by_a_named_cloud(mutant):
    caught = [name for name in NAMES if not same(E.brute(*R.clouds()[name], mutant=mutant), brute(name))]
    assert caught, mutant
    expected = {"less_equal": "planes_tie", "float32_distance": "tilted", "last_on_tie": "planes_tie", "skip_validity": "collinear"}
    assert expected[mutant] in caught, (mutant, caught)


def test_small_sets_and_edges():
    p = R.uniform(3, 8)
    for n in (0, 1, 2):
        m = E.moments(p[:n])
        assert m["report"] == {"n": n, "skipped": 0, "few": 1} and m["out"][13:16].tolist() == [0.0, 1.0, 0.0]
        r = E.brute(p[:n], [[0, 1, 2]], 0.05)
        assert r["report"]["best"] == -1 and r["report"]["n_valid"] == 0 and not r["mask"].any()
    r = E.brute(p, np.zeros((0, 3), np.int32), 0.05)
    assert r["report"] == {"n_usable": 8, "n_valid": 0, "best": -1, "best_count": 0, "few": 1}
    with pytest.raises(ValueError):
        E.brute(p, [[0, 1, 2]], 0.0)
    with pytest.raises(ValueError):
        E.brute(p, [[0, 1, 2]], float("nan"))


def test_ransac_against_the_reference(golden):
    """the reference's run of fit_plane_ransac_refined on its own triples: its mask and count exactly (the clouds were chosen
    with no distance near the threshold), its float32 mean of the inliers within n 2^-24 max|p|"""
    expect, clouds = golden
    assert len(expect["ransac"]) >= 3
    for name, e in expect["ransac"].items():
        p = clouds[name]
        assert p.shape == (expect["n"], 3) and len(e["triples"]) == expect["h"]
        for r in (E.brute(p, e["triples"], expect["threshold"]), R.ransac(p, e["triples"], expect["threshold"])):
            assert np.flatnonzero(r["mask"]).tolist() == e["mask_rows"], name
            assert r["report"]["best_count"] == e["count"] == int(r["counts"][r["report"]["best"]]), name
        c = E.brute(p, e["triples"], expect["threshold"])["plane"][6:9]
        assert np.abs(c - np.array(e["centroid"])).max() <= len(p) * 2.0 ** -24 * np.abs(p).max(), name


def test_svd_normal_against_the_reference_on_the_mirror_slab(golden):
    """the one input on which the reference's fit_plane_svd is claimed (its column of Vh is the eigenvector only where the
    eigenvector matrix is symmetric up to signs).  Its scatter is a float32 product: entries off by n 2^-24 of the largest, so
    by Davis-Kahan the direction may turn by 4 n 2^-24 lambda_max / (lambda_2 - lambda_1)"""
    expect, clouds = golden
    p = clouds["mirror_slab"]
    assert np.array_equal(p, R.clouds()["mirror_slab"][0])
    o = E.moments(p)["out"]
    val = o[10:13]
    bound = 4 * len(p) * 2.0 ** -24 * val[2] / (val[1] - val[0])
    assert bound < 1e-2
    ref = np.array(expect["svd"]["mirror_slab"]["svd_normal"])
    cosine = abs(float(np.dot(o[13:16], ref))) / np.linalg.norm(ref)
    angle = float(np.arccos(min(1.0, cosine)))
    print("angle to the reference's normal %.3e rad, allowed %.3e" % (angle, bound))
    assert angle <= bound and ref[1] > 0 and o[14] > 0


def test_yaw_losses_against_the_reference(golden):
    """float32 rotations and squared distances of at most 3 terms in the recorded run: 1e-4 relative"""
    expect, clouds = golden
    assert len(expect["yaw"]) >= 2
    for name, e in expect["yaw"].items():
        losses, index = R.yaw_losses(clouds[name + "_verts"], clouds[name + "_target"], 18, "bbox")
        assert index == e["argmin"], name
        rec = np.array(e["losses"])
        assert rec.min() > 0 and np.all(np.abs(losses - rec) <= 1e-4 * rec), (name, (np.abs(losses - rec) / rec).max())      # every loss against itself
        assert np.allclose(R.yaw_rotation(np.linspace(0, 2 * 3.14159, 18)[index]), np.array(e["rotation"]), atol=1e-6), name


def test_frame_and_box_definitions():
    m, inv = R.plane_frame([0.0, 2.0, 0.0], [1.0, 2.0, 3.0])
    assert np.allclose(m @ inv, np.eye(4), atol=1e-15) and np.allclose(m[:3, 1], [0, 1, 0]) and np.allclose(m[:3, 3], [1, 2, 3])
    assert abs(np.linalg.det(m[:3, :3]) - 1) < 1e-12
    m, _ = R.plane_frame([0.95, 0.3, 0.0], [0, 0, 0])
    assert abs(np.linalg.det(m[:3, :3]) - 1) < 1e-12 and np.allclose(m[:3, :3].T @ m[:3, :3], np.eye(3), atol=1e-12)
    rng = np.random.default_rng(1)
    box = rng.uniform(-1, 1, (4000, 3)) * [2.0, 0.3, 0.5]
    c, rot, ext = R.yaw_obb(box @ R.yaw_rotation(0.6).T + [1.0, 2.0, 3.0])
    assert np.allclose(c, [1, 2, 3], atol=0.05) and np.allclose(ext, [4.0, 0.6, 1.0], atol=0.05)
    assert abs(abs(rot[0, 0]) - np.cos(0.6)) < 0.02 and np.allclose(rot[1], [0, 1, 0])


def test_selftest_program_under_sanitizers():
    """the twin with its own main(), built as a stand-alone program with -fsanitize=address,undefined (runtimes linked
    statically), on a lattice whose layers tie with the threshold; never loaded into Python"""
    if not emu_build.sanitizers_link():
        pytest.skip("no sanitizer runtime for g++ on this machine")
    # (a compile error of the twin's program is a failure, not a skip: the probe above has shown that the sanitizers link)
    exe = E.selftest_binary(sanitize=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


def test_refusals_decided_on_host_state():
    """every argument check of r3g_plane_ransac and r3g_plane_moments precedes the first use of the context, so the refusals
    can be read without a GPU: R3G_ERR_INVALID (-1) and a text that names the argument"""
    from r3g import ffi
    L = ffi.lib()
    rep, plane, out, rep4 = (ctypes.c_int64 * 8)(), (ctypes.c_double * 16)(), (ctypes.c_double * 16)(), (ctypes.c_int64 * 4)()
    buf = (ctypes.c_float * 12)()
    bp = ctypes.cast(buf, ctypes.c_void_p)

    def ransac(n=4, h=1, thr=0.05, points=bp, triples=bp, report=rep, pl=plane):
        rc = L.r3g_plane_ransac(None, points, n, triples, h, thr, None, None, report, pl, None)
        return rc, L.r3g_last_error().decode()

    for kw, word in (({"thr": 0.0}, "threshold"), ({"thr": -1.0}, "threshold"), ({"thr": float("nan")}, "threshold"),
                     ({"thr": float("inf")}, "threshold"), ({"h": -1}, "n_hyp"), ({"h": 65537}, "n_hyp"), ({"n": -1}, "n_points"),
                     ({"n": 2 ** 31}, "n_points"), ({"points": None}, "null buffer"), ({"triples": None}, "null buffer"),
                     ({"report": None}, "null buffer"), ({"pl": None}, "null buffer"), ({}, "null argument")):
        rc, text = ransac(**kw)
        assert rc == -1 and word in text and "r3g_plane_ransac" in text, (kw, rc, text)
    for args, word in (((None, bp, -1, None, out, rep4, None), "n_points"), ((None, bp, 2 ** 31, None, out, rep4, None), "n_points"),
                       ((None, None, 4, None, out, rep4, None), "null buffer"), ((None, bp, 4, None, None, rep4, None), "null buffer"),
                       ((None, bp, 4, None, out, None, None), "null buffer"), ((None, bp, 4, None, out, rep4, None), "null argument")):
        rc = L.r3g_plane_moments(*args)
        assert rc == -1 and word in L.r3g_last_error().decode(), (args, rc)
    assert L.r3g_plane_times(None, None) == -1
