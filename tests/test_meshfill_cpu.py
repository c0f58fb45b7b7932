"""Hole filling without a GPU: the host twin of csrc/meshfill_core.h (tests/emu_meshfill.py) against the
numpy / Python restatement (tests/meshfill_ref.py), plus literals that depend on neither: restored faces, exact centroids,
watertightness and Euler numbers of the results."""
import subprocess

import numpy as np
import pytest

import emu_build
import emu_meshfill as emu
import emu_meshtopo as temu
import meshfill_ref as ref
import meshtopo_ref as tref

ARRAYS = ("loop_start", "loop_verts", "status", "new_faces")
_CACHE = {}


def assert_twin_equals_restatement(v, f, **kw):
    e, r = emu.plan(v, f, **kw), ref.plan(v, f, **kw)
    assert e["report"] == r["report"]
    for k in ARRAYS:
        assert np.array_equal(e[k], r[k]), k
    assert e["new_verts"].tobytes() == r["new_verts"].tobytes()
    # the same plan whatever order the slots are walked in
    e2 = emu.plan(v, f, reverse=True, **kw)
    assert e2["report"] == e["report"] and all(np.array_equal(e2[k], e[k]) for k in ARRAYS + ("new_verts",))
    return e


def topology(v, f, n_verts=None):
    return temu.build(v, f, n_verts=n_verts)["report"]


def golden_a():
    """golden A's mesh (closed, one body, Euler number 2) with its topology report, computed once and read-only"""
    if "A" not in _CACHE:
        v, f = tref.golden_mesh("A")
        rep = topology(v, f)
        assert rep["boundary"] == 0 and rep["nonmanifold"] == 0 and rep["bodies"] == 1 and rep["euler"] == 2
        _CACHE["A"] = (v, f, rep)
        for a in (v, f):
            a.setflags(write=False)
    return _CACHE["A"]


def test_tetrahedron_minus_a_face():
    v, f = tref.tetrahedron()
    for k in range(4):
        rest = np.delete(f, k, axis=0)
        for mode in ("fan", "centroid"):
            e = assert_twin_equals_restatement(v, rest, mode=mode)
            assert (e["report"]["boundary"], e["report"]["loops"], e["report"]["longest"], e["report"]["filled"]) == (3, 1, 3, 1)
        e = emu.plan(v, rest)
        assert e["report"]["faces_added"] == 1 and e["report"]["rounds"] == 2
        assert np.array_equal(ref.canonical(e["new_faces"]), ref.canonical(f[k:k + 1]))       # a rotation of the removed face
        assert np.array_equal(ref.canonical(np.concatenate([rest, e["new_faces"]])), ref.canonical(f))


def test_cube_minus_one_side():
    v, f = tref.cube()
    rest = f[:-2]                               # without the side 1, 5, 7, 3: the plane z = 1
    fan = assert_twin_equals_restatement(v, rest)
    assert (fan["report"]["longest"], fan["report"]["faces_added"], fan["report"]["verts_added"]) == (4, 2, 0)
    cen = assert_twin_equals_restatement(v, rest, mode="centroid")
    assert (cen["report"]["faces_added"], cen["report"]["verts_added"]) == (4, 1)
    assert cen["new_verts"].tolist() == [[0.5, 0.5, 1.0]] and (cen["new_faces"][:, 0] == 8).all()
    for mode in ("fan", "centroid"):
        vv, ff, _ = emu.fill_holes(v, rest, mode=mode)
        rep = topology(vv, ff)
        assert rep["boundary"] == 0 and rep["nonmanifold"] == 0 and rep["clash"] == 0 and rep["euler"] == 2
        assert rep["six_volume_q"] == 6 << rep["vol_scale"]                   # the unit cube again, wound outward
        again = emu.plan(vv, ff, mode=mode)["report"]
        assert again["boundary"] == 0 and again["faces_added"] == 0 and again["rounds"] == 0
    # max_loop 3 leaves the quad alone
    e = assert_twin_equals_restatement(v, rest, max_loop=3)
    assert (e["report"]["oversize"], e["report"]["filled"], e["report"]["faces_added"]) == (1, 0, 0) and e["status"].tolist() == [1]


def test_centroid_of_a_pentagon_is_summed_in_rank_order():
    """x coordinates 2^60, 1, -2^60, 1, 1 in rank order: the float64 running sum loses the first 1 ((2^60 + 1) rounds to 2^60)
    and keeps the last two, so x = 2 / 5; summed in any order that pairs the two large terms first it would be 3 / 5"""
    v, f = ref.cone(5)
    f = np.ascontiguousarray(f)
    e0 = emu.plan(v, f, mode="centroid")
    a = e0["loop_verts"].tolist()
    assert e0["report"]["loops"] == 1 and len(a) == 5
    big = np.float32(2.0 ** 60)
    v = v.copy()
    v[a, 0] = [big, 1, -big, 1, 1]
    v[a, 1] = [1, big, 1, -big, 1]
    v[a, 2] = [3, 3, 3, 3, 4]
    e = assert_twin_equals_restatement(v, f, mode="centroid")
    want = np.array([np.float32(np.float64(2) / np.float64(5)), np.float32(np.float64(1) / np.float64(5)),
                     np.float32(np.float64(16) / np.float64(5))], np.float32)
    assert e["new_verts"].tobytes() == want.reshape(1, 3).tobytes()
    assert np.float32(np.float64(3) / np.float64(5)) != want[0]
    v[a[2], 2] = np.inf                                                        # non-finite inputs propagate
    assert np.isinf(emu.plan(v, f, mode="centroid")["new_verts"][0, 2])


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 129, 4097])
def test_open_cones(n):
    v, f = ref.cone(n)
    for faces in (f, ref.permuted(f, n)):
        for mode in ("fan", "centroid"):
            e = assert_twin_equals_restatement(v, faces, max_loop=n, mode=mode)
            assert (e["report"]["loops"], e["report"]["filled"], e["report"]["longest"], e["report"]["tangled"]) == (1, 1, n, 0)
            vv, ff, _ = emu.fill_holes(v, faces, max_loop=n, mode=mode)
            rep = topology(vv, ff)
            assert rep["boundary"] == 0 and rep["nonmanifold"] == 0 and rep["clash"] == 0 and rep["euler"] == 2
            if n > 3:
                o = assert_twin_equals_restatement(v, faces, max_loop=n - 1, mode=mode)
                assert (o["report"]["oversize"], o["report"]["faces_added"], o["report"]["verts_added"]) == (1, 0, 0)
    with pytest.raises(emu.EmuError):
        emu.plan(v, f, max_loop=2)


def test_tube_bow_tie_and_reversed_face():
    v, f = ref.tube(65)
    e = assert_twin_equals_restatement(v, f, max_loop=65)
    assert (e["report"]["loops"], e["report"]["filled"], e["report"]["faces_added"]) == (2, 2, 126)
    assert e["loop_start"].tolist() == [0, 65, 130]
    # half-edge 0 is (0 -> 1) on the lower rim, which face 0 shares with nobody: the lower rim leads
    assert e["loop_verts"][0] == 0 and set(e["loop_verts"][:65].tolist()) == set(range(65))
    v, f = ref.bow_tie()
    e = assert_twin_equals_restatement(v, f)
    assert e["report"]["boundary"] == 10 and e["report"]["tangled"] == 10 and e["report"]["loops"] == 0 and e["report"]["faces_added"] == 0
    v, f = ref.cone(7)
    bent = f.copy()
    bent[3] = bent[3, ::-1]
    e = assert_twin_equals_restatement(v, bent)
    assert e["report"]["loops"] == 0 and e["report"]["tangled"] == e["report"]["boundary"] == 7
    fixed = temu.orient(v, bent, 0)["faces"]
    e = assert_twin_equals_restatement(v, fixed, max_loop=7)
    assert (e["report"]["filled"], e["report"]["faces_added"], e["report"]["tangled"]) == (1, 5, 0)


def test_golden_a_with_disjoint_faces_removed():
    v, f, _ = golden_a()
    rng = np.random.default_rng(20)
    used = np.zeros(len(v), bool)
    gone = []
    for k in rng.permutation(len(f)):
        if len(gone) == 40:
            break
        if not used[f[k]].any():
            gone.append(int(k))
            used[f[k]] = True
    rest = np.delete(f, gone, axis=0)
    e = assert_twin_equals_restatement(v, rest)
    assert (e["report"]["loops"], e["report"]["filled"], e["report"]["longest"], e["report"]["faces_added"]) == (40, 40, 3, 40)
    filled = np.concatenate([rest, e["new_faces"]])
    assert np.array_equal(ref.canonical(filled), ref.canonical(f))
    rep = topology(v, filled)
    assert rep["boundary"] == 0 and rep["nonmanifold"] == 0 and rep["bodies"] == 1 and rep["euler"] == 2
    assert emu.plan(v, filled)["report"]["faces_added"] == 0
    assert_twin_equals_restatement(v, rest, mode="centroid")
    # faces only
    e2 = emu.plan(None, rest, n_verts=len(v))
    assert e2["report"] == e["report"] and np.array_equal(e2["new_faces"], e["new_faces"])


def test_golden_a_with_vertex_stars_removed():
    v, f, whole = golden_a()
    rng = np.random.default_rng(21)
    blocked = np.zeros(len(v), bool)
    stars = []
    for c in rng.permutation(len(v)):
        if len(stars) == 12:
            break
        ring = np.unique(f[(f == c).any(1)])
        if blocked[ring].any():
            continue
        # keep the stars two rings apart, so that no two holes touch
        ring2 = np.unique(f[np.isin(f, ring).any(1)])
        stars.append(int(c))
        blocked[ring2] = True
    star = np.isin(f, stars).any(1)
    rest = f[~star]
    valence = sorted(int((f == c).any(1).sum()) for c in stars)
    for mode in ("fan", "centroid"):
        e = assert_twin_equals_restatement(v, rest, mode=mode)
        lens = sorted(np.diff(e["loop_start"]).tolist())
        assert e["report"]["loops"] == e["report"]["filled"] == len(stars) and lens == valence
        vv, ff, _ = emu.fill_holes(v, rest, mode=mode)
        rep = topology(vv, ff)
        assert rep["boundary"] == 0 and rep["nonmanifold"] == 0 and rep["euler"] == 2
        assert rep["vref"] == whole["vref"] - len(stars) + (len(stars) if mode == "centroid" else 0)


def test_error_paths_of_the_twin():
    v, f = tref.cube()
    bad = f.copy()
    bad[0, 0] = 8
    for fn in (emu.plan, ref.plan):
        with pytest.raises(ValueError) as err:
            fn(v, bad)
        assert err.value.code == -2
    for kw in ({"max_loop": 2}, {"mode": 2}):
        with pytest.raises(emu.EmuError) as err:
            emu.plan(v, f, **kw)
        assert err.value.code == -1
    with pytest.raises(emu.EmuError):
        emu.plan(None, f, mode="centroid", n_verts=8)


def test_surface_exists_without_a_gpu():
    from r3g import meshfill
    from r3g.mesh import Mesh
    repair = ref.trimesh_stand_in().repair
    for fn in ("boundary_loops", "fill_holes"):
        assert callable(getattr(meshfill, fn))
    assert meshfill.REPORT_FIELDS == emu.REPORT_FIELDS and callable(repair.fill_holes)
    assert Mesh().fill_holes() is False and repair.fill_holes(Mesh()) is False
    v, f = tref.cube()
    with pytest.raises(ValueError):
        Mesh(v, f[:-2], vertex_colors=np.zeros((8, 4), np.uint8)).fill_holes(mode="centroid")


def test_standalone_program_runs_the_core_header():
    """tests/emu/meshfill_selftest.cpp: its own main over the twin, built and run as a plain program (no sanitizer here)"""
    exe = emu_build.program("meshfill", ["meshfill_selftest.cpp"] + emu_build.TWINS["meshfill"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "meshfill selftest ok" in out.stdout
