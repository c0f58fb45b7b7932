"""Mesh topology without a GPU: the host twin of csrc/meshtopo_core.h (tests/emu_meshtopo.py) against
the numpy / scipy restatement (tests/meshtopo_ref.py) on fixtures whose answers are known, and the quantised volume against the
restatement's float64 volume within the bound the section derives."""
import os
import subprocess

import numpy as np
import pytest

import emu_build
import emu_meshtopo as emu
import meshtopo_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPO_FIELDS = ("usable", "skipped", "vref", "edges", "boundary", "clash", "nonmanifold", "bodies", "unorientable", "euler", "nonfinite")

FIXTURES = {
    "tetrahedron": ref.tetrahedron, "cube": ref.cube, "cube_reversed_0": lambda: ref.cube_reversed(0),
    "cube_reversed_5": lambda: ref.cube_reversed(5), "cube_minus_one": lambda: (ref.cube()[0], ref.cube()[1][:-1]),
    "shared_edge": ref.shared_edge, "moebius": ref.moebius, "torus": ref.torus, "two_balls": ref.two_balls,
    "duplicated_face": lambda: (ref.cube()[0], np.concatenate([ref.cube()[1], ref.cube()[1][3:4]])),
    "degenerate_face": lambda: (ref.cube()[0], np.concatenate([ref.cube()[1], np.array([[2, 2, 5]], np.int32)])),
    "cube_and_moebius": ref.cube_and_moebius, "moebius_and_cube": lambda: ref.cube_and_moebius(cube_first=False),
    "double_face": ref.double_face, "strip": lambda: ref.strip(257), "golden_A": lambda: ref.golden_mesh("A"), "golden_B": lambda: ref.golden_mesh("B"),
}
_CACHE = {}


def states(name):
    """(verts, faces, twin state, restatement state) of a fixture, computed once and read-only"""
    if name not in _CACHE:
        v, f = FIXTURES[name]()
        _CACHE[name] = (v, f, emu.build(v, f), ref.build(v, f))
        for a in (v, f):
            a.setflags(write=False)
    return _CACHE[name]


def adjacency_from_mates(mate):
    """r3g.meshtopo.face_adjacency's rule on the twin's mates: one row per deg = 2 edge, pairs ascending, rows sorted"""
    m = mate.reshape(-1).astype(np.int64)
    h = np.flatnonzero(m > np.arange(len(m)))
    pairs = np.sort(np.stack([h // 3, m[h] // 3], 1), axis=1)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))].reshape(-1, 2)


def volume_bound(rep, faces):
    """|six_volume_q / 2^s - the exact sum| <= faces * 2^-(s + 1): one llrint per face"""
    return faces * 2.0 ** -(rep["vol_scale"] + 1)


def assert_bodies_decided(name):
    """every body's |six-volume| exceeds its quantisation bound, so the twin's integer sign is the restatement's float sign"""
    _, _, e, r = states(name)
    vols, n = ref.body_volumes(r)
    for b, x in vols.items():
        assert abs(x) > volume_bound(e["report"], n[b]), (name, b, x)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_twin_equals_the_restatement(name):
    v, f, e, r = states(name)
    for k in ("mate", "body", "flip"):
        assert np.array_equal(e[k], r[k]), k
    for k in TOPO_FIELDS:
        assert e["report"][k] == r["report"][k], k
    assert e["report"]["euler"] == e["report"]["vref"] - e["report"]["edges"] + e["report"]["usable"]
    broken = np.flatnonzero(((e["mate"] == -1) | (e["mate"] == -2)).any(1))
    assert np.array_equal(broken, r["broken"])
    assert np.array_equal(adjacency_from_mates(e["mate"]), r["adjacency"])
    # the same state whatever order the faces are walked in (what the device's atomics decide is the order, nothing else)
    e2 = emu.build(v, f, reverse=True)
    assert e2["report"] == e["report"] and all(np.array_equal(e2[k], e[k]) for k in ("mate", "body", "flip"))
    # topology needs no vertices
    e3 = emu.build(None, f, n_verts=len(v))
    assert all(np.array_equal(e3[k], e[k]) for k in ("mate", "body", "flip")) and not e3["report"]["has_verts"]
    assert e3["report"]["six_volume_q"] == 0 and e3["report"]["two_area_q"] == 0


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_quantised_volume_and_area_within_the_bound(name):
    _, f, e, r = states(name)
    rep = e["report"]
    assert (rep["vol_scale"], rep["area_scale"]) == (r["s_vol"], r["s_area"])
    counted = rep["usable"] - rep["nonfinite"]
    assert abs(rep["six_volume_q"] / 2.0 ** rep["vol_scale"] - r["report"]["six_volume"]) <= volume_bound(rep, counted)
    assert abs(rep["two_area_q"] / 2.0 ** rep["area_scale"] - r["report"]["two_area"]) <= counted * 2.0 ** -(rep["area_scale"] + 1)
    # 2^29 faces of the largest magnitude the scale admits stay inside int64
    assert 2 ** 29 * (2 ** 33 + 1) < 2 ** 63


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "cube_reversed_0", "cube_reversed_5", "torus", "two_balls", "golden_A"])
@pytest.mark.parametrize("outward", [0, 1, 2])
def test_orient_equals_the_restatement(name, outward):
    v, f, _, _ = states(name)
    assert_bodies_decided(name)
    eo = emu.orient(v, f, outward)
    rf, rfaces, rbodies = ref.orient(v, f, outward)
    assert np.array_equal(eo["faces"], rf)
    assert (eo["faces_reversed"], eo["bodies_reversed"]) == (rfaces, rbodies)
    again = emu.orient(v, eo["faces"], outward)
    assert again["faces_reversed"] == 0 and again["bodies_reversed"] == 0 and np.array_equal(again["faces"], eo["faces"])
    assert eo["report"]["clash"] == 0
    # the state left behind describes the rewritten faces
    fresh = emu.build(v, eo["faces"])
    assert fresh["report"] == eo["report"] and all(np.array_equal(fresh[k], eo[k]) for k in ("mate", "body", "flip"))


def test_tetrahedron_and_cube_literals():
    for name in ("tetrahedron", "cube"):
        rep = states(name)[2]["report"]
        want = {"tetrahedron": (4, 6, 4), "cube": (8, 18, 12)}[name]
        assert (rep["vref"], rep["edges"], rep["usable"]) == want and rep["euler"] == 2
        assert rep["boundary"] == rep["nonmanifold"] == rep["clash"] == 0 and rep["bodies"] == 1 and rep["unorientable"] == 0
    rep = states("cube")[2]["report"]
    assert abs(rep["six_volume_q"] / 2.0 ** rep["vol_scale"] / 6 - 1.0) <= volume_bound(rep, 12) / 6
    assert rep["two_area_q"] / 2.0 ** rep["area_scale"] / 2 == 6.0
    e = states("cube")[2]
    assert (e["mate"] >= 0).all() and np.array_equal(e["mate"].reshape(-1)[e["mate"].reshape(-1)], np.arange(36))


@pytest.mark.parametrize("k", [0, 5])
def test_cube_with_one_face_reversed(k):
    v, f, e, _ = states("cube_reversed_%d" % k)
    assert e["report"]["clash"] == 3 and e["report"]["boundary"] == 0 and e["report"]["unorientable"] == 0
    wound = emu.orient(v, f, 0)
    changed = np.flatnonzero((wound["faces"] != f).any(1))
    assert np.array_equal(changed, [k] if k else np.arange(1, 12))       # face 0 keeps its winding: the others follow it
    assert np.array_equal(wound["faces"][changed], f[changed][:, ::-1])
    for outward in (1, 2):
        fixed = emu.orient(v, f, outward)
        assert np.array_equal(fixed["faces"], ref.cube()[1])
        assert fixed["faces_reversed"] == 1 and fixed["bodies_reversed"] == (1 if k == 0 else 0)
        assert fixed["report"]["six_volume_q"] > 0


def test_cube_minus_one_triangle():
    _, f, e, _ = states("cube_minus_one")
    rep = e["report"]
    assert rep["boundary"] == 3 and rep["nonmanifold"] == 0 and rep["euler"] == 1
    broken = np.flatnonzero((e["mate"] == -1).any(1))
    removed = set(ref.cube()[1][-1].tolist())
    neighbours = [i for i in range(11) if len(removed & set(f[i].tolist())) == 2]
    assert len(broken) == 3 and broken.tolist() == neighbours
    assert not (rep["usable"] > 0 and rep["boundary"] == 0 and rep["nonmanifold"] == 0)        # not watertight


def test_shared_edge_is_non_manifold():
    _, f, e, _ = states("shared_edge")
    assert e["report"]["nonmanifold"] == 1 and e["report"]["boundary"] == 0 and e["report"]["bodies"] == 2
    on_edge = (e["mate"] == -2)
    assert on_edge.sum() == 4                                            # the one edge has degree 4
    for h in np.flatnonzero(on_edge.reshape(-1)):
        assert {int(f[h // 3, h % 3]), int(f[h // 3, (h % 3 + 1) % 3])} == {0, 1}


def test_moebius_strip_is_one_unorientable_body():
    v, f, e, _ = states("moebius")
    assert e["report"]["bodies"] == 1 and e["report"]["unorientable"] == 1 and not e["flip"].any()
    for outward in (0, 1, 2):
        o = emu.orient(v, f, outward)
        assert np.array_equal(o["faces"], f) and o["faces_reversed"] == 0 and o["bodies_reversed"] == 0


@pytest.mark.parametrize("name", ["cube_and_moebius", "moebius_and_cube"])
@pytest.mark.parametrize("inward", [False, True])
def test_an_unorientable_body_weighs_on_no_reversal(name, inward):
    """one orientable body (the cube) beside one unorientable body whose det-sum is large and negative: the strip is never
    touched and never counted, so outward 1 and 2 both leave the cube outward, and a second call reverses nothing"""
    v, f, e, r = states(name)
    assert e["report"]["bodies"] == 2 and e["report"]["unorientable"] == 1
    assert r["report"]["six_volume"] < -6.0                              # the mesh's total is negative although the cube is outward
    cube_faces = np.flatnonzero(r["orientable"][np.maximum(e["body"], 0)])
    assert len(cube_faces) == 12
    assert_bodies_decided(name)
    start = f.copy()
    if inward:
        start[cube_faces] = start[cube_faces][:, ::-1]
    for outward in (1, 2):
        first = emu.orient(v, start, outward)
        assert np.array_equal(first["faces"], f)                         # the cube ends outward, the strip as it was
        assert (first["faces_reversed"], first["bodies_reversed"]) == ((12, 1) if inward else (0, 0))
        rf, rfaces, rbodies = ref.orient(v, start, outward)
        assert np.array_equal(rf, f) and (rfaces, rbodies) == (first["faces_reversed"], first["bodies_reversed"])
        for _ in range(2):
            again = emu.orient(v, first["faces"], outward)
            assert again["faces_reversed"] == 0 and again["bodies_reversed"] == 0 and np.array_equal(again["faces"], f)


def test_two_faces_that_share_three_edges():
    _, _, e, r = states("double_face")
    assert e["report"]["edges"] == 3 and e["report"]["boundary"] == 0 and e["report"]["clash"] == 0 and e["report"]["euler"] == 2
    assert r["adjacency"].tolist() == [[0, 1]] * 3 and adjacency_from_mates(e["mate"]).tolist() == [[0, 1]] * 3


def test_torus_and_balls():
    assert states("torus")[2]["report"]["euler"] == 0
    v, f, e, r = states("two_balls")
    assert e["report"]["bodies"] == 2 and e["report"]["euler"] == 4 and e["report"]["clash"] == 0
    assert_bodies_decided("two_balls")
    multi = emu.orient(v, f, 1)
    assert multi["bodies_reversed"] == 1 and multi["faces_reversed"] == 32
    assert np.array_equal(np.flatnonzero((multi["faces"] != f).any(1)), np.arange(32, 64))
    assert r["report"]["six_volume"] > 0                                 # the outward ball is the larger one: the total says "fine"
    assert emu.orient(v, f, 2)["faces_reversed"] == 0
    small = ref.two_balls(inner_radius=2.0)                              # now the inward ball dominates: the total is negative
    whole = emu.orient(*small, 2)
    assert whole["bodies_reversed"] == 2 and whole["faces_reversed"] == 64
    assert np.array_equal(whole["faces"], small[1][:, ::-1])


def test_duplicated_and_degenerate_faces():
    _, f, e, _ = states("duplicated_face")
    rep = e["report"]
    assert rep["nonmanifold"] == 3 and rep["skipped"] == 0 and (e["mate"][[3, 12]] == -2).all()
    _, f, e, _ = states("degenerate_face")
    rep = e["report"]
    assert rep["skipped"] == 1 and rep["usable"] == 12 and (e["mate"][12] == -3).all() and e["body"][12] == -1
    cube = states("cube")[2]
    assert np.array_equal(e["mate"][:12], cube["mate"]) and rep["euler"] == 2


def test_bad_inputs():
    v, f = ref.cube()
    for bad in (8, -1):
        g = f.copy()
        g[7, 1] = bad
        with pytest.raises(emu.EmuError) as err:
            emu.build(v, g)
        assert err.value.code == -2
        with pytest.raises(ref.BadIndex):
            ref.build(v, g)
        with pytest.raises(emu.EmuError):
            emu.orient(v, g, 0)
    with pytest.raises(emu.EmuError) as err:
        emu.build(v, np.zeros((0, 3), np.int32))
    assert err.value.code == -1
    with pytest.raises(emu.EmuError):
        emu.orient(None, f, 1, n_verts=8)                                # a volume needs vertices
    w = v.copy()
    w[3, 1] = np.nan
    e, clean = emu.build(w, f), emu.build(v, f)
    assert e["report"]["nonfinite"] == int((f == 3).any(1).sum()) and r_topology(e) == r_topology(clean)
    assert np.array_equal(e["mate"], clean["mate"])
    r = ref.build(w, f)
    assert r["report"]["nonfinite"] == e["report"]["nonfinite"]
    assert abs(e["report"]["six_volume_q"] / 2.0 ** e["report"]["vol_scale"] - r["report"]["six_volume"]) <= volume_bound(e["report"], 12 - e["report"]["nonfinite"])


def r_topology(state):
    return {k: state["report"][k] for k in TOPO_FIELDS if k != "nonfinite"}


def test_golden_sphere():
    v, f, e, r = states("golden_A")
    rep = e["report"]
    assert (rep["vref"], rep["usable"], rep["edges"], rep["euler"]) == (7470, 14936, 22404, 2)
    assert rep["boundary"] == rep["nonmanifold"] == rep["clash"] == 0 and rep["bodies"] == 1 and rep["unorientable"] == 0
    assert_bodies_decided("golden_A")
    assert rep["six_volume_q"] < 0                                       # skimage's face order winds inward
    for outward in (1, 2):
        o = emu.orient(v, f, outward)
        assert o["faces_reversed"] == 14936 and np.array_equal(o["faces"], f[:, ::-1])
        assert emu.orient(v, np.ascontiguousarray(f[:, ::-1]), outward)["faces_reversed"] == 0      # hy3dgen's order
    radius = np.sqrt(399.5)
    assert abs(-rep["six_volume_q"] / 2.0 ** rep["vol_scale"] / 6 / (4 / 3 * np.pi * radius ** 3) - 1) < 0.01


def test_long_chain_keeps_its_parity():
    v, f, e, _ = states("strip")
    assert e["report"]["bodies"] == 1 and e["report"]["clash"] == 256 and e["report"]["unorientable"] == 0
    assert np.array_equal(e["flip"], np.arange(257) % 2)
    assert e["rounds"] > 0


def test_api_surface_is_declared():
    from r3g import ffi
    hdr = open(os.path.join(ROOT, "include", "r3g.h")).read()
    for name in ("r3g_meshtopo_build", "r3g_meshtopo_report", "r3g_meshtopo_mates", "r3g_meshtopo_bodies", "r3g_meshtopo_orient"):
        assert name in ffi.SYMBOLS and name + "(" in hdr
    for counter in ('"meshtopo_builds"', '"meshtopo_rounds"'):
        assert counter in hdr and counter in ffi.counter.__doc__
    import r3g.meshtopo as meshtopo
    for fn in ("build", "mates", "bodies", "report", "face_adjacency", "broken_faces", "fix_winding", "fix_normals"):
        assert callable(getattr(meshtopo, fn))
    from r3g.mesh import Mesh
    empty = Mesh()
    assert not empty.is_watertight and not empty.is_winding_consistent and not empty.is_volume
    assert empty.euler_number == 0 and empty.body_count == 0 and empty.volume == 0.0 and empty.area == 0.0
    assert empty.face_adjacency.shape == (0, 2) and empty.fix_normals() is empty
    m = Mesh(*ref.cube())
    assert np.array_equal(m.invert().faces, ref.cube()[1][:, ::-1])


def test_standalone_program_runs_the_core_header():
    """tests/emu/meshtopo_selftest.cpp: its own main over the twin (cube and Moebius strip), built and run as a plain program"""
    exe = emu_build.program("meshtopo", ["meshtopo_selftest.cpp"] + emu_build.TWINS["meshtopo"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "meshtopo selftest ok" in out.stdout
