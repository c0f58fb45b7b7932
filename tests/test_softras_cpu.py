"""The soft silhouette's host twin (tests/emu/softras_emu.cpp: the text of csrc/softras_core.h) against the float64 restatement
(tests/softras_ref.py).  No GPU: the device equals the twin bit for bit (tests/test_softras_gpu.py), so the errors measured here
are the device's.

Which scenes may be compared.  The integer output `face` can only be demanded equal where no decision of the definition lies
within float32's reach of its threshold.  The restatement reports a scene's margins; the slack a margin has to exceed is
    bary, depth, key: 1e-5.  A barycentric is a quotient of two edge functions, each a difference of two products of coordinate
        differences: its error is at most about 8 eps M^2 / |area| (M = the largest |x|, |y| that occurs, eps = 2^-24), 7e-7 for
        the random scenes here (M = 35, |area| above 1) -- 1e-5 leaves an order of magnitude.  pz and the key gap are sums of three
        such quotients times z <= 4.
    blur: 1e-4.  d2 = dx^2 + dy^2 with dx = px - (xa + t ex): |error of dx| <= 6 eps M, so |error of d2| <= 17 eps M d; at the
        blur threshold d = sqrt(blur_radius) <= 5, giving 1.8e-4 at worst and 4e-5 for the default radius.
    edge (gradients only): 2e-4, the same bound for the difference of two such d2 (the winning edge decides the gradient's branch).
A value that is exactly 0 in float64 is a tie of the INPUT, not a margin: the scenes that have such ties on purpose (on_edge,
blur_tie, coincident) use coordinates for which float32 computes the same numerators exactly.

Seeds.  Tried for each random family: 0 .. 11 (the shared lattice: 0 .. 39).  Qualified for `face`: rand40 {0, 3, 6}, small and
small_sharp all twelve, shared {0, 3, 6, 7, 8, 10}.  Qualified for gradients too: small {4, 9, 10, 11}, small_sharp {2, 4, 9, 10,
11}, shared {39}.  No pixel is excluded from any comparison."""
import math
import subprocess

import numpy as np
import pytest
import torch

import emu_build
import emu_softras as E
import softras_ref as R

EPS = 2.0 ** -24
FACE_SLACK = {"bary": 1e-5, "depth": 1e-5, "key": 1e-5, "blur": 1e-4}
GRAD_SLACK = dict(FACE_SLACK, edge=2e-4)
SIGMOID_ERR_BOUND = 1.0e-7        # measured 8.9e-8 (test_sigmoid_error), rounded up
GRAD_REL_MEASURED = 5.0e-6        # the largest relative gradient error measured over grad_scenes() (4.98e-6, small_sharp_2; the test prints each)


def grad_rel_bound(K):
    """four times the measured error (the margin covers scenes not in the set), and the sigmoid's error in each of the K factors"""
    return 4 * GRAD_REL_MEASURED + K * (SIGMOID_ERR_BOUND + 2 * EPS)


def small(seed, **kw):
    return R.random_scene(seed, size=(17, 19), F=12, K=4, **kw)


def face_scenes():
    s = R.named_scenes()
    out = {n: s[n] for n in ("full_cover", "outside", "behind", "degenerate", "coincident", "on_edge", "on_edge_blur0", "blur_tie", "wide_blur", "sharp")}
    for seed in (0, 3, 6):
        out["rand40_%d" % seed] = R.random_scene(seed)
    out["rand40_blur0_3"] = R.random_scene(3, blur=0.0)
    for seed in (0, 1, 2):
        out["small_%d" % seed] = small(seed)
    for seed in (0, 3):
        out["shared_%d" % seed] = R.shared_scene(seed, size=(17, 19), n=4, K=4)
    return out


def grad_scenes():
    out = {"full_cover": R.named_scenes()["full_cover"], "shared_39": R.shared_scene(39, size=(17, 19), n=4, K=4)}
    for seed in (4, 9, 10):
        out["small_%d" % seed] = small(seed)
    for seed in (2, 4):
        out["small_sharp_%d" % seed] = small(seed, sigma=0.05, blur=4.0)
    return out


_CACHE = {}


def both(name, sc):
    """(restatement with margins, twin forward) of a scene, computed once"""
    if name not in _CACHE:
        ref = R.render(torch.tensor(sc["pos"].astype(np.float64)), sc["tri"], sc["size"], sc["K"], sc["sigma"], sc["blur"], want_margins=True)
        _CACHE[name] = (ref, E.forward(sc["pos"], sc["tri"], sc["size"], sc["K"], sc["sigma"], sc["blur"]))
    return _CACHE[name]


def test_sigmoid_error():
    """sr_sigmoid against float64 over a dense sweep of [-100, 100] (past the clamp at +-80 on both sides)"""
    x = np.linspace(-100.0, 100.0, 4000001).astype(np.float32)
    s = E.sigmoid(x)
    ref = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    err = np.abs(s - ref).max()
    print("sr_sigmoid: max |error| %.3e" % err)
    assert err <= SIGMOID_ERR_BOUND
    assert np.all(s > 0) and np.all(s <= 1) and np.all(np.diff(s[::1000]) >= 0)
    assert E.sigmoid(np.array([np.inf, -np.inf, 0.0], np.float32)).tolist() == [1.0, E.sigmoid(np.array([-80.0], np.float32))[0], 0.5]


@pytest.mark.parametrize("name", sorted(face_scenes()))
def test_face_lists_equal(name):
    sc = face_scenes()[name]
    ref, emu = both(name, sc)
    short = {k: v for k, v in ref["margins"].items() if k in FACE_SLACK and not v > FACE_SLACK[k]}
    assert not short, "the scene does not qualify: margins %s" % short
    assert np.array_equal(emu["face"], ref["face"].numpy())


def tolerances(sc, ref):
    """per-entry bounds of |dist|, |zbuf| and the per-pixel bound of |alpha|, from the formats' precision (module docstring)"""
    drawn = R.drawn_faces(sc["pos"], sc["tri"])
    v = sc["pos"].astype(np.float64)[sc["tri"][drawn].reshape(-1)].reshape(-1, 3, 3)
    H, W = sc["size"]
    M = max(np.abs(v[:, :, :2]).max(), H, W)
    area = np.abs(R._edge(v[:, 2, 0], v[:, 2, 1], v[:, 0, 0], v[:, 0, 1], v[:, 1, 0], v[:, 1, 1])).min()
    d = ref["dist"].numpy()
    dist_tol = 17 * EPS * M * np.sqrt(np.abs(d)) + 4 * EPS * np.abs(d)
    z_tol = (3 * 8 * EPS * M * M / area + 8 * EPS) * np.abs(v[:, :, 2]).max()
    valid = ref["face"].numpy() >= 0
    # a factor (1 - s_k) carries the sigmoid's error, one rounding of its own and one of the running product, and the slope of the
    # sigmoid (at most 1 / (4 sigma)) times the distance's error; factors lie in [0, 1], so the errors add
    sigma = float(np.float32(sc["sigma"]))
    alpha_tol = np.where(valid, SIGMOID_ERR_BOUND + 2 * EPS + (dist_tol + 2 * EPS * np.abs(d)) / (4 * sigma), 0.0).sum(-1) + EPS
    return dist_tol, z_tol, alpha_tol


@pytest.mark.parametrize("name", sorted(face_scenes()))
def test_float_outputs(name):
    sc = face_scenes()[name]
    ref, emu = both(name, sc)
    dist_tol, z_tol, alpha_tol = tolerances(sc, ref)
    assert np.array_equal(emu["face"], ref["face"].numpy())
    ed, ez, ea = (np.abs(emu[k] - ref[k].numpy()) for k in ("dist", "zbuf", "alpha"))
    print("%s: dist %.2e (bound %.2e), zbuf %.2e (%.2e), alpha %.2e (%.2e)" % (name, ed.max(), dist_tol.max(), ez.max(), z_tol, ea.max(), alpha_tol.max()))
    assert np.all(ed <= dist_tol) and np.all(ez <= z_tol) and np.all(ea <= alpha_tol)


def _grad_alpha(sc):
    return np.random.default_rng(5).uniform(-1, 1, sc["size"]).astype(np.float32)


@pytest.mark.parametrize("name", sorted(grad_scenes()))
def test_gradient(name):
    sc = grad_scenes()[name]
    ref, emu = both(name, sc)
    short = {k: v for k, v in ref["margins"].items() if k in GRAD_SLACK and not v > GRAD_SLACK[k]}
    assert not short, "the scene does not qualify: margins %s" % short
    ga = _grad_alpha(sc)
    g64 = R.gradient(sc["pos"], sc["tri"], sc["size"], sc["K"], sc["sigma"], sc["blur"], ga)
    g32 = E.backward(sc["pos"], sc["tri"], sc["size"], sc["K"], sc["sigma"], sc["blur"], emu["face"], emu["dist"], ga)["grad_pos"]
    scale = np.abs(g64).max()
    rel = np.abs(g32 - g64).max() / scale if scale else 0.0
    print("%s: max |grad| %.3e, relative error %.3e (bound %.1e)" % (name, scale, rel, grad_rel_bound(sc["K"])))
    assert np.all(g32[:, 2] == 0) and np.all(g64[:, 2] == 0)
    assert scale > 0 and rel <= grad_rel_bound(sc["K"])


def test_restatement_gradient_against_central_differences():
    """the yardstick itself: autograd of the restatement against its own central differences in float64"""
    sc = small(4)
    ga = _grad_alpha(sc).astype(np.float64)
    g = R.gradient(sc["pos"], sc["tri"], sc["size"], sc["K"], sc["sigma"], sc["blur"], ga)

    def loss(p):
        return float((R.render(torch.tensor(p), sc["tri"], sc["size"], sc["K"], sc["sigma"], sc["blur"])["alpha"].numpy() * ga).sum())
    p0 = sc["pos"].astype(np.float64)
    h, worst = 1e-6, 0.0
    for v in range(0, len(p0), 5):
        for c in range(3):
            a, b = p0.copy(), p0.copy()
            a[v, c] += h
            b[v, c] -= h
            worst = max(worst, abs((loss(a) - loss(b)) / (2 * h) - g[v, c]))
    assert worst <= 1e-6 * max(1.0, np.abs(g).max()), worst


def test_more_layers_than_K():
    """40 stacked quads under K = 20: every covered pixel keeps the 20 nearest, in ascending depth, faces in (pz, face) order"""
    sc = R.named_scenes()["stacked"]
    emu = E.forward(sc["pos"], sc["tri"], sc["size"], sc["K"], sc["sigma"], sc["blur"])
    full = emu["face"][8, 9]
    assert np.all(full >= 40) and len(set(full.tolist())) == 20      # the nearest quads are the last ones
    z = np.where(emu["face"] >= 0, emu["zbuf"], np.float32(1e30))
    assert np.all(np.diff(z, axis=-1) >= 0)


MUTANT_SCENES = {"blur_less_equal": "blur_tie", "no_face_key": "coincident", "unclipped_depth": "wide_blur", "narrow_box": "wide_blur",
                 "ignore_endpoint": "wide_blur", "divide_out": "saturate"}


@pytest.mark.parametrize("mutant", sorted(E.MUTANTS))
def test_mutants_are_caught(mutant):
    sc = R.named_scenes()[MUTANT_SCENES[mutant]]
    args = (sc["pos"], sc["tri"], sc["size"], sc["K"], sc["sigma"], sc["blur"])
    good, bad = E.forward(*args), E.forward(*args, mutant=mutant)
    ga = _grad_alpha(sc)
    g_good = E.backward(*args, good["face"], good["dist"], ga)
    g_bad = E.backward(*args, good["face"], good["dist"], ga, mutant=mutant)
    if mutant in ("ignore_endpoint", "divide_out"):
        assert all(np.array_equal(good[k], bad[k]) for k in ("face", "dist", "zbuf", "alpha"))      # a gradient-only departure
        assert np.all(np.isfinite(g_good["grad_pos"]))
        assert not np.array_equal(g_good["grad_pos"], g_bad["grad_pos"], equal_nan=True)
    elif mutant == "unclipped_depth":
        assert not np.array_equal(good["zbuf"], bad["zbuf"])
    else:
        assert not np.array_equal(good["face"], bad["face"])


def test_corner_csr():
    tri = np.array([[0, 1, 2], [2, 1, 3], [3, 9, -1]], np.int32)
    start, ids = E.corner_csr(tri, 4)
    assert start.tolist() == [0, 1, 3, 5, 7] and ids.tolist() == [0, 1, 4, 2, 3, 5, 6]


def test_selftest_program_under_sanitizers():
    if not emu_build.sanitizers_link():
        pytest.skip("no sanitizer runtime for g++ on this machine")
    out = subprocess.run([E.selftest_binary(sanitize=True)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
