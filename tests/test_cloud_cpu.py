"""Point-cloud neighbour search, host side: the host twin of csrc/cloud_core.h (tests/emu/cloud_emu.cpp)
-- its grid walk against its own brute force and against the numpy restatement of the definition (tests/cloud_ref.py), bit
for bit and index for index -- then scipy's cKDTree in float64, the automatic resolution, and the PLY layer of r3g/cloud.py.
No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-re-gen_amd"))

import cloud_ref as R  # noqa: E402
import emu_build  # noqa: E402
import emu_cloud as E  # noqa: E402

KS = (1, 2, 8, 30, 32)
RESOLUTIONS = (1, 3, 16, 0)          # 0: automatic


def _clouds():
    """name -> (points, queries, forced resolutions)"""
    big = R.uniform(4097, 10)
    lat = R.lattice(9)
    nonfin, _ = R.with_nonfinite(R.uniform(600, 14))
    out = {"uniform4097": (big, R.queries_for(big, 300), RESOLUTIONS),
           "lattice9": (lat, np.concatenate([lat, R.queries_for(lat, 90), R.far_queries(10)]), (8,) + RESOLUTIONS),
           "tripled": (R.tripled(300), R.queries_for(R.tripled(300), 150), RESOLUTIONS),
           "coplanar": (R.coplanar(500), R.queries_for(R.coplanar(500), 150), RESOLUTIONS),
           "repeated": (R.repeated(70), np.concatenate([R.repeated(3), R.uniform(40, 15)]), RESOLUTIONS),
           "far": (R.uniform(700, 16), R.far_queries(200), RESOLUTIONS),
           "nonfinite": (nonfin, R.queries_for(nonfin, 150), RESOLUTIONS)}
    for n in (63, 64, 65):
        p = R.uniform(n, 20 + n)
        out["uniform%d" % n] = (p, R.queries_for(p, 60), RESOLUTIONS)
    return out


CLOUDS = _clouds()
_REF = {}


def reference(name):
    """the numpy restatement at k = 32, computed once per cloud (the list for a smaller k is its prefix)"""
    if name not in _REF:
        p, q, _ = CLOUDS[name]
        _REF[name] = R.knn(q, p, 32)
    return _REF[name]


def same(d_a, i_a, d_b, i_b):
    return np.array_equal(R.bits(d_a), R.bits(d_b)) and np.array_equal(i_a, i_b)


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_grid_walk_equals_brute_force_and_numpy(name):
    p, q, resolutions = CLOUDS[name]
    rd, ri = reference(name)
    for k in KS:
        bd, bi, _ = E.brute(q, p, k)
        assert same(bd, bi, rd[:, :k], ri[:, :k]), (name, k, "twin brute force != numpy restatement")
        for res in resolutions:
            for rev in (False, True):
                gd, gi, info = E.grid(q, p, k, res, rev)
                assert same(gd, gi, bd, bi), (name, k, res, rev, info)


def test_every_lattice_point_sits_on_a_cell_border():
    """the lattice case is what it claims: at forced resolution 8 every coordinate is an exact multiple of the cell size"""
    lat = R.lattice(9)
    t = (lat - lat.min(0)) * np.float32(8.0)
    assert np.array_equal(t, np.round(t)) and lat.min() == 0.0 and lat.max() == 1.0
    _, _, info = E.grid(lat[:1], lat, 1, 8)
    assert info["resolution"] == 8


def test_duplicates_are_distinct_neighbours():
    p = R.tripled(200)
    q = p[:50]
    d2, ix, _ = E.grid(q, p, 3, 0)
    assert (d2 == 0).all()                                       # the three copies of the query point itself
    assert (np.diff(ix, axis=1) > 0).all()                      # distinct, ascending indices
    assert np.array_equal(p[ix[:, 0]], q) and np.array_equal(p[ix[:, 2]], q)


def test_nonfinite_targets_are_skipped_and_counted():
    p, n_bad = R.with_nonfinite(R.uniform(600, 14))
    q = R.queries_for(p, 100)
    d2, ix, info = E.grid(q, p, 8, 0)
    assert info["skipped"] == n_bad
    assert R.usable(p)[ix].all()                                 # original indices, none of a skipped row
    assert same(d2, ix, *R.knn(q, p, 8))


def test_k_beyond_the_usable_points_pads():
    p = R.uniform(5, 30)
    p[1, 0] = np.nan
    q = R.uniform(7, 31)
    for fn in (lambda: E.brute(q, p, 8)[:2], lambda: E.grid(q, p, 8, 3)[:2], lambda: E.grid(q, p, 8, 0, True)[:2]):
        d2, ix = fn()
        assert np.isinf(d2[:, 4:]).all() and (d2[:, 4:] > 0).all() and (ix[:, 4:] == -1).all()
        assert np.isfinite(d2[:, :4]).all() and (ix[:, :4] >= 0).all()
        assert same(d2, ix, *R.knn(q, p, 8))


def test_nonfinite_queries_get_the_quiet_nan():
    p = R.uniform(100, 32)
    q = R.uniform(6, 33)
    q[1, 2], q[4, 0] = np.inf, np.nan
    for k in (1, 8):
        d2, ix, _ = E.grid(q, p, k, 0)
        assert (R.bits(d2[[1, 4]]) == 0x7fc00000).all() and (ix[[1, 4]] == -1).all()
        assert same(d2, ix, *R.knn(q, p, k))


def test_refusals_of_the_twin():
    p = R.uniform(10, 34)
    for kw in (dict(k=0), dict(k=33), dict(resolution=257), dict(resolution=-1)):
        with pytest.raises(ValueError):
            E.grid(p, p, **kw)
    with pytest.raises(ValueError):
        E.grid(p, np.full((4, 3), np.nan, np.float32))


def test_automatic_resolution_rule():
    """min(256, max(1, floor(cbrt(n / P)))) in integers"""
    for per in (1, 2, 4, 8, 16):
        for n in (1, 3, per, 8 * per - 1, 8 * per, 27 * per, 1000 * per + 1, 4097, 10 ** 6, 256 ** 3 * per - 1, 256 ** 3 * per, 2 ** 31 - 1):
            want = 1
            while want < 256 and (want + 1) ** 3 * per <= n:
                want += 1
            assert E.auto_resolution(n, per) == want, (n, per)
    assert E.auto_resolution(4097, 4) == 10


def test_against_ckdtree_in_float64():
    """sqrt(d2) within rtol 1e-6 of scipy's float64 distances: the five float32 roundings of the definition bound the
    relative error of d2 by about 5 * 2^-24 = 3e-7, half of that after the root"""
    from scipy.spatial import cKDTree
    p = R.uniform(4097, 10)
    q = R.queries_for(p, 400, seed=40)
    d2, ix, _ = E.grid(q, p, 8, 0)
    dist, _ = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), k=8)
    got = np.sqrt(d2.astype(np.float64))
    nz = dist > 0
    assert np.allclose(got[nz], dist[nz], rtol=1e-6, atol=0.0)
    assert (got[~nz] == 0).all()


def test_selftest_program_under_sanitizers():
    """the twin with its own main(), built as a stand-alone program with -fsanitize=address,undefined (runtimes linked
    statically), on the lattice case; never loaded into Python"""
    if not emu_build.sanitizers_link():
        pytest.skip("no sanitizer runtime for g++ on this machine")
    exe = E.selftest_binary(sanitize=True)      # (a compile error of the twin's program is a failure, not a skip)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


# ---- the PLY layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", (True, False))
@pytest.mark.parametrize("colours", (True, False))
def test_ply_round_trip(tmp_path, binary, colours):
    from r3g import cloud
    v = R.uniform(257, 50)
    c = np.random.default_rng(51).integers(0, 256, (257, 3)).astype(np.uint8) if colours else None
    path = str(tmp_path / "c.ply")
    cloud.save_ply(path, v, c, binary=binary)
    pc = cloud.load_ply(path)
    assert isinstance(pc, cloud.PointCloud) and pc.vertices.dtype == np.float64
    assert np.array_equal(pc.vertices.astype(np.float32), v)
    assert (pc.colors is None) if c is None else np.array_equal(pc.colors, c)


def test_pointcloud_export_and_trimesh_stand_in(tmp_path):
    from meshfill_ref import trimesh_stand_in
    tm = trimesh_stand_in()
    v = R.uniform(33, 52)
    c = np.random.default_rng(53).integers(0, 256, (33, 4)).astype(np.uint8)          # RGBA in: RGB is kept
    path = str(tmp_path / "pred.ply")
    tm.PointCloud(v, colors=c).export(path)
    raw = open(path, "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\n")
    back = tm.load(path)
    assert isinstance(back, tm.PointCloud)
    assert np.array_equal(back.vertices.astype(np.float32), v) and np.array_equal(back.colors, c[:, :3])


def test_ply_reader_ignores_other_properties_and_faces(tmp_path):
    from r3g import cloud
    text = ("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
            "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
            "0 0 0 0.5 1 2 3 255\n1 0.25 0 0.5 4 5 6 255\n0 1 -2.5 0.5 7 8 9 255\n3 0 1 2\n")
    path = str(tmp_path / "m.ply")
    open(path, "w").write(text)
    pc = cloud.load_ply(path)
    assert np.array_equal(pc.vertices, [[0, 0, 0], [1, 0.25, 0], [0, 1, -2.5]])
    assert np.array_equal(pc.colors, [[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    # the same content, binary, with a double-precision vertex and the face element in front
    import struct
    head = ("ply\nformat binary_little_endian 1.0\nelement face 1\nproperty list uchar int vertex_indices\nelement vertex 2\n"
            "property double x\nproperty double y\nproperty double z\nproperty short q\nend_header\n").encode()
    body = struct.pack("<B3i", 3, 0, 1, 1) + struct.pack("<3dh", 1.5, 2.5, -3.5, 7) + struct.pack("<3dh", 0.1, 0.2, 0.3, -1)
    pc = cloud.load_ply(head + body)
    assert np.array_equal(pc.vertices, [[1.5, 2.5, -3.5], [0.1, 0.2, 0.3]]) and pc.colors is None
    with pytest.raises(ValueError):
        cloud.load_ply(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n")
