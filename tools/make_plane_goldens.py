#!/usr/bin/env python3
"""Record the goldens of tests/test_plane_cpu.py and tests/test_plane_gpu.py from the reference's own plane fit and yaw search
(host only, run once by hand):

    python tools/make_plane_goldens.py REFERENCE_ROOT

REFERENCE_ROOT is a checkout of the reference project.  Its src/scene_reconstruction/source/pose_matching_planar.py cannot be
imported here (it needs pytorch3d, cv2 and the rest of its stage), so the file is parsed with `ast` at run time and only the
function nodes fit_plane_svd, fit_plane_ransac_refined and find_best_initial_yaw are compiled, into a namespace that holds
torch and logging; nothing of its text is copied.  find_best_initial_yaw calls two pytorch3d names, for which this tool
injects stand-ins OF ITS OWN: `chamfer_distance`, a brute-force float32 restatement of pytorch3d's default (per batch item the
mean over x of the squared distance to the nearest y, plus the same the other way; returns (loss, None)), and
`euler_angles_to_matrix` for convention "XYZ" (R_x R_y R_z of the three angles).  The recorded yaw losses are therefore the
reference's search over this tool's Chamfer, not pytorch3d's own kernels.

Writes tests/golden/plane_clouds.npz and tests/golden/plane_expect.json.  Per RANSAC cloud (n = 512, H = 32, threshold 0.05): the
triples (the reference's stream: one torch.randperm(n)[:3] per iteration after torch.manual_seed(seed)), the reference's mask as
row indices, its count, the centroid it returns and its fit_plane_svd normal of the whole cloud.  A cloud is regenerated with
another seed until, in float64 (tests/plane_ref.py), no |d - threshold| is at most 1e-5 times the cloud's extent and no
cross-product length lies within 10 % of 1e-6: then neither the counts nor the validity can depend on float32 rounding.  Both
are asserted.  Per yaw pair: the 18 losses and the arg-min, regenerated until the best loss is below the second best by more
than 1e-3 relative (asserted).
"""
import ast
import json
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_ref  # noqa: E402

N, H, THRESHOLD = 512, 32, 0.05
MARGIN = 1e-5
WANTED = ("fit_plane_svd", "fit_plane_ransac_refined", "find_best_initial_yaw")


def chamfer_distance(x, y, batch_reduction="mean"):
    """this tool's stand-in for pytorch3d.loss.chamfer_distance (see the module docstring)"""
    d2 = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(dim=-1)
    loss = d2.min(dim=2).values.mean(dim=1) + d2.min(dim=1).values.mean(dim=1)
    assert batch_reduction is None
    return loss, None


def euler_angles_to_matrix(angles, convention):
    """this tool's stand-in for pytorch3d.transforms.euler_angles_to_matrix, convention "XYZ" only"""
    assert convention == "XYZ"
    c, s, o, l = torch.cos(angles), torch.sin(angles), torch.zeros_like(angles[:, 0]), torch.ones_like(angles[:, 0])
    rx = torch.stack([l, o, o, o, c[:, 0], -s[:, 0], o, s[:, 0], c[:, 0]], dim=1).reshape(-1, 3, 3)
    ry = torch.stack([c[:, 1], o, s[:, 1], o, l, o, -s[:, 1], o, c[:, 1]], dim=1).reshape(-1, 3, 3)
    rz = torch.stack([c[:, 2], -s[:, 2], o, s[:, 2], c[:, 2], o, o, o, l], dim=1).reshape(-1, 3, 3)
    return rx @ ry @ rz


def load_reference(reference_root):
    path = os.path.join(reference_root, "src", "scene_reconstruction", "source", "pose_matching_planar.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in nodes) == sorted(WANTED)
    ns = {"torch": torch, "logging": logging, "os": os, "chamfer_distance": chamfer_distance, "euler_angles_to_matrix": euler_angles_to_matrix}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns


def ransac_clear(p, triples):
    """the two float64 conditions of the module docstring"""
    q = p.astype(np.float64)
    extent = float((q.max(axis=0) - q.min(axis=0)).max())
    p0, nr, valid = plane_ref.hypotheses(p, triples)
    for k, t in enumerate(triples):
        a, b, c = q[t[0]], q[t[1]], q[t[2]]
        ln = np.linalg.norm(np.cross(b - a, c - a))
        if 0.9e-6 <= ln <= 1.1e-6:
            return False
        if valid[k] and np.abs(plane_ref.distances(p, p0[k], nr[k]) - THRESHOLD).min() <= MARGIN * extent:
            return False
    return True


def reference_triples(seed):
    torch.manual_seed(seed)
    return np.stack([torch.randperm(N)[:3].numpy() for _ in range(H)]).astype(np.int32)


RANSAC_CLOUDS = {
    "floor": lambda seed: plane_ref.slab(seed, N, outliers=0.4),
    "tilted_floor": lambda seed: plane_ref.slab(seed, N, tilt_deg=5.0, outliers=0.2),
    "rough_floor": lambda seed: plane_ref.slab(seed, N, tilt_deg=-3.0, noise=0.03, outliers=0.3),
}


def yaw_pair(seed, index):
    """an L-shaped set of vertices and a noisy sample of it turned to candidate `index` of the 18"""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(-1.0, 1.0, 220), rng.uniform(0.0, 0.4, 220), rng.uniform(-0.2, 0.2, 220)], axis=1)
    b = np.stack([rng.uniform(0.6, 1.0, 120), rng.uniform(0.0, 0.8, 120), rng.uniform(-0.2, 0.9, 120)], axis=1)
    verts = np.concatenate([a, b])
    angle = np.linspace(0.0, 2 * 3.14159, 18)[index]
    pick = rng.permutation(len(verts))[:300]
    target = verts[pick] @ plane_ref.yaw_rotation(angle).T + rng.normal(0.0, 0.01, (300, 3)) + np.array([0.3, -0.2, 0.5])
    return verts.astype(np.float32), target.astype(np.float32)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference(sys.argv[1])
    arrays, expect = {}, {"n": N, "h": H, "threshold": THRESHOLD, "ransac": {}, "svd": {}, "yaw": {}}
    for name, make in RANSAC_CLOUDS.items():
        seed = None
        for seed in range(100, 200):
            p, triples = make(seed), reference_triples(seed)
            if ransac_clear(p, triples):
                break
        assert ransac_clear(p, triples), name
        torch.manual_seed(seed)
        normal, centroid, mask = ref["fit_plane_ransac_refined"](torch.from_numpy(p), iterations=H, threshold=THRESHOLD)
        svd_normal, _ = ref["fit_plane_svd"](torch.from_numpy(p))
        rows = torch.nonzero(mask).flatten().tolist()
        arrays[name] = p
        expect["ransac"][name] = {"seed": seed, "triples": triples.tolist(), "mask_rows": rows, "count": len(rows),
                                  "centroid": [float(v) for v in centroid.flatten()], "refined_normal": [float(v) for v in normal],
                                  "svd_normal": [float(v) for v in svd_normal]}
    # the mirror-symmetric slab of tests/plane_ref.py, the one input on which the reference's normal is claimed
    p = plane_ref.clouds()["mirror_slab"][0]
    svd_normal, svd_point = ref["fit_plane_svd"](torch.from_numpy(np.array(p)))
    arrays["mirror_slab"] = np.array(p)
    expect["svd"]["mirror_slab"] = {"svd_normal": [float(v) for v in svd_normal], "centroid": [float(v) for v in svd_point.flatten()]}
    for name, index in (("yaw_l_5", 5), ("yaw_l_13", 13)):
        losses = None
        for seed in range(300, 400):
            verts, target = yaw_pair(seed, index)
            captured = {}

            def spy(x, y, batch_reduction="mean", _c=captured):
                _c["loss"] = chamfer_distance(x, y, batch_reduction)[0]
                return _c["loss"], None
            ref["chamfer_distance"] = spy
            best_r = ref["find_best_initial_yaw"](torch.from_numpy(verts), torch.from_numpy(target), num_angles=18)
            losses = captured["loss"].double().numpy()
            order = np.sort(losses)
            if order[0] < order[1] * (1.0 - 1e-3):
                break
        order = np.sort(losses)
        assert order[0] < order[1] * (1.0 - 1e-3), name
        arrays[name + "_verts"], arrays[name + "_target"] = verts, target
        expect["yaw"][name] = {"seed": seed, "losses": [float(v) for v in losses], "argmin": int(np.argmin(losses)),
                               "rotation": [[float(v) for v in row] for row in best_r]}
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "plane_clouds.npz"), **arrays)
    with open(os.path.join(GOLDEN, "plane_expect.json"), "w") as f:
        json.dump({"torch": torch.__version__, **expect}, f, separators=(",", ":"))
    print("wrote", len(arrays), "arrays;", {k: v["count"] for k, v in expect["ransac"].items()}, {k: v["argmin"] for k, v in expect["yaw"].items()})


if __name__ == "__main__":
    main()
