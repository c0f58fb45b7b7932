"""The scene of the pose-fit tests and the float64 restatement of its two device paths (test-only): an L-shaped prism standing on a
tilted floor in front of a pinhole camera, its hard mask at 64 x 48, a cloud sampled from the faces the camera sees, and

    render64:            tests/softras_ref.py's brute-force silhouette behind r3g.softras.pinhole
    point_face_loss64:   brute-force point-to-triangle distances (differentiable torch float64)

`python tests/posefit_scene.py` runs r3g.posefit.fit on these two and records the loss curve and the final hard-mask IoU in
tests/golden/posefit_expect.json."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posefit_expect.json")
SIZE = (48, 64)
CAMERA = dict(R=np.eye(3), t=np.zeros(3), fx=60.0, fy=60.0, cx=32.0, cy=24.0)
FLOOR_NORMAL, FLOOR_POINT = np.array([0.05, -0.9, -0.43]), np.array([0.0, 1.0, 6.0])
TARGET = dict(uv=(0.3, -0.2), yaw=0.025, scale=1.1)      # yaw is multiplied by rotation_speed_mult = 20: half a radian
CONFIG = {"sigma": 1e-3, "faces_per_pixel": 20, "learning_rate": 0.01, "max_iterations": 80, "early_stop_min_iterations": 80}


def l_prism():
    """verts float64 [14, 3] in plane coordinates (y up, standing on y = 0), faces int64 [24, 3]; no symmetry"""
    ring = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 3), (0, 3), (0, 1)]
    v = [[x, 0.0, z] for x, z in ring] + [[x, 1.5, z] for x, z in ring]
    caps = [[0, 1, 2], [0, 2, 6], [6, 3, 4], [6, 4, 5]]
    f = [c for c in caps] + [[a + 7, c + 7, b + 7] for a, b, c in caps]
    for i in range(7):
        j = (i + 1) % 7
        f += [[i, i + 7, j], [j, i + 7, j + 7]]
    return np.array(v, np.float64), np.array(f, np.int64)


def plane_to_world():
    from r3g import plane
    return plane.plane_frame(FLOOR_NORMAL, FLOOR_POINT)[0]


def world_mesh():
    """the prism as the fit receives it: standing on the floor at the plane's origin"""
    v, f = l_prism()
    m = plane_to_world()
    return v @ m[:3, :3].T + m[:3, 3], f


def cam(dtype, device):
    return {k: (torch.as_tensor(v, dtype=dtype, device=device) if isinstance(v, np.ndarray) else v) for k, v in CAMERA.items()}


def render64(faces, sigma_px2, K):
    import softras_ref as R
    from r3g import softras
    c = cam(torch.float64, "cpu")

    def render(verts):
        pos = softras.pinhole(verts, c["R"], c["t"], c["fx"], c["fy"], c["cx"], c["cy"])
        return R.render(pos, faces, SIZE, K, sigma_px2, R.default_blur(float(np.float32(sigma_px2))))["alpha"]
    return render


def hard_mask(verts, faces):
    """pixels whose centre lies inside a face (float64) -> bool [H, W], and the face in front there"""
    import softras_ref as R
    from r3g import softras
    c = cam(torch.float64, "cpu")
    pos = softras.pinhole(torch.as_tensor(verts, dtype=torch.float64), c["R"], c["t"], c["fx"], c["fy"], c["cx"], c["cy"])
    r = R.render(pos, faces, SIZE, 1, 1.0, 0.0)
    return (r["face"][..., 0] >= 0).numpy(), r["face"][..., 0].numpy()


def iou(a, b):
    return float((a & b).sum()) / float((a | b).sum())


def boundary_share(mask):
    """the share of pixels within one pixel (8-neighbourhood) of the mask's boundary: those whose 3 x 3 window is not constant"""
    p = np.pad(mask, 1, mode="edge")
    win = np.stack([p[i:i + mask.shape[0], j:j + mask.shape[1]] for i in range(3) for j in range(3)])
    return float((win.min(0) != win.max(0)).mean())


def tri_dist2(p, tri):
    """squared distances of points [N, 3] to triangles [F, 3, 3] -> [N, F] (torch, differentiable): the plane's distance where the
    projection falls inside, else the nearest of the three segments"""
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    p = p[:, None]
    n = torch.cross(b - a, c - a, dim=-1)
    nn = (n * n).sum(-1)
    h = ((p - a) * n).sum(-1)
    proj = p - (h / nn)[..., None] * n
    inside = torch.ones_like(h, dtype=torch.bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (torch.cross(v - u, proj - u, dim=-1) * n).sum(-1) >= 0
    best = torch.where(inside, h * h / nn, torch.full_like(h, float("inf")))
    for u, v in ((a, b), (b, c), (c, a)):
        e = v - u
        t = (((p - u) * e).sum(-1) / (e * e).sum(-1)).clamp(0, 1)
        d = p - (u + t[..., None] * e)
        best = torch.minimum(best, torch.where(inside, best, (d * d).sum(-1)))
    return best


def point_face_loss64(base_verts, faces, points):
    tri = base_verts[torch.as_tensor(faces)]

    def loss(similarity):
        s, R, t = similarity
        local = ((points - t) @ R) / s
        return (s * s).reshape(()) * tri_dist2(local, tri).min(1).values.mean()
    return loss


def target_verts(dtype=torch.float64):
    """the prism in the pose the fit should find, by the same formulas as PlanarPose"""
    from r3g import posefit
    v, f = world_mesh()
    pose = posefit.PlanarPose(torch.as_tensor(v, dtype=dtype), torch.as_tensor(f), plane_to_world(), None, np.zeros(SIZE))
    with torch.no_grad():
        pose.translation_uv[0, 0], pose.translation_uv[0, 1] = TARGET["uv"]
        pose.rotation_yaw[0], pose.scale[0, 0] = TARGET["yaw"], TARGET["scale"]
        return pose.transform().numpy()


def scene(n_points=300, seed=0):
    """dict(verts, faces (the start), mask bool [H, W], cloud float64 [n, 3])"""
    v, f = world_mesh()
    tv = target_verts()
    mask, front = hard_mask(tv, f)
    seen = np.unique(front[front >= 0])
    rng = np.random.default_rng(seed)
    tri = tv[f[seen]]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    pick = rng.choice(len(seen), n_points, p=area / area.sum())
    r1, r2 = np.sqrt(rng.uniform(size=n_points)), rng.uniform(size=n_points)
    w = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], 1)
    cloud = (tri[pick] * w[:, :, None]).sum(1)
    return dict(verts=v, faces=f, mask=mask, cloud=cloud, target=tv)


def reference_fit(iterations=None):
    """r3g.posefit.fit with the two float64 restatements on the CPU -> (result dict, final hard-mask IoU)"""
    from r3g import posefit, softras
    sc = scene()
    cfg = dict(CONFIG) if iterations is None else dict(CONFIG, max_iterations=iterations)
    v, f = torch.as_tensor(sc["verts"]), torch.as_tensor(sc["faces"])
    pose = posefit.PlanarPose(v, f, plane_to_world(), render64(sc["faces"], softras.sigma_to_pixels(cfg["sigma"], *SIZE), cfg["faces_per_pixel"]),
                              sc["mask"].astype(np.float64), config=cfg)
    pose.point_loss = point_face_loss64(pose.base_verts_plane, sc["faces"], torch.as_tensor(sc["cloud"]))
    out = posefit.fit(pose)
    return out, iou(hard_mask(pose.transform().detach().numpy(), sc["faces"])[0], sc["mask"])


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "3d-re-gen_amd")]
    res, final_iou = reference_fit()
    sc = scene()
    start_iou = iou(hard_mask(sc["verts"], sc["faces"])[0], sc["mask"])
    with open(GOLDEN, "w") as fh:
        json.dump({"losses": res["losses"], "final_iou": final_iou, "start_iou": start_iou, "boundary_share": boundary_share(sc["mask"])}, fh)
    print("start IoU %.3f, final IoU %.3f, loss %.4f -> %.4f, boundary share %.3f" % (start_iou, final_iou, res["losses"][0], res["losses"][-1],
                                                                                     boundary_share(sc["mask"])))
