"""The scenes of the face-to-point pose-fit tests and the restatements of r3g.posefit.face_point_loss / mesh_cloud_loss (test-only):

    plate scene:   a flat square plate meshed 8 x 8, scaled by 1.5 about its centre, against a 16 x 16 lattice of points on the unscaled
                   plate.  Every point lies on the scaled plate, so the point -> face half is zero with a zero gradient; the faces that
                   stick out past the lattice are what the face -> point half sees.  `scale_loop` runs 60 Adam steps on the scale alone.
    L-prism scene: tests/posefit_scene.py's, with the face half added to its float64 point loss.

face_point_loss64 is a brute force over every (point, face) pair in torch float64 (differentiable); TwinFaceCloud evaluates the
product's float32 definition and gradient formula on the host (tests/emu_facecloud.py).  `python tests/posefit_faces_scene.py` records
tests/golden/posefit_faces_expect.json."""
import json
import os
import sys

import numpy as np
import torch

import facecloud_ref as R
import posefit_scene as S

GOLDEN = os.path.join(S.ROOT, "tests", "golden", "posefit_faces_expect.json")
PLATE_SCALE, PLATE_STEPS, PLATE_LR = 1.5, 60, 0.005


def plate():
    """(verts float32 [81, 3] of the UNSCALED plate about the origin, faces int32 [128, 3], lattice float32 [256, 3])"""
    v, f = R.grid_mesh(8, 1.0)
    t = np.linspace(-0.5, 0.5, 16)
    x, y = np.meshgrid(t, t, indexing="xy")
    return v, f, np.stack([x.ravel(), y.ravel(), np.zeros(256)], 1).astype(np.float32)


def np_mesh_cloud_loss(verts, faces, points):
    """[UPSTREAM-RECALLED] pytorch3d.loss.point_mesh_face_distance for one mesh and one cloud, as recalled, in numpy float64 over every
    pair: mean_i min_f d2(p_i, t_f) + mean_f min_i d2(p_i, t_f) -> (sum, point half, face half)"""
    d2 = R.point_triangle(np.asarray(points, np.float64)[:, None], np.asarray(verts, np.float64)[np.asarray(faces)][None])[0]     # [N, F]
    return d2.min(1).mean() + d2.min(0).mean(), d2.min(1).mean(), d2.min(0).mean()


def face_point_loss64(verts, faces, points):
    """torch float64, differentiable in verts: the mean over the faces of the squared distance to the nearest point"""
    return S.tri_dist2(points, verts[torch.as_tensor(faces, dtype=torch.int64)]).min(0).values.mean()


class TwinFaceCloud(torch.autograd.Function):
    """r3g.cloud.FaceCloudDistance through the host twin, with its conversions: verts of any float type are rounded to float32, dist2 [F]
    comes back in their type; the backward is the twin's gather on the float32 incoming gradient"""

    @staticmethod
    def forward(ctx, verts, faces, points, csr):
        import emu_facecloud as emu
        d2, ix, w, df, _ = emu.brute(points, verts.detach().to(torch.float32).numpy(), faces)
        ctx.saved = (ix, w, df, csr, verts.shape[0], verts.dtype)
        return torch.from_numpy(d2).to(verts.dtype)

    @staticmethod
    def backward(ctx, grad):
        import emu_facecloud as emu
        ix, w, df, csr, nv, dtype = ctx.saved
        return torch.from_numpy(emu.gather(nv, grad.to(torch.float32).numpy(), ix, w, df, *csr)).to(dtype), None, None, None


def twin_face_point_loss(faces, points):
    import emu_facecloud as emu
    csr = {}

    def loss(verts):
        if "csr" not in csr:
            csr["csr"] = emu.corner_csr(faces, verts.shape[0])
        d2 = TwinFaceCloud.apply(verts, faces, points, csr["csr"])
        return d2.sum() / d2.shape[0]
    return loss


def scale_loop(face_loss, dtype, device="cpu", steps=PLATE_STEPS):
    """Adam(lr = PLATE_LR) on the scale alone, from PLATE_SCALE: verts = scale * plate; face_loss(verts) -> scalar
    -> (losses, final scale)"""
    v = torch.as_tensor(plate()[0], dtype=dtype, device=device)
    scale = torch.nn.Parameter(torch.tensor(PLATE_SCALE, dtype=dtype, device=device))
    opt = torch.optim.Adam([scale], lr=PLATE_LR)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = face_loss(scale * v)
        loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    return losses, float(scale.detach())


def plate_loops():
    """the float64 loop and the same loop through the float32 twin -> (losses64, scale64, losses32, scale32).  Both keep the scale,
    the move of the vertices and Adam in float64, as the device test does: what differs is the float32 definition of the face half
    alone, not the order of a float32 reduction in torch."""
    v, f, p = plate()
    p64 = torch.as_tensor(p, dtype=torch.float64)
    l64, s64 = scale_loop(lambda verts: face_point_loss64(verts, f, p64), torch.float64)
    l32, s32 = scale_loop(twin_face_point_loss(f, p), torch.float64)
    return l64, s64, l32, s32


def reference_fit(iterations=None):
    """posefit_scene.reference_fit with the face half added to the float64 point loss -> (result dict, final hard-mask IoU)"""
    from r3g import posefit, softras
    sc = S.scene()
    cfg = dict(S.CONFIG) if iterations is None else dict(S.CONFIG, max_iterations=iterations)
    v, f = torch.as_tensor(sc["verts"]), torch.as_tensor(sc["faces"])
    pose = posefit.PlanarPose(v, f, S.plane_to_world(), S.render64(sc["faces"], softras.sigma_to_pixels(cfg["sigma"], *S.SIZE), cfg["faces_per_pixel"]),
                              sc["mask"].astype(np.float64), config=cfg)
    cloud = torch.as_tensor(sc["cloud"])
    point_half = S.point_face_loss64(pose.base_verts_plane, sc["faces"], cloud)

    def both(similarity):
        s, Rm, t = similarity
        return point_half(similarity) + face_point_loss64(s * (pose.base_verts_plane @ Rm.T) + t, sc["faces"], cloud)
    pose.point_loss = both
    out = posefit.fit(pose)
    return out, S.iou(S.hard_mask(pose.transform().detach().numpy(), sc["faces"])[0], sc["mask"])


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(S.ROOT, "tests"), os.path.join(S.ROOT, "3d-re-gen_amd")]
    l64, s64, l32, s32 = plate_loops()
    res, final_iou = reference_fit()
    with open(GOLDEN, "w") as fh:
        json.dump({"plate_scale": s64, "plate_scale_twin": s32, "plate_margin": 4 * abs(s64 - s32), "plate_losses": [l64[0], l64[-1]],
                   "prism_losses": res["losses"], "prism_final_iou": final_iou}, fh)
    print("plate: scale %.9f (twin %.9f), loss %.6e -> %.6e; prism: loss %.4f -> %.4f, final IoU %.4f" %
          (s64, s32, l64[0], l64[-1], res["losses"][0], res["losses"][-1], final_iou))
