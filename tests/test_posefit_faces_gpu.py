"""r3g.posefit's face -> point half on the device: mesh_cloud_loss against the numpy restatement of the recalled pytorch3d formula, the
plate scene in which only the face half carries information (its Adam loop on the scale against the recorded float64 run), and the
L-prism fit with face_to_point=True against its recorded float64 run; without the flag the fit uses the point half alone."""
import json

import numpy as np
import pytest
import torch

import facecloud_ref as R
import meshdist_ref
import posefit_faces_scene as P
import posefit_scene as S

pytestmark = pytest.mark.gpu


def cuda(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def test_mesh_cloud_loss_against_the_restatement():
    from r3g import cloud, ffi, posefit, softras
    sc = S.scene()
    v, f, pts = sc["target"] * 1.07 + 0.02, sc["faces"], sc["cloud"]
    want, want_point, want_face = P.np_mesh_cloud_loss(np.float32(v), f, np.float32(pts))
    dv, df, dp = cuda(v), cuda(f, torch.int32), cuda(pts)
    ident = (torch.tensor(1.0, device="cuda"), torch.eye(3, device="cuda"), torch.zeros(3, device="cuda"))
    with ffi.device_lock(0):
        grid = posefit.BaseGrid(dv, df)
        cloud.build(dp)
        csr = softras.corner_csr(df, dv.shape[0])
        face_half = float(posefit.face_point_loss(dv, df, csr))
        both = float(posefit.mesh_cloud_loss(grid, dp, ident, dv, df, csr))
    ext = R.extent(v, pts)
    print("mesh_cloud_loss: device %.8e (face half %.8e), restatement %.8e (%.8e)" % (both, face_half, want, want_face))
    # each distance within the half's DIST_TOL of the extent and d (d^2) = 2 d dd: the mean moves by at most 2 sqrt(mean d^2) DIST_TOL
    # extent; the float32 mean of at most 300 terms adds 300 * 2^-24 relative, the sum of the halves one rounding more
    tol = lambda half, dist_tol: 2 * np.sqrt(half) * dist_tol * ext + 300 * 2.0 ** -24 * half      # noqa: E731
    assert abs(face_half - want_face) <= tol(want_face, R.DIST_TOL)
    assert abs(both - want) <= tol(want_face, R.DIST_TOL) + tol(want_point, meshdist_ref.DIST_TOL) + 2.0 ** -24 * want


def test_plate_scene_only_the_face_half_carries_information():
    from r3g import cloud, posefit, softras
    v, f, p = P.plate()
    dv, df, dp = cuda(v), cuda(f, torch.int32), cuda(p)
    s = torch.tensor(P.PLATE_SCALE, device="cuda", requires_grad=True)
    # (no ffi.device_lock around a backward: autograd runs it on a thread of its own, which takes the lock itself)
    grid = posefit.BaseGrid(dv, df)
    cloud.build(dp)
    csr = softras.corner_csr(df, dv.shape[0])
    point_half = posefit.point_face_loss(grid, dp, (s, torch.eye(3, device="cuda"), torch.zeros(3, device="cuda")))
    (g_point,) = torch.autograd.grad(point_half, s)
    face_half = posefit.face_point_loss(s * dv, df, csr)
    (g_face,) = torch.autograd.grad(face_half, s)
    # the point half is s^2 mean |l - q|^2 with l = p / s: l and the closest point q each carry a few float32 roundings of coordinates
    # below 0.5, |l - q| <= e = 8 * 2^-24 * 0.5 * sqrt(3); its derivative is 2 s mean |l - q|^2 - 2 s mean (l - q) . l, |l| <= 0.5
    e = 8 * 2.0 ** -24 * 0.5 * np.sqrt(3)
    print("plate: point half %.3e (gradient %.3e), face half %.6e (gradient %.6e)" % (float(point_half.detach()), float(g_point), float(face_half.detach()), float(g_face)))
    assert 0 <= float(point_half.detach()) <= P.PLATE_SCALE ** 2 * e * e
    assert abs(float(g_point)) <= 2 * P.PLATE_SCALE * e * e + 2 * P.PLATE_SCALE * e * 0.5
    assert float(face_half.detach()) > 1e-3 and float(g_face) > 1e-3


def test_plate_scale_loop_reaches_the_recorded_scale():
    """60 Adam steps on the scale alone; the scale, the move of the vertices and Adam in float64, as the recorded loops have them"""
    from r3g import cloud, posefit, softras
    with open(P.GOLDEN) as fh:
        rec = json.load(fh)
    v, f, p = P.plate()
    df = cuda(f, torch.int32)
    cloud.build(cuda(p))
    csr = softras.corner_csr(df, len(v))
    losses, scale = P.scale_loop(lambda verts: posefit.face_point_loss(verts, df, csr), torch.float64, "cuda")
    print("plate loop: device scale %.12f, float64 run %.12f, through the twin %.12f, margin %.3e; loss %.6e -> %.6e" %
          (scale, rec["plate_scale"], rec["plate_scale_twin"], rec["plate_margin"], losses[0], losses[-1]))
    assert losses[-1] < losses[0] and scale < P.PLATE_SCALE - 0.1
    assert abs(scale - rec["plate_scale"]) <= rec["plate_margin"]


def _prism_pose():
    from r3g import posefit
    sc = S.scene()
    verts, faces = cuda(sc["verts"]), cuda(sc["faces"], torch.int32)
    render = posefit.camera_renderer(faces, S.cam(torch.float32, "cuda"), S.SIZE, S.CONFIG)
    return sc, faces, posefit.PlanarPose(verts, faces, S.plane_to_world(), render, sc["mask"].astype(np.float32), config=S.CONFIG)


def test_planar_fit_with_the_face_half_reaches_the_recorded_fit():
    from r3g import posefit
    with open(P.GOLDEN) as fh:
        rec = json.load(fh)
    from r3g import cloud, softras
    sc, faces, pose = _prism_pose()
    pts = cuda(sc["cloud"])
    # the first loss, taken apart: the same model with the point half alone, and the face half of the start pose by itself
    pose.point_loss = posefit.cloud_loss(pose.base_verts_plane, faces, pts)
    with torch.no_grad():
        point_only = float(pose()[0])
        cloud.build(pts)
        face_half = float(posefit.face_point_loss(pose.transform(), faces, softras.corner_csr(faces, pose.base_verts_plane.shape[0])))
    pose.point_loss = posefit.cloud_loss(pose.base_verts_plane, faces, pts, face_to_point=True)
    out = posefit.fit(pose)
    final = S.iou(S.hard_mask(pose.transform().detach().cpu().numpy().astype(np.float64), sc["faces"])[0], sc["mask"])
    share = S.boundary_share(sc["mask"])
    print("fit with the face half: loss %.5f -> %.5f (float64 run: %.5f -> %.5f), IoU %.4f (float64 run %.4f, boundary share %.4f)" %
          (out["losses"][0], out["losses"][-1], rec["prism_losses"][0], rec["prism_losses"][-1], final, rec["prism_final_iou"], share))
    assert out["iterations"] == S.CONFIG["max_iterations"]
    # the kernels are deterministic, so the first loss is silhouette + (point half + face half) of the same float32 terms: it differs
    # from (silhouette + point half) + face half by the rounding of three float32 additions of values no larger than the loss, 2^-24 of it each
    assert abs(out["losses"][0] - (point_only + face_half)) <= 3 * 2.0 ** -24 * out["losses"][0] and face_half > 1e-3
    assert out["losses"][-1] < out["losses"][0]
    assert final >= rec["prism_final_iou"] - share


def test_without_the_flag_the_fit_uses_the_point_half_alone():
    """cloud_loss by default, with face_to_point=False, and the closure written out by hand (point_face_loss on a BaseGrid, the
    text cloud_loss had before the flag) give the same losses and the same bytes of the final vertices"""
    from r3g import posefit
    runs = []
    for variant in ("default", "explicit", "by hand"):
        sc, faces, pose = _prism_pose()
        pts = cuda(sc["cloud"])
        if variant == "default":
            pose.point_loss = posefit.cloud_loss(pose.base_verts_plane, faces, pts)
        elif variant == "explicit":
            pose.point_loss = posefit.cloud_loss(pose.base_verts_plane, faces, pts, face_to_point=False)
        else:
            grid = posefit.BaseGrid(pose.base_verts_plane, faces)
            pose.point_loss = lambda similarity: posefit.point_face_loss(grid, pts, similarity)      # noqa: B023
        out = posefit.fit(pose, config=dict(S.CONFIG, max_iterations=12))
        runs.append((out["losses"], pose.transform().detach().cpu().numpy().tobytes()))
    assert runs[0] == runs[1] == runs[2]
