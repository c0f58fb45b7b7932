"""The face -> point half of the pose fit's 3D loss without a GPU: the restatements of tests/posefit_faces_scene.py against each other
and against the host twin, the plate scene in which only the face half carries information, and the record in
tests/golden/posefit_faces_expect.json."""
import json

import numpy as np
import torch

import emu_facecloud as emu
import facecloud_ref as R
import posefit_faces_scene as P
import posefit_scene as S
from r3g import posefit


def test_public_names():
    assert callable(posefit.face_point_loss) and callable(posefit.mesh_cloud_loss)
    assert posefit.cloud_loss.__defaults__ == (False,) and "face_to_point" in posefit.cloud_loss.__code__.co_varnames
    assert posefit.DEFAULTS == {"silhoutte_loss": 1.0, "loss_3d": 1.0, "loss_bbox": 1.0, "rotation_speed_mult": 20.0, "learning_rate": 0.01,
                                "max_iterations": 100, "early_stop_grad_threshold": 5e-3, "early_stop_min_iterations": 100, "sigma": 5e-7,
                                "faces_per_pixel": 20}


def test_mesh_cloud_loss_restatements_agree():
    """the numpy restatement of the recalled point_mesh_face_distance, the torch float64 halves, and the twin's face half on the L-prism"""
    sc = S.scene()
    v, f, cloud = sc["target"] * 1.07 + 0.02, sc["faces"], sc["cloud"]
    total, point_half, face_half = P.np_mesh_cloud_loss(v, f, cloud)
    ident = (torch.tensor(1.0, dtype=torch.float64), torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    p64 = float(S.point_face_loss64(torch.tensor(v), f, torch.tensor(cloud))(ident))
    f64 = float(P.face_point_loss64(torch.tensor(v), f, torch.tensor(cloud)))
    assert abs(p64 - point_half) <= 1e-12 and abs(f64 - face_half) <= 1e-12 and abs(total - (p64 + f64)) <= 1e-12
    assert point_half > 1e-4 and face_half > 1e-4
    twin = emu.brute(cloud, v, f)[0].astype(np.float64).mean()
    # each distance within DIST_TOL of the extent and d (d^2) = 2 d dd: the mean moves by at most 2 sqrt(mean d^2) DIST_TOL extent
    assert abs(twin - face_half) <= 2 * np.sqrt(face_half) * R.DIST_TOL * R.extent(v, cloud)


def test_plate_scene_only_the_face_half_carries_information():
    v, f, p = P.plate()
    s = torch.tensor(P.PLATE_SCALE, dtype=torch.float64, requires_grad=True)
    v64, p64 = torch.tensor(v, dtype=torch.float64), torch.tensor(p, dtype=torch.float64)
    ident = (s, torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    point_half = S.point_face_loss64(v64, f, p64)(ident)
    (g_point,) = torch.autograd.grad(point_half, s)
    # every lattice point lies on the scaled plate, z = 0 exactly and the in-plane arithmetic on multiples of 1/15 and 1/8: rounding alone
    assert float(point_half.detach()) <= 1e-28 and abs(float(g_point)) <= 1e-14
    face_half = P.face_point_loss64(s * v64, f, p64)
    (g_face,) = torch.autograd.grad(face_half, s)
    assert float(face_half.detach()) > 1e-3 and float(g_face) > 1e-3
    # the twin's float32 face half and its gradient formula say the same
    loss = P.twin_face_point_loss(f, p)
    s32 = torch.tensor(P.PLATE_SCALE, dtype=torch.float64, requires_grad=True)
    twin = loss(s32 * v64)
    (g_twin,) = torch.autograd.grad(twin, s32)
    assert abs(float(twin.detach()) - float(face_half.detach())) <= 1e-8 and abs(float(g_twin) - float(g_face)) <= 1e-6 * float(g_face)


def test_plate_scale_loop_and_its_record():
    with open(P.GOLDEN) as fh:
        rec = json.load(fh)
    l64, s64, l32, s32 = P.plate_loops()
    print("plate: float64 scale %.12f, through the twin %.12f (recorded %.12f, %.12f), margin %.3e" %
          (s64, s32, rec["plate_scale"], rec["plate_scale_twin"], rec["plate_margin"]))
    assert l64[-1] < l64[0] and s64 < P.PLATE_SCALE - 0.1 and l32[-1] < l32[0] and s32 < P.PLATE_SCALE - 0.1
    assert abs(s64 - rec["plate_scale"]) <= 1e-10 and abs(s32 - rec["plate_scale_twin"]) <= 1e-10      # (a hundredth of the margin)
    assert rec["plate_margin"] == 4 * abs(rec["plate_scale"] - rec["plate_scale_twin"]) and rec["plate_margin"] > 0
    assert np.allclose([l64[0], l64[-1]], rec["plate_losses"], rtol=0, atol=1e-12)


def test_recorded_prism_fit_reproduces():
    """the first steps of the float64 loop with both halves, and what the record says about the whole"""
    with open(P.GOLDEN) as fh:
        rec = json.load(fh)
    with open(S.GOLDEN) as fh:
        point_only = json.load(fh)
    res, _ = P.reference_fit(iterations=3)
    assert np.allclose(res["losses"], rec["prism_losses"][:3], rtol=0, atol=1e-9)
    assert len(rec["prism_losses"]) == S.CONFIG["max_iterations"] and rec["prism_losses"][-1] < rec["prism_losses"][0]
    assert rec["prism_losses"][0] > point_only["losses"][0]                  # the face half adds to the first loss
    assert rec["prism_final_iou"] > point_only["start_iou"] + 0.2
