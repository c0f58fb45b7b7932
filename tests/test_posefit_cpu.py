"""r3g.posefit's plain-torch parts against a numpy restatement of the reference's formulas (diff_model_planar.py: focal and dice
loss, bounding_box_loss, Model.forward's transform), r3g.softras's screen conventions, and the recorded float64 fit.  No GPU."""
import json

import numpy as np
import torch

import posefit_scene as S
from r3g import posefit, softras


def np_silhouette_loss(P, T):
    bce = -(T * np.log(P) + (1 - T) * np.log(1 - P))
    focal = (0.5 * (1 - np.exp(-bce)) ** 2 * bce).mean()
    dice = 1 - (2 * (P * T).sum() + 1e-6) / (P.sum() + T.sum() + 1e-6)
    return 0.75 * dice + 0.25 * focal


def test_silhouette_loss():
    rng = np.random.default_rng(0)
    P, T = rng.uniform(0.01, 0.99, (48, 64)), (rng.uniform(size=(48, 64)) > 0.6).astype(np.float64)
    got = float(posefit.silhouette_loss(torch.tensor(P), torch.tensor(T)))
    assert abs(got - np_silhouette_loss(P, T)) <= 1e-12
    assert float(posefit.silhouette_loss(torch.tensor(T * 0.999998 + 1e-6), torch.tensor(T))) < 1e-5


def test_bounding_box_loss():
    rng = np.random.default_rng(1)
    v = rng.uniform(-2, 2, (50, 3))
    box = [-1.0, -0.5, -1.5, 1.2, 0.4, 0.9]
    pen = np.maximum(np.array(box[:3]) - v, 0) + np.maximum(v - np.array(box[3:]), 0)
    pen[:, 1] = 0      # the floor axis is ignored
    assert abs(float(posefit.bounding_box_loss(torch.tensor(v), box)) - pen.sum() / 50) <= 1e-12
    assert float(posefit.bounding_box_loss(torch.tensor(v * 0.1), box)) == 0.0


def rodrigues(w):
    """so3_exponential_map of one axis-angle vector"""
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def test_planar_pose_transform():
    v, f = S.world_mesh()
    m = S.plane_to_world()
    pose = posefit.PlanarPose(torch.tensor(v), torch.tensor(f), m, None, np.zeros(S.SIZE))
    with torch.no_grad():
        pose.translation_uv[0, 0], pose.translation_uv[0, 1], pose.rotation_yaw[0], pose.scale[0, 0] = 0.4, -0.7, 0.031, 1.3
    # Model.__init__ and Model.forward, step by step
    inv = np.linalg.inv(m)
    vp = v @ inv[:3, :3].T + inv[:3, 3]
    lo, hi = vp.min(0), vp.max(0)
    pivot = np.array([(lo[0] + hi[0]) / 2, lo[1], (lo[2] + hi[2]) / 2])
    base = vp - pivot
    rotated = (base * 1.3) @ rodrigues(np.array([0, 0.031 * 20.0, 0])).T
    translated = rotated + np.array([pivot[0], 0.0, pivot[2]]) + np.array([0.4, 0.0, -0.7])
    want = translated @ m[:3, :3].T + m[:3, 3]
    assert np.abs(pose.transform().detach().numpy() - want).max() <= 1e-12
    s, R, t = pose.similarity()
    assert np.abs((float(s) * base @ R.detach().numpy().T + t.detach().numpy()) - want).max() <= 1e-12
    # at the start the model reproduces its input up to the lift onto the floor (pivot y -> 0)
    start = posefit.PlanarPose(torch.tensor(v), torch.tensor(f), m, None, np.zeros(S.SIZE)).transform().detach().numpy()
    assert np.abs(start - (v - lo[1] * m[:3, 1])).max() <= 1e-12


def test_ndc_to_pixels_and_sigma():
    ndc = torch.tensor([[1.0, 1.0, 2.0], [-1.0, -1.0, 3.0], [0.0, 0.0, 4.0]], dtype=torch.float64)
    sq = softras.ndc_to_pixels(ndc, 64, 64).numpy()      # +x left, +y up: (1, 1) is the top-left corner
    assert np.array_equal(sq, [[0, 0, 2], [64, 64, 3], [32, 32, 4]])
    wide = softras.ndc_to_pixels(ndc, 48, 64).numpy()     # the shorter side (48 rows) spans [-1, 1]; the longer one 64 / 48 of it
    assert np.array_equal(wide, [[8, 0, 2], [56, 48, 3], [32, 24, 4]])
    tall = softras.ndc_to_pixels(ndc, 64, 48).numpy()
    assert np.array_equal(tall, [[0, 8, 2], [48, 56, 3], [24, 32, 4]])
    # pixel (i, j) samples (j + 0.5, i + 0.5): its NDC centre maps back onto it
    j, i = 5, 9
    c = torch.tensor([[1 - (2 * j + 1) / 64, 1 - (2 * i + 1) / 64, 1.0]], dtype=torch.float64)
    assert np.allclose(softras.ndc_to_pixels(c, 64, 64).numpy()[0, :2], [j + 0.5, i + 0.5], atol=1e-12)
    assert softras.sigma_to_pixels(5e-7, 1024, 1024) == 5e-7 * 512 * 512 and softras.sigma_to_pixels(1.0, 48, 64) == 576.0
    assert abs(softras.default_blur_radius(1e-4) - np.log(1 / 1e-4 - 1) * 1e-4) < 1e-18


def test_pinhole():
    v = torch.tensor([[0.5, -0.25, 2.0]], dtype=torch.float64, requires_grad=True)
    R, t = torch.eye(3, dtype=torch.float64), torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64)
    pos = softras.pinhole(v, R, t, 60.0, 50.0, 32.0, 24.0)
    assert np.allclose(pos.detach().numpy(), [[32 + 60 * 0.5 / 4, 24 - 50 * 0.25 / 4, 4.0]], atol=1e-12)
    pos[0, 0].backward()
    assert np.allclose(v.grad.numpy(), [[60 / 4, 0, -60 * 0.5 / 16]], atol=1e-12)


def test_recorded_fit_reproduces():
    """the first steps of the float64 loop behind tests/golden/posefit_expect.json, and what the record says about the whole"""
    with open(S.GOLDEN) as fh:
        rec = json.load(fh)
    res, _ = S.reference_fit(iterations=3)
    assert np.allclose(res["losses"], rec["losses"][:3], rtol=0, atol=1e-9)
    assert len(rec["losses"]) == S.CONFIG["max_iterations"] and rec["losses"][-1] < rec["losses"][0]
    assert rec["final_iou"] > rec["start_iou"] + 0.2
    sc = S.scene()
    assert abs(rec["boundary_share"] - S.boundary_share(sc["mask"])) < 1e-12 and 0 < rec["boundary_share"] < 0.2
