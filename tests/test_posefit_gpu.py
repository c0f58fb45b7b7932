"""r3g.posefit on the device: the gradient of point_face_loss against float64 central differences of a brute-force restatement,
and the whole planar fit (soft silhouettes, point-to-face term, Adam) against the recorded float64 run of the same loop."""
import json

import numpy as np
import pytest
import torch

import posefit_scene as S

pytestmark = pytest.mark.gpu


def offset_points(n=120, seed=1, lift=0.05, inner=0.2):
    """points `lift` above interior points (every barycentric >= `inner`) of the prism's faces, in plane coordinates: the nearest
    feature is that face's inside, and the test asserts by what margin"""
    v, f = S.l_prism()
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(f), n)
    w = rng.dirichlet(np.ones(3), n) * (1 - 3 * inner) + inner
    tri = v[f[pick]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    centre = v.mean(0)
    base = (tri * w[:, :, None]).sum(1)
    nrm *= np.sign(((base - centre) * nrm).sum(1, keepdims=True))      # outward, whatever the winding
    return base + lift * nrm


def test_point_face_loss_gradient():
    from r3g import posefit
    v, f = S.l_prism()
    pts = offset_points()
    d2 = np.sort(S.tri_dist2(torch.tensor(pts), torch.tensor(v)[torch.tensor(f)]).numpy(), 1)
    # margin: every other face is at least 0.03 farther (by distance) unless it is the coplanar neighbour, which gives the same point
    far = np.sqrt(d2[:, 1:]) - np.sqrt(d2[:, :1])
    assert np.all((far > 0.03) | (far < 1e-12)) and np.all(np.abs(np.sqrt(d2[:, 0]) - 0.05) < 1e-12)
    # a similarity near the identity, applied to the points so that T^-1 p lands on `pts` at the expansion point
    s0, yaw0, t0 = 1.1, 0.3, np.array([0.2, -0.1, 0.4])

    def sim(par):
        s, yaw, t = par[0], par[1], par[2:5]
        return s, posefit.yaw_matrix(yaw), t
    R0 = posefit.yaw_matrix(torch.tensor(yaw0, dtype=torch.float64)).numpy()
    world = s0 * pts @ R0.T + t0
    par0 = np.concatenate([[s0, yaw0], t0])
    ref_loss = S.point_face_loss64(torch.tensor(v), f, torch.tensor(world))

    def loss64(p):
        return float(ref_loss(sim(torch.tensor(p))))
    h, fd = 1e-6, np.zeros(5)
    for i in range(5):
        a, b = par0.copy(), par0.copy()
        a[i] += h
        b[i] -= h
        fd[i] = (loss64(a) - loss64(b)) / (2 * h)
    grid = posefit.BaseGrid(torch.tensor(v, dtype=torch.float32).cuda(), torch.tensor(f, dtype=torch.int32).cuda())
    par = torch.tensor(par0, device="cuda", requires_grad=True)
    loss = posefit.point_face_loss(grid, torch.tensor(world, device="cuda"), sim(par))
    loss.backward()
    got = par.grad.cpu().numpy()
    print("point_face_loss: loss %.6e (float64 %.6e), gradient %s, central differences %s" % (float(loss), loss64(par0), got, fd))
    # q comes back as float32: |error| <= 8 * 2^-24 * max |coordinate| <= 2e-6; the gradient 2 s^2 mean((l - q) . dl) moves by at most
    # 2 s^2 * 2e-6 * max |dl| (<= 4 here): 2e-5.  The central differences of a piecewise quadratic add 1e-9.
    assert abs(float(loss) - loss64(par0)) <= 1e-6
    assert np.abs(got - fd).max() <= 2e-5 and np.abs(fd).max() > 1e-3


def test_planar_fit_reaches_the_recorded_fit():
    from r3g import posefit
    with open(S.GOLDEN) as fh:
        rec = json.load(fh)
    sc = S.scene()
    verts = torch.tensor(sc["verts"], dtype=torch.float32, device="cuda")
    faces = torch.tensor(sc["faces"], dtype=torch.int32, device="cuda")
    render = posefit.camera_renderer(faces, S.cam(torch.float32, "cuda"), S.SIZE, S.CONFIG)
    pose = posefit.PlanarPose(verts, faces, S.plane_to_world(), render, sc["mask"].astype(np.float32), config=S.CONFIG)
    pose.point_loss = posefit.cloud_loss(pose.base_verts_plane, faces, torch.tensor(sc["cloud"], dtype=torch.float32, device="cuda"))
    out = posefit.fit(pose)
    final = S.iou(S.hard_mask(pose.transform().detach().cpu().numpy().astype(np.float64), sc["faces"])[0], sc["mask"])
    share = S.boundary_share(sc["mask"])
    print("fit: loss %.5f -> %.5f (float64 run: %.5f -> %.5f), IoU %.4f (float64 run %.4f, boundary share %.4f), %d iterations" %
          (out["losses"][0], out["losses"][-1], rec["losses"][0], rec["losses"][-1], final, rec["final_iou"], share, out["iterations"]))
    assert out["iterations"] == S.CONFIG["max_iterations"]
    assert out["losses"][-1] < out["losses"][0]
    assert final >= rec["final_iou"] - share
