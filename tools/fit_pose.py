#!/usr/bin/env python3
"""Fit the planar pose of a mesh to a mask and a point cloud on the GPU, the way the reference's pose matching does once the
floor is known (r3g.posefit):

    python tools/fit_pose.py MESH.glb MASK.png CLOUD.ply --camera fx,fy,cx,cy [--sigma 5e-7] [--iterations 100] [--lr 0.01]
                             [--face-to-point]

The cloud and the mesh are in the camera's frame (x right, y down, z forward).  The floor comes from r3g.plane.fit_floor on the
cloud; the mask's size is the render size.  --face-to-point adds the face -> nearest-point half to the 3D term (section 4p), which
makes it pytorch3d's point_mesh_face_distance; without it the term is the point -> face half alone.  Prints one JSON line: the
plane, the fitted translation_uv, yaw (radians) and scale, the first and last loss and the iterations run.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("mask")
    ap.add_argument("cloud")
    ap.add_argument("--camera", required=True, help="fx,fy,cx,cy in pixels of the mask")
    ap.add_argument("--sigma", type=float, default=5e-7, help="in squared NDC units, as the reference's config has it")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--face-to-point", action="store_true", help="add the face -> nearest-point half to the 3D term")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise SystemExit("fit_pose.py needs a GPU (the product has no CPU path)")
    from r3g import cloud, plane, posefit
    from r3g.mesh import load_glb
    fx, fy, cx, cy = (float(x) for x in a.camera.split(","))
    mesh = load_glb(a.mesh)      # (a GLB as this stage writes it: one primitive, float32 positions, uint32 indices)
    verts = torch.from_numpy(np.asarray(mesh.vertices, np.float32).copy()).cuda()
    faces = torch.from_numpy(np.asarray(mesh.faces).astype(np.int32)).cuda()
    mask = (np.asarray(Image.open(a.mask).convert("L"), np.float32) > 127).astype(np.float32)
    pts = torch.from_numpy(cloud.load_ply(a.cloud).vertices).to(torch.float32).cuda()
    floor = plane.fit_floor(pts, 2000, 0.05, generator=torch.Generator().manual_seed(a.seed))
    m = plane.plane_frame(floor["normal"], floor["point"][0])[0]
    cfg = {"sigma": a.sigma, "max_iterations": a.iterations, "learning_rate": a.lr}
    cam = dict(R=torch.eye(3, device="cuda"), t=torch.zeros(3, device="cuda"), fx=fx, fy=fy, cx=cx, cy=cy)
    pose = posefit.PlanarPose(verts, faces, m, posefit.camera_renderer(faces, cam, mask.shape, cfg), mask, config=cfg)
    pose.point_loss = posefit.cloud_loss(pose.base_verts_plane, faces, pts, face_to_point=a.face_to_point)
    out = posefit.fit(pose)
    print(json.dumps({"tool": "fit_pose", "face_to_point": bool(a.face_to_point), "faces": int(faces.shape[0]), "points": int(pts.shape[0]), "size": list(mask.shape),
                      "plane_method": floor["method"], "normal": [float(v) for v in floor["normal"].cpu()],
                      "translation_uv": [float(v) for v in pose.translation_uv.detach().cpu().reshape(-1)],
                      "yaw": float(pose.rotation_yaw.detach()) * pose.config["rotation_speed_mult"], "scale": float(pose.scale.detach()),
                      "loss_first": out["losses"][0], "loss_last": out["losses"][-1], "iterations": out["iterations"]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
