#!/usr/bin/env python3
"""A point cloud (.ply) to a mesh (.glb) on the GPU: the reference's mesh_pointcloud (r3g.recon.mesh_pointcloud, DESIGN.md
section 4l) -- normals, their orientation, the Poisson surface, the density trim and the repairs.

    python tools/mesh_cloud.py IN.ply OUT.glb [--depth 8] [--remesh 0.5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-re-gen_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cloud")
    ap.add_argument("mesh")
    ap.add_argument("--depth", type=int, default=8, help="lattice of 2^depth + 1 nodes per axis, 2 .. 8")
    ap.add_argument("--remesh", type=float, default=0.5, help="share of the faces the decimation removes")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_cloud.py needs an MI355X (the product has no CPU path)")
    from r3g import cloud
    pc = cloud.load_ply(a.cloud)
    mesh = pc.to_mesh(depth=a.depth, remesh_percentage=a.remesh)
    mesh.export(a.mesh)
    print("%s: %d points -> %s: %d vertices, %d faces (%s)" % (a.cloud, len(pc.vertices), a.mesh, mesh.n_vertices, mesh.n_faces, mesh.metadata))


if __name__ == "__main__":
    main()
