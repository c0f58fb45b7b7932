"""Stand-in for the `trimesh` package where it is not installed (it is not in this image).

The reference stage imports trimesh only for `isinstance(mesh, trimesh.Trimesh)` in its optional remesh step
(src/2d_to_3d_models/run.py:21,36); the mesh object itself comes from hy3dgen.  Its evaluation
(src/evaluation/run_eval.py) loads two .ply clouds with `trimesh.load(path).vertices`; `PointCloud` and the PLY reader
of r3g/cloud.py serve that.  With this directory on PYTHONPATH
*instead of* a real trimesh, that check sees the mesh class of the MI355X path.  Do NOT put it on the path when the real
trimesh is installed."""
from r3g.cloud import PointCloud, load_ply as _load_ply  # noqa: F401
from r3g.mesh import Mesh as Trimesh, load_glb as _load_glb  # noqa: F401


def load(data):
    """a path ending in .ply: the PointCloud of its vertices (the reference's evaluation reads its clouds so); anything else
    (a .glb path, or GLB bytes) as before: the Mesh written by Mesh.to_glb"""
    if isinstance(data, str) and data.lower().endswith(".ply"):
        return _load_ply(data)
    return _load_glb(data)


import sys as _sys

if __name__ in _sys.modules:      # `import trimesh.repair`: fill_holes, fix_winding, fix_normals, fix_inversion, broken_faces on the GPU
    from . import repair  # noqa: F401
else:       # executed from its file under a name that is not in sys.modules: there is no package to import from
    import importlib.util as _util
    import os as _os
    _spec = _util.spec_from_file_location(__name__ + ".repair", _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "repair.py"))
    repair = _util.module_from_spec(_spec)
    _spec.loader.exec_module(repair)

__r3g_compat__ = True
__version__ = "0+r3g.compat"
