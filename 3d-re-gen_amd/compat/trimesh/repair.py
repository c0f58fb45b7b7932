"""trimesh.repair as the reference's consumers of this stage call it (pose fitting: fix_normals on every loaded GLB; the
background mesher: fill_holes, fix_winding, fix_normals(multibody=True), broken_faces), on the GPU through r3g.meshtopo and
r3g.meshfill.  The mesh is changed in place, as trimesh does.  fill_holes closes simple boundary loops by a fan from the loop's
first vertex (trimesh closes triangles and quads only and picks its own quad diagonal: the default max_loop=4 keeps to its
reach).  fix_invalid_faces and anything that welds geometry are not provided."""
import numpy as np


def fill_holes(mesh, max_loop=4):
    """close every simple boundary loop of at most max_loop edges -> is the mesh watertight afterwards"""
    return mesh.fill_holes(max_loop=max_loop)


def fix_winding(mesh):
    """reverse faces until every orientable body is consistently wound"""
    mesh._orient(0)


def fix_inversion(mesh, multibody=False):
    """reverse what is wound inward: every body of negative volume (multibody), or the whole mesh if its volume is negative.
    Implies fix_winding: the sign of a volume means something only on consistently wound faces."""
    mesh._orient(1 if multibody else 2)


def fix_normals(mesh, multibody=False):
    """fix_winding, then fix_inversion"""
    mesh._orient(1 if multibody else 2)


def broken_faces(mesh, color=None):
    """the ascending indices of the faces with an edge that is not shared by exactly two faces -> int64 [K]; with `color`
    (RGBA) they are painted in mesh.face_colors as well"""
    if mesh.is_empty:
        return np.zeros(0, np.int64)
    from r3g import meshtopo
    broken = meshtopo.broken_faces(*mesh.device_buffers()).cpu().numpy()
    if color is not None:
        colors = getattr(mesh, "face_colors", None)
        if colors is None or len(colors) != mesh.n_faces:
            colors = np.full((mesh.n_faces, 4), 255, np.uint8)
        colors[broken] = np.asarray(color, np.uint8)
        mesh.face_colors = colors
    return broken
