"""The reference's planar pose fit on this library: `PlanarPose` restates diff_model_planar.py's Model
(translation on the floor plane, yaw about its normal, uniform scale, pivot at the bottom centre in plane space) and `fit` its Adam
loop (pose_matching_planar.py).  The silhouette comes from r3g.softras, the 3D term from `point_face_loss` on r3g.meshdist's grid;
`r3g.plane.fit_floor`, `plane_frame` and `best_initial_yaw` provide the plane and the start.

`point_face_loss` is the point -> nearest-face half of pytorch3d's point_mesh_face_distance, computed on the STATIC base mesh: the
target points are moved by the inverse similarity in torch, r3g_meshdist_closest gives each one's closest point q on the base mesh,
q is held constant, and the loss is s^2 mean |T^-1 p - q|^2.  Because q minimises the distance, the derivative through q vanishes:
this is the exact gradient wherever the distance is differentiable (away from the medial axis).  `face_point_loss` is the other half,
face -> nearest point, on r3g.cloud's grid over the target points; `mesh_cloud_loss` is their sum, and
`cloud_loss(..., face_to_point=True)` puts it into a fit.  The default fit uses the point half alone, as before."""
import math

import torch
import torch.nn.functional as F

from . import cloud, meshdist, softras

DEFAULTS = {"silhoutte_loss": 1.0, "loss_3d": 1.0, "loss_bbox": 1.0, "rotation_speed_mult": 20.0, "learning_rate": 0.01, "max_iterations": 100,
            "early_stop_grad_threshold": 5e-3, "early_stop_min_iterations": 100, "sigma": 5e-7, "faces_per_pixel": 20}


def focal_loss(inputs, targets, alpha=0.5, gamma=2.0):
    bce = F.binary_cross_entropy(inputs, targets, reduction="none")
    pt = torch.exp(-bce)
    return (alpha * (1 - pt) ** gamma * bce).mean()


def dice_loss(P, T):
    return 1 - (2 * (P * T).sum() + 1e-6) / (P.sum() + T.sum() + 1e-6)


def silhouette_loss(P, T):
    """0.75 dice + 0.25 focal(alpha = 0.5, gamma = 2) of a soft mask P against a target T, both in [0, 1]"""
    return 0.75 * dice_loss(P, T) + 0.25 * focal_loss(P, T)


def bounding_box_loss(verts, bbox, ignore_axis=1):
    """mean over the vertices of how far they leave the box (min xyz, max xyz), the floor axis ignored"""
    box = torch.as_tensor(bbox, dtype=verts.dtype, device=verts.device)
    penalty = torch.relu(box[:3] - verts) + torch.relu(verts - box[3:])
    mask = torch.ones(3, dtype=verts.dtype, device=verts.device)
    mask[ignore_axis] = 0
    return (penalty * mask).sum() / verts.shape[0]


def yaw_matrix(angle):
    """rotation by `angle` (a 0-d or 1-element tensor) about plane-y: so3_exponential_map((0, angle, 0))"""
    a = angle.reshape(())
    c, s, o, l = torch.cos(a), torch.sin(a), torch.zeros_like(a), torch.ones_like(a)
    return torch.stack([torch.stack([c, o, s]), torch.stack([o, l, o]), torch.stack([-s, o, c])])


class BaseGrid:
    """section 4f's grid over the static base mesh, built once per fit; it lives in the device's shared context until the next
    r3g.meshdist.build there"""

    def __init__(self, verts, faces, resolution=None):
        self.device = verts.device
        self.info = meshdist.build(verts, faces, resolution)

    def closest(self, points):
        return meshdist.closest(points)[2]


def point_face_loss(base_mesh_grid, points, similarity):
    """points [N, 3] (world), similarity = (s, R [3, 3], t [3]) mapping the base mesh to the world: s^2 mean |T^-1 p - q|^2"""
    s, R, t = similarity
    local = ((points - t) @ R) / s      # R^T (p - t) / s, row vectors
    q = base_mesh_grid.closest(local.detach().to(torch.float32)).to(local.dtype)
    return (s * s).reshape(()) * ((local - q) ** 2).sum(-1).mean()


class PlanarPose(torch.nn.Module):
    """verts [V, 3] (world), faces [F, 3], plane_to_world 4 x 4 (r3g.plane.plane_frame).  render(pos_world) -> soft mask [H, W] and
    point_loss(similarity) -> scalar are the two device paths; `camera_renderer` and `cloud_loss` build the GPU ones."""

    def __init__(self, verts, faces, plane_to_world, render, mask, point_loss=None, config=None, background_bbox=None, resigmoid=True):
        super().__init__()
        self.config = dict(DEFAULTS, **(config or {}))
        dt, dev = verts.dtype, verts.device
        m = torch.as_tensor(plane_to_world, dtype=dt, device=dev)
        self.register_buffer("A", m[:3, :3].clone())
        self.register_buffer("origin", m[:3, 3].clone())
        in_plane = (verts - self.origin) @ self.A      # world_to_plane: A^T (x - o)
        lo, hi = in_plane.min(0).values, in_plane.max(0).values
        pivot = torch.stack([(lo[0] + hi[0]) / 2, lo[1], (lo[2] + hi[2]) / 2])
        self.register_buffer("base_verts_plane", in_plane - pivot)
        self.register_buffer("pivot_plane_centered", torch.stack([pivot[0], torch.zeros_like(pivot[1]), pivot[2]]))
        self.register_buffer("faces", faces)
        self.register_buffer("image_ref", torch.as_tensor(mask, dtype=dt, device=dev))
        self.background_bbox = background_bbox
        self.render, self.point_loss, self.resigmoid = render, point_loss, resigmoid
        self.translation_uv = torch.nn.Parameter(torch.zeros(1, 2, dtype=dt, device=dev))
        self.rotation_yaw = torch.nn.Parameter(torch.zeros(1, dtype=dt, device=dev))
        self.scale = torch.nn.Parameter(torch.ones(1, 1, dtype=dt, device=dev))

    def similarity(self):
        """(s, R, t): world = s R b + t for a vertex b of base_verts_plane"""
        Ry = yaw_matrix(self.rotation_yaw * self.config["rotation_speed_mult"])
        floor = torch.stack([self.translation_uv[0, 0], torch.zeros_like(self.translation_uv[0, 0]), self.translation_uv[0, 1]])
        return self.scale.reshape(()), self.A @ Ry, self.A @ (self.pivot_plane_centered + floor) + self.origin

    def transform(self):
        s, R, t = self.similarity()
        return s * (self.base_verts_plane @ R.T) + t

    def forward(self):
        verts = self.transform()
        P = self.render(verts)
        if self.resigmoid:
            P = torch.sigmoid(P)      # (the reference passes the shader's alpha through a second sigmoid)
        T = self.image_ref
        T = (T > 0.5).to(P.dtype) if T.max() > 1 else T
        loss = self.config["silhoutte_loss"] * silhouette_loss(P, T)
        if self.point_loss is not None:
            loss = loss + self.config["loss_3d"] * self.point_loss(self.similarity())
        if self.background_bbox is not None:
            loss = loss + self.config["loss_bbox"] * bounding_box_loss(verts, self.background_bbox)
        return loss, verts, P


def camera_renderer(faces, camera, size, config=None):
    """the GPU silhouette of world vertices under a pinhole camera dict(R, t, fx, fy, cx, cy): verts -> alpha [H, W].  The config's
    sigma is in squared NDC units, as the reference has it."""
    cfg = dict(DEFAULTS, **(config or {}))
    H, W = size
    sigma = softras.sigma_to_pixels(cfg["sigma"], H, W)
    state = {}

    def render(verts):
        if "csr" not in state:
            state["csr"] = softras.corner_csr(faces, verts.shape[0])
        pos = softras.pinhole(verts, camera["R"], camera["t"], camera["fx"], camera["fy"], camera["cx"], camera["cy"])
        return softras.rasterize(pos, faces, (H, W), K=cfg["faces_per_pixel"], sigma=sigma, csr=state["csr"])[0]
    return render


def face_point_loss(verts, faces, csr):
    """verts [V, 3] (world, differentiable), faces [F, 3], csr = r3g.softras.corner_csr(faces, V), against the cloud of the last
    r3g.cloud.build on the device: the mean over the usable faces of the squared distance to the face's nearest point
    (r3g.cloud.FaceCloudDistance).  Each face's nearest point p and the barycentric weights w of its closest point r are held
    constant, so d loss / d vertex_a = -2 w_a (p - r) / usable; because r minimises over the triangle and p over the cloud, the
    derivatives through both vanish: this is the exact gradient wherever the distance is differentiable.  A face with an index
    outside [0, V) or a non-finite vertex takes no part.  The cloud gets no gradient."""
    d2 = cloud.FaceCloudDistance.apply(verts, faces, csr)
    ok = ~torch.isnan(d2.detach())
    return torch.where(ok, d2, torch.zeros_like(d2)).sum() / ok.sum().clamp(min=1)


def mesh_cloud_loss(base_mesh_grid, points, similarity, verts, faces, csr):
    """[UPSTREAM-RECALLED] pytorch3d.loss.point_mesh_face_distance(mesh, pcl) for one mesh and one cloud, as recalled: the mean over
    the points of the squared distance to the nearest face (`point_face_loss`) plus the mean over the faces of the squared distance
    to the nearest point (`face_point_loss`).  verts are the base vertices moved by `similarity`; the cloud of r3g.cloud.build is
    `points`.  There is no min_triangle_area: a face without area is served by its edges."""
    return point_face_loss(base_mesh_grid, points, similarity) + face_point_loss(verts, faces, csr)


def cloud_loss(base_verts, faces, points, face_to_point=False):
    """the GPU 3D term of a fit: builds the base grid once -> point_loss(similarity).  face_to_point=True adds the face -> point half
    (`mesh_cloud_loss`): the cloud's grid is built once as well (it lives in the device's shared context until the next
    r3g.cloud.build, orient_normals or dbscan there), and the closure moves the base vertices by the similarity in torch."""
    grid = BaseGrid(base_verts, faces)
    if not face_to_point:
        return lambda similarity: point_face_loss(grid, points, similarity)
    cloud.build(points)
    csr = softras.corner_csr(faces, base_verts.shape[0])

    def both(similarity):
        s, R, t = similarity
        return mesh_cloud_loss(grid, points, similarity, s * (base_verts @ R.T) + t, faces, csr)
    return both


def fit(model, config=None, callback=None):
    """The reference's loop: Adam(lr), clip_grad_norm_(1.0), early stop once the (clipped) gradient norm falls below the threshold
    after early_stop_min_iterations -> dict(losses, iterations, grad_norm)"""
    cfg = dict(DEFAULTS, **(model.config if config is None else config))
    opt = torch.optim.Adam(model.parameters(), lr=cfg["learning_rate"])
    losses, norm = [], math.inf
    for i in range(int(cfg["max_iterations"])):
        opt.zero_grad()
        loss, verts, P = model()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
        norm = math.sqrt(sum(float(p.grad.norm()) ** 2 for p in model.parameters() if p.grad is not None))
        losses.append(float(loss.detach()))
        if callback is not None:
            callback(i, losses[-1], verts, P)
        opt.step()
        if i >= cfg["early_stop_min_iterations"] and norm < cfg["early_stop_grad_threshold"]:
            break
    return {"losses": losses, "iterations": len(losses), "grad_norm": norm}
