"""Differentiable soft silhouettes on the GPU (include/r3g.h "soft silhouettes"): the renderer behind the
reference's planar pose fit, where upstream builds pytorch3d's MeshRasterizer(blur_radius, faces_per_pixel) with
SoftSilhouetteShader (utils_SR/render_utils.py).

`rasterize` is the K-nearest soft rasteriser (r3g_softras_forward); with a `pos` that requires grad its alpha carries the
gradient to the vertices' xy through `SoftSilhouette` (r3g_softras_backward: face-centric sums in a fixed order, then a gather
over `corner_csr`; no floating-point atomics, so the same bits on every call).  z receives no gradient.  Positions are in PIXEL
coordinates: pixel (row i, column j) samples (j + 0.5, i + 0.5), row 0 is the top; sigma and blur_radius are in squared pixels.
`ndc_to_pixels` / `sigma_to_pixels` carry pytorch3d's screen convention over, so the reference's `sigma: 5e-7` passes through
unchanged; `pinhole` projects camera-space vertices.  There is no CPU path: tensors live on the GPU."""
import ctypes
import math

import torch

from . import ffi

REPORT = ("pairs", "used", "skipped", "tiles")
BACK_REPORT = ("found",)
PASSES = ("bin", "forward", "backward", "gather")
MAX_K = 32


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _mesh_args(pos, tri):
    if not (isinstance(pos, torch.Tensor) and pos.is_cuda and pos.ndim == 2 and pos.shape[1] == 3):
        raise ValueError("expected pos as a CUDA tensor [V, 3] (there is no CPU path)")
    if not (isinstance(tri, torch.Tensor) and tri.ndim == 2 and tri.shape[1] == 3):
        raise ValueError("expected tri as a tensor [F, 3]")
    return pos.detach().to(torch.float32).contiguous(), tri.detach().to(device=pos.device, dtype=torch.int32).contiguous()


def default_blur_radius(sigma):
    """the reference's blur radius: ln(1 / 1e-4 - 1) * sigma"""
    return math.log(1.0 / 1e-4 - 1.0) * float(sigma)


def corner_csr(tri, n_verts):
    """the corners of each vertex, for the gather of the backward: (start int32 [V + 1], ids int32 [corners]); vertex v owns
    ids[start[v]:start[v + 1]], corner 3 f + a in ascending order (a stable sort of tri.flatten()).  Built once per mesh; a corner
    whose index lies outside [0, V) belongs to no vertex (its face is not drawn)."""
    flat = tri.detach().reshape(-1).to(torch.int64)
    ok = (flat >= 0) & (flat < n_verts)
    key = torch.where(ok, flat, torch.full_like(flat, n_verts))
    ids = torch.sort(key, stable=True).indices[:int(ok.sum())]
    start = torch.zeros(n_verts + 1, dtype=torch.int64, device=flat.device)
    if n_verts:
        start[1:] = torch.cumsum(torch.bincount(flat[ok], minlength=n_verts), 0)
    return start.to(torch.int32).contiguous(), ids.to(torch.int32).contiguous()


def forward_raw(pos, tri, size, K, sigma, blur_radius):
    """r3g_softras_forward -> (alpha [H, W], face int32 [H, W, K], dist [H, W, K], zbuf [H, W, K], report dict)"""
    p, t = _mesh_args(pos, tri)
    H, W = int(size[0]), int(size[1])
    dev = p.device.index or 0
    ok = 1 <= H <= 16384 and 1 <= W <= 16384 and 1 <= int(K) <= MAX_K      # (the library refuses these too; nothing is allocated for them)
    alpha = torch.empty((H, W) if ok else (1, 1), dtype=torch.float32, device=p.device)
    face = torch.empty((H, W, int(K)) if ok else (1, 1, 1), dtype=torch.int32, device=p.device)
    dist, zbuf = torch.empty_like(face, dtype=torch.float32), torch.empty_like(face, dtype=torch.float32)
    rep = (ctypes.c_int64 * 8)()
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_softras_forward(ffi.context(dev), _ptr(p), p.shape[0], _ptr(t), t.shape[0], H, W, int(K), float(sigma),
                                                float(blur_radius), _ptr(alpha), _ptr(face), _ptr(dist), _ptr(zbuf), rep, ffi.stream_ptr()))
    return alpha, face, dist, zbuf, dict(zip(REPORT, (int(v) for v in rep)))


def backward_raw(pos, tri, size, K, sigma, blur_radius, face, dist, grad_alpha, csr=None):
    """r3g_softras_backward -> (grad_face [F, 3, 2], grad_pos [V, 3], report dict); csr = corner_csr(tri, V) (built when None)"""
    p, t = _mesh_args(pos, tri)
    H, W = int(size[0]), int(size[1])
    dev = p.device.index or 0
    face = face.detach().to(torch.int32).contiguous()
    dist = dist.detach().to(torch.float32).contiguous()
    ga = grad_alpha.detach().to(torch.float32).contiguous()
    if tuple(face.shape) != (H, W, int(K)) or tuple(dist.shape) != (H, W, int(K)) or tuple(ga.shape) != (H, W):
        raise ValueError("expected face, dist [H, W, K] and grad_alpha [H, W] of the forward")
    start, ids = csr if csr is not None else corner_csr(t, p.shape[0])
    if start.numel() != p.shape[0] + 1 or ids.numel() > 3 * t.shape[0]:
        raise ValueError("corner_csr of another mesh")
    gf = torch.empty((t.shape[0], 3, 2), dtype=torch.float32, device=p.device)
    gp = torch.empty((p.shape[0], 3), dtype=torch.float32, device=p.device)
    if ids.numel() < 3 * t.shape[0]:      # the library reads [0, 3 F) at most: pad the ids of a mesh with out-of-range corners
        ids = torch.cat([ids, torch.full((3 * t.shape[0] - ids.numel(),), -1, dtype=torch.int32, device=ids.device)])
    rep = (ctypes.c_int64 * 4)()
    with ffi.device_lock(dev), torch.cuda.device(p.device):
        ffi.check(ffi.lib().r3g_softras_backward(ffi.context(dev), _ptr(p), p.shape[0], _ptr(t), t.shape[0], H, W, int(K), float(sigma),
                                                 float(blur_radius), _ptr(face), _ptr(dist), _ptr(ga), _ptr(start), _ptr(ids), _ptr(gf), _ptr(gp),
                                                 rep, ffi.stream_ptr()))
    return gf, gp, dict(zip(BACK_REPORT, (int(v) for v in rep)))


def times(device=0):
    """milliseconds of the passes of the last complete forward / backward on the device's context -> dict over PASSES (-1: not run)"""
    ms = (ctypes.c_double * 4)()
    with ffi.device_lock(device):
        ffi.check(ffi.lib().r3g_softras_times(ffi.context(device), ms))
    return dict(zip(PASSES, (float(v) for v in ms)))


class SoftSilhouette(torch.autograd.Function):
    """alpha, face, dist, zbuf = SoftSilhouette.apply(pos, tri, size, K, sigma, blur_radius, csr); only alpha is differentiable, and
    only with respect to pos (its z column gets zeros)"""

    @staticmethod
    def forward(ctx, pos, tri, size, K, sigma, blur_radius, csr):
        alpha, face, dist, zbuf, _ = forward_raw(pos, tri, size, K, sigma, blur_radius)
        ctx.save_for_backward(pos.detach(), tri, face, dist)
        ctx.args = (tuple(size), int(K), float(sigma), float(blur_radius), csr)
        ctx.pos_dtype = pos.dtype
        ctx.mark_non_differentiable(face, dist, zbuf)
        return alpha, face, dist, zbuf

    @staticmethod
    def backward(ctx, grad_alpha, *_):
        pos, tri, face, dist = ctx.saved_tensors
        size, K, sigma, blur_radius, csr = ctx.args
        _, gp, _ = backward_raw(pos, tri, size, K, sigma, blur_radius, face, dist, grad_alpha, csr)
        return gp.to(ctx.pos_dtype), None, None, None, None, None, None


def rasterize(pos, tri, size, K=20, sigma=1e-4, blur_radius=None, csr=None):
    """The soft silhouette of a mesh -> alpha [H, W], face int32 [H, W, K] (-1: empty), dist [H, W, K], zbuf [H, W, K].
    pos [V, 3]: x, y in pixels, z the view depth; size = (H, W); sigma, blur_radius in squared pixels; blur_radius=None means
    ln(1 / 1e-4 - 1) * sigma, as in the reference.  alpha is differentiable with respect to pos; csr = corner_csr(tri, V) saves
    rebuilding it at every step of an optimisation."""
    if blur_radius is None:
        blur_radius = default_blur_radius(sigma)
    if pos.requires_grad and csr is None:
        csr = corner_csr(tri.to(pos.device), pos.shape[0])
    return SoftSilhouette.apply(pos, tri, tuple(size), K, sigma, blur_radius, csr)


def ndc_to_pixels(verts_ndc, H, W):
    """pytorch3d's NDC (+x left, +y up, the shorter side of the image spans [-1, 1]) -> pixel-space pos; z passes through"""
    half = 0.5 * min(int(H), int(W))
    x = 0.5 * W - verts_ndc[..., 0] * half
    y = 0.5 * H - verts_ndc[..., 1] * half
    return torch.stack([x, y, verts_ndc[..., 2]], -1)


def sigma_to_pixels(sigma_ndc, H, W):
    """a sigma or blur radius given in squared NDC units (as the reference's config has it) -> squared pixels"""
    half = 0.5 * min(int(H), int(W))
    return sigma_ndc * half * half


def pinhole(verts, R, t, fx, fy, cx, cy):
    """world vertices [V, 3] -> pixel-space pos [V, 3] of a pinhole camera looking down +z with y down: X_cam = R X + t,
    (fx X / Z + cx, fy Y / Z + cy, Z).  Plain torch, differentiable."""
    cam = verts @ R.transpose(-1, -2) + t
    z = cam[..., 2]
    return torch.stack([fx * cam[..., 0] / z + cx, fy * cam[..., 1] / z + cy, z], -1)
