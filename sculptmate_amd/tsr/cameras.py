"""Cameras and rays on the host, with the names, signatures and results of TripoSR/tsr/utils.py:115-149 and 255-397:
`rays_intersect_bbox`, `get_ray_directions`, `get_rays`, `get_spherical_cameras`.

Everything here is torch on the CPU in fp32, each operation in the reference's order: the rays that reach the ray kernel
(csrc/render.hip) are the reference's bit for bit (tests/test_render_host.py).  The box test below restates what the kernel
does per ray; the kernel does not call it.
"""
import functools
import math

import torch
import torch.nn.functional as F


def rays_intersect_bbox(rays_o, rays_d, radius, near: float = 0.0, valid_thresh: float = 0.01):
    """Slab test of rays against the cube of half-edge (1 - 1e-3) * radius -> (t_near [..., 1], t_far [..., 1], valid [...]).
    A direction component smaller than 1e-6 in magnitude counts as +1e-6 (also a negative one); t_near is clamped at `near`;
    a ray is valid when t_far - t_near > valid_thresh, and both distances of an invalid ray are zero."""
    lead = rays_o.shape[:-1]
    o, d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    d_safe = torch.where(d.abs() < 1e-6, torch.full_like(d, 1e-6), d)
    if isinstance(radius, (int, float)):
        radius = torch.tensor([[-radius, radius]] * 3, dtype=torch.float32, device=o.device)
    box = (1.0 - 1.0e-3) * radius
    at_hi = (box[..., 1] - o) / d_safe
    at_lo = (box[..., 0] - o) / d_safe
    t_near = torch.minimum(at_hi, at_lo).amax(dim=-1).clamp_min(near)
    t_far = torch.maximum(at_hi, at_lo).amin(dim=-1)
    valid = t_far - t_near > valid_thresh
    t_near = torch.where(valid, t_near, torch.zeros_like(t_near))
    t_far = torch.where(valid, t_far, torch.zeros_like(t_far))
    return t_near.view(*lead, 1), t_far.view(*lead, 1), valid.view(*lead)


def get_ray_directions(H: int, W: int, focal, principal=None, use_pixel_centers: bool = True, normalize: bool = True):
    """Camera-space directions [H, W, 3] of the pixel grid: x right, y up, looking down -z."""
    half = 0.5 if use_pixel_centers else 0
    if isinstance(focal, float):
        fx = fy = focal
        cx, cy = W / 2, H / 2
    else:
        fx, fy = focal
        assert principal is not None
        cx, cy = principal
    u, v = torch.meshgrid(torch.arange(W, dtype=torch.float32) + half, torch.arange(H, dtype=torch.float32) + half,
                          indexing="xy")
    dirs = torch.stack([(u - cx) / fx, -(v - cy) / fy, -torch.ones_like(u)], -1)
    return F.normalize(dirs, dim=-1) if normalize else dirs


def get_rays(directions, c2w, keepdim: bool = False, normalize: bool = False):
    """Rotate camera-space directions into the world with the camera-to-world matrices -> (rays_o, rays_d).
    directions [N, 3] | [H, W, 3] | [B, H, W, 3]; c2w [4, 4] | [B, 4, 4] (or one per ray for [N, 3])."""
    assert directions.shape[-1] == 3
    if directions.ndim == 2:
        c2w = c2w[None] if c2w.ndim == 2 else c2w
        assert c2w.ndim == 3
        rot, pos, dirs = c2w[:, :3, :3], c2w[:, :3, 3], directions[:, None, :]
    elif directions.ndim == 3:
        assert c2w.ndim in (2, 3)
        dirs = directions[:, :, None, :] if c2w.ndim == 2 else directions[None, :, :, None, :]
        rot = c2w[None, None, :3, :3] if c2w.ndim == 2 else c2w[:, None, None, :3, :3]
        pos = c2w[None, None, :3, 3] if c2w.ndim == 2 else c2w[:, None, None, :3, 3]
    else:
        assert directions.ndim == 4 and c2w.ndim == 3
        dirs, rot, pos = directions[:, :, :, None, :], c2w[:, None, None, :3, :3], c2w[:, None, None, :3, 3]
    rays_d = (dirs * rot).sum(-1)
    rays_o = pos.expand(rays_d.shape)
    if normalize:
        rays_d = F.normalize(rays_d, dim=-1)
    if not keepdim:
        rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    return rays_o, rays_d


@functools.lru_cache(maxsize=32)
def _spherical_cameras(n_views, elevation_deg, camera_distance, fovy_deg, height, width):
    azimuth = torch.linspace(0, 360.0, n_views + 1)[:n_views] * math.pi / 180
    elevation = torch.full_like(azimuth, elevation_deg) * math.pi / 180
    dist = torch.full_like(azimuth, camera_distance)
    # x back, y right, z up; azimuth from +x towards +y
    pos = torch.stack([dist * torch.cos(elevation) * torch.cos(azimuth),
                       dist * torch.cos(elevation) * torch.sin(azimuth),
                       dist * torch.sin(elevation)], dim=-1)
    world_up = torch.as_tensor([0, 0, 1], dtype=torch.float32)[None, :].repeat(n_views, 1)
    fovy = torch.full_like(azimuth, fovy_deg) * math.pi / 180
    lookat = F.normalize(torch.zeros_like(pos) - pos, dim=-1)
    # The reference calls torch.cross without `dim`, which takes the FIRST axis of length 3: the view axis when n_views == 3.
    # Its three-view turntable is therefore not a turntable; kept, because the contract is the reference's rays bit for bit.
    axis = 0 if n_views == 3 else -1
    right = F.normalize(torch.cross(lookat, world_up, dim=axis), dim=-1)
    up = F.normalize(torch.cross(right, lookat, dim=axis), dim=-1)
    top = torch.cat([torch.stack([right, up, -lookat], dim=-1), pos[:, :, None]], dim=-1)
    c2w = torch.cat([top, torch.zeros_like(top[:, :1])], dim=1)
    c2w[:, 3, 3] = 1.0
    # the unit-focal directions are normalised FIRST, then x and y are divided by the focal length, and the rotated result is
    # normalised again (utils.py:383-395): not the pinhole directions of that focal length, but what the reference renders
    focal = 0.5 * height / torch.tan(0.5 * fovy)
    dirs = get_ray_directions(H=height, W=width, focal=1.0)[None].repeat(n_views, 1, 1, 1)
    dirs[..., :2] = dirs[..., :2] / focal[:, None, None, None]
    rays_o, rays_d = get_rays(dirs, c2w, keepdim=True, normalize=True)
    return rays_o.contiguous(), rays_d.contiguous()


def get_spherical_cameras(n_views: int, elevation_deg: float, camera_distance: float, fovy_deg: float, height: int, width: int):
    """Turntable of n_views cameras on a circle at `elevation_deg`, looking at the origin -> (rays_o, rays_d), each
    [n_views, height, width, 3] on the host.  Cached per argument tuple; the tensors returned are the caller's own copies."""
    o, d = _spherical_cameras(int(n_views), float(elevation_deg), float(camera_distance), float(fovy_deg), int(height), int(width))
    return o.clone(), d.clone()
