"""Thin torch-tensor front-ends over the C ABI (include/sculpt_hip.h).

torch is plumbing here: it owns HBM allocations and the current HIP stream; every function below
passes raw device pointers + sizes into libsculpt_hip.so.  No function has a CPU path.
"""
import ctypes
import math
import numbers
import struct
import threading
import os

import numpy as np
import torch

from . import _lib
from ._lib import SculptError, check, lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _opt(t):
    return _ptr(t) if t is not None else None


def _req(t, dtype, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise SculptError("%s must be a CUDA/HIP tensor (no CPU fallback)" % name)
    if t.dtype != dtype:
        raise SculptError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise SculptError("%s must be contiguous" % name)
    return t


# ----------------------------------------------------------------------------------------------
# NeRF decoder
# ----------------------------------------------------------------------------------------------
class PackedMLP:
    """Decoder weights re-ordered for the MFMA kernels (sculpt_mlp_pack), resident in HBM."""

    def __init__(self, weights, biases, device):
        Ws = [np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, np.float32)
              for w in weights]
        bs = [np.ascontiguousarray(b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b, np.float32)
              for b in biases]
        n = len(Ws)
        dims = np.array([Ws[0].shape[1]] + [w.shape[0] for w in Ws], np.int32)
        self.in_channels = int(dims[0])
        self.n_hidden = n - 2
        nbytes = lib.sculpt_mlp_packed_bytes(self.in_channels, self.n_hidden)
        host = np.zeros(nbytes // 4, np.float32)
        WP = (ctypes.c_void_p * n)(*[w.ctypes.data for w in Ws])
        BP = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
        check(lib.sculpt_mlp_pack(WP, BP, n, dims.ctypes.data, host.ctypes.data, nbytes))
        self.blob = torch.from_numpy(host).to(device)


class ChannelLastPlanes:
    """A scene code re-laid as [3][H][W][C] for the point-query kernel (sculpt_planes_channel_last)."""

    def __init__(self, planes):
        planes = _req(planes.contiguous(), torch.float32, "planes")
        _, self.C, self.H, self.W = planes.shape
        self.data = torch.empty((3, self.H, self.W, self.C), dtype=torch.float32, device=planes.device)
        check(lib.sculpt_planes_channel_last(_ptr(planes), self.C, self.H, self.W, _ptr(self.data), _stream()))


def triplane_query(planes, mlp, points, radius=0.87, density_bias=-1.0,
                   want=("density", "features", "density_act", "color"), align_corners=False):
    """query_triplane (nerf_renderer.py:41-91) at arbitrary points -> dict of [N,1]/[N,3] tensors.
    align_corners=True is SF3D.query_triplane's sampling (StableFast/sf3d/system.py:170-199).
    planes: [3,C,H,W] (reference layout) or a ChannelLastPlanes (much faster for many points)."""
    shape = points.shape[:-1]
    pts = _req(points.reshape(-1, 3).contiguous(), torch.float32, "points")
    N = pts.shape[0]
    flags = _lib.QUERY_ALIGN_CORNERS if align_corners else 0
    if isinstance(planes, ChannelLastPlanes):
        C, H, W = planes.C, planes.H, planes.W
        planes = planes.data
        flags |= _lib.QUERY_CHANNEL_LAST
    else:
        planes = _req(planes, torch.float32, "planes")
        _, C, H, W = planes.shape
    out = {}
    for k, w in (("density", 1), ("features", 3), ("density_act", 1), ("color", 3)):
        out[k] = torch.empty((N, w), dtype=torch.float32, device=pts.device) if k in want else None
    check(lib.sculpt_triplane_query_ex(_ptr(planes), C, H, W, _ptr(mlp.blob), mlp.n_hidden, _ptr(pts), N,
                                       float(radius), float(density_bias), flags, _ptr(out["density"]),
                                       _ptr(out["features"]), _ptr(out["density_act"]), _ptr(out["color"]),
                                       _stream()))
    return {k: v.view(*shape, v.shape[-1]) for k, v in out.items() if v is not None}


_t_vals_cache = {}


def ray_t_vals(n_samples, device):
    """torch.linspace(0, 1, S + 1) made on the host (nerf_renderer.py:109-111), uploaded once per (S, device): the fp32
    roundings of this table are part of the parity contract, like grid_axis_coords for the lattice."""
    key = (int(n_samples), str(device))
    t = _t_vals_cache.get(key)
    if t is None:
        t = _t_vals_cache[key] = torch.linspace(0, 1, int(n_samples) + 1).to(device)
    return t


def _ray_args(who, planes, rays_o, rays_d, n_samples):
    """What the two ray front-ends check and flatten -> (ChannelLastPlanes, the rays' leading shape, rays_o [N,3], rays_d [N,3], S)."""
    if tuple(rays_o.shape) != tuple(rays_d.shape) or rays_o.shape[-1] != 3:
        raise SculptError("%s: rays_o %s and rays_d %s must both be [..., 3]" % (who, tuple(rays_o.shape), tuple(rays_d.shape)))
    S = int(n_samples)
    if S < 1:
        raise SculptError("%s: n_samples must be at least 1" % who)
    if not isinstance(planes, ChannelLastPlanes):
        planes = ChannelLastPlanes(planes)
    ro = _req(rays_o.reshape(-1, 3).contiguous(), torch.float32, "rays_o")
    rd = _req(rays_d.reshape(-1, 3).contiguous(), torch.float32, "rays_d")
    return planes, tuple(rays_o.shape[:-1]), ro, rd, S


def render_rays(planes, mlp, rays_o, rays_d, radius=0.87, density_bias=-1.0, n_samples=128, want=()):
    """TriplaneNeRFRenderer._forward (nerf_renderer.py:93-152) for one scene code in one launch (sculpt_render_rays).
    planes: [3,C,H,W] (converted to channel-last here, once) or a ChannelLastPlanes; rays_o / rays_d: [..., 3] world rays.
    Returns (comp_rgb [..., 3], extras) with extras[k] for k in want: "opacity" [...], "z_vals" [..., S], "weights" [..., S]."""
    unknown = set(want) - {"opacity", "z_vals", "weights"}
    if unknown:
        raise SculptError("render_rays: unknown output %s" % sorted(unknown))
    planes, shape, ro, rd, S = _ray_args("render_rays", planes, rays_o, rays_d, n_samples)
    N, dev = ro.shape[0], ro.device
    rgb = torch.empty((N, 3), dtype=torch.float32, device=dev)
    out = {k: torch.empty((N,) + w, dtype=torch.float32, device=dev) if k in want else None
           for k, w in (("opacity", ()), ("z_vals", (S,)), ("weights", (S,)))}
    check(lib.sculpt_render_rays(_ptr(planes.data), planes.C, planes.H, planes.W, _ptr(mlp.blob), mlp.n_hidden, _ptr(ro), _ptr(rd),
                                 N, float(radius), float(density_bias), _ptr(ray_t_vals(S, dev)), S, _ptr(rgb),
                                 _ptr(out["opacity"]), _ptr(out["z_vals"]), _ptr(out["weights"]), _stream()))
    return rgb.view(*shape, 3), {k: v.view(*shape, *v.shape[1:]) for k, v in out.items() if v is not None}


_RENDER_PASSES = (("opacity", ()), ("z_vals", None), ("weights", None), ("depth_sum", ()), ("normal_sum", (3,)), ("premul", (3,)))


def render_passes(planes, mlp, rays_o, rays_d, radius=0.87, density_bias=-1.0, n_samples=128, want=()):
    """render_rays with passes beside the colour picture (sculpt_render_passes): raw per-ray sums over the samples, with the
    weights of the colour picture, exactly 0 for a ray that misses the box.  Arguments and the first return value as render_rays.
    extras[k] for k in want: "opacity" [...], "z_vals" [..., S], "weights" [..., S] (render_rays' own bits, whatever else is asked),
    "depth_sum" [...] = sum w z, "premul" [..., 3] = sum w color (comp_rgb = premul + (1 - opacity)), "normal_sum" [..., 3] =
    sum w n with n = field_normals' `normal` at the sample points.  tsr/passes.py turns the sums into depth, normal and rgba.
    Still one launch; with "normal_sum" it is the forward-mode kernel (the field's gradient at every sample, about 4.5 x the time
    of the colour kernel), without it the colour kernel at its own price.  Nothing per sample is written unless asked for."""
    names = [k for k, _ in _RENDER_PASSES]
    unknown = set(want) - set(names)
    if unknown:
        raise SculptError("render_passes: unknown output %s" % sorted(unknown))
    planes, shape, ro, rd, S = _ray_args("render_passes", planes, rays_o, rays_d, n_samples)
    N, dev = ro.shape[0], ro.device
    rgb = torch.empty((N, 3), dtype=torch.float32, device=dev)
    out = {k: torch.empty((N,) + ((S,) if w is None else w), dtype=torch.float32, device=dev) if k in want else None
           for k, w in _RENDER_PASSES}
    check(lib.sculpt_render_passes(_ptr(planes.data), planes.C, planes.H, planes.W, _ptr(mlp.blob), mlp.n_hidden, _ptr(ro), _ptr(rd),
                                   N, float(radius), float(density_bias), _ptr(ray_t_vals(S, dev)), S, _ptr(rgb),
                                   *[_ptr(out[k]) for k in names], _stream()))
    return rgb.view(*shape, 3), {k: v.view(*shape, *v.shape[1:]) for k, v in out.items() if v is not None}


def field_normals(planes, mlp, points, radius=0.87, align_corners=False, want=("normal",)):
    """Gradient of the raw density with respect to the point, and the outward unit normal -grad / |grad| of the density's
    iso-surface through it (sculpt_triplane_density_grad: forward mode through the point query's own sample + MLP, one launch).
    planes: [3,C,H,W] (converted to channel-last here, once) or a ChannelLastPlanes; points: [..., 3].
    Returns a dict with the keys of `want`: "normal" [..., 3] (exactly 0 where the gradient is 0 or not finite), "grad" [..., 3],
    "density" [..., 1] (triplane_query's `density` from channel-last planes, bit for bit)."""
    want = tuple(want)
    unknown = set(want) - {"normal", "grad", "density"}
    if unknown:
        raise SculptError("field_normals: unknown output %s" % sorted(unknown))
    if not want:
        raise SculptError("field_normals: want is empty (any of normal, grad, density)")
    if points.shape[-1] != 3:
        raise SculptError("field_normals: points %s must be [..., 3]" % (tuple(points.shape),))
    if not isinstance(planes, ChannelLastPlanes):
        planes = ChannelLastPlanes(planes)
    shape = tuple(points.shape[:-1])
    pts = _req(points.reshape(-1, 3).contiguous(), torch.float32, "points")
    N = pts.shape[0]
    out = {k: torch.empty((N, w), dtype=torch.float32, device=pts.device) if k in want else None
           for k, w in (("grad", 3), ("normal", 3), ("density", 1))}
    check(lib.sculpt_triplane_density_grad(_ptr(planes.data), planes.C, planes.H, planes.W, _ptr(mlp.blob), mlp.n_hidden, _ptr(pts), N,
                                           float(radius), _lib.QUERY_ALIGN_CORNERS if align_corners else 0, _ptr(out["grad"]),
                                           _ptr(out["normal"]), _ptr(out["density"]), _stream()))
    return {k: v.view(*shape, v.shape[-1]) for k, v in out.items() if v is not None}


def grid_axis_coords(resolution, radius):
    """Per-axis lattice coordinate table, computed on the host exactly as the reference does:
    torch.linspace(0, 1, R) (isosurface.py:28-32) then scale_tensor(., (0,1), (-r, r))
    (system.py:177-181, utils.py:222-231).  R floats -- the lattice is separable."""
    g = torch.linspace(0, 1, resolution)
    g = (g - 0) / (1 - 0)
    return g * (radius - (-radius)) + (-radius)


_ws_cache = {}


def _workspace(key, nbytes, device):
    t = _ws_cache.get(key)
    if t is None or t.numel() < nbytes or t.device != device:
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _ws_cache[key] = t
    return t


_DENSITY_FLAGS = {"fp32": 0, "bf16l3": _lib.DENSITY_BF16L3}


def lattice_decode(planes, mlp, axis, radius, density_bias=0.0, out_add=0.0, want=("density_act",), align_corners=True,
                   out=None):
    """One decoder head on the full R^3 lattice point(ix, iy, iz) = (axis[ix], axis[iy], axis[iz]), flat order
    (ix*R + iy)*R + iz, through the separable layer-0 tables (sculpt_plane_features_ex + sculpt_grid_decode): what
    triplane_query + the head MLP give at those points, with the first layer's sum regrouped per plane.
    axis f32 [R] device (world coordinates exactly as the caller's positions have them); planes [3,C,H,W] channel-first.
    want: "density_act" -> f32 [R^3] = exp(row 0 + density_bias) + out_add; "features" -> f32 [R^3, 3] = rows 1..3, raw."""
    planes = _req(planes, torch.float32, "planes")
    axis = _req(axis, torch.float32, "axis")
    R = int(axis.numel())
    _, C, H, W = planes.shape
    ws = _workspace(("dg", planes.device), lib.sculpt_density_grid_workspace_bytes(R, R), planes.device)
    res = {}
    if "density_act" in want:
        res["density_act"] = out if out is not None else torch.empty(R * R * R, dtype=torch.float32, device=planes.device)
    if "features" in want:
        res["features"] = torch.empty((R * R * R, 3), dtype=torch.float32, device=planes.device)
    if not res:
        raise SculptError("lattice_decode: want must name density_act and / or features")
    flags = _lib.QUERY_ALIGN_CORNERS if align_corners else 0
    check(lib.sculpt_plane_features_ex(_ptr(planes), C, H, W, _ptr(mlp.blob), _ptr(axis), R, 0, R, float(radius), flags,
                                       _ptr(ws), _stream()))
    check(lib.sculpt_grid_decode(_ptr(mlp.blob), mlp.n_hidden, R, 0, R, float(density_bias), float(out_add), _ptr(ws),
                                 _ptr(res["density_act"]) if "density_act" in res else None,
                                 _ptr(res["features"]) if "features" in res else None, _stream()))
    return res


def density_grid(planes, mlp, resolution, radius=0.87, density_bias=-1.0, x_begin=0, x_end=None, out=None,
                 out_add=0.0, events=None, precision="fp32"):
    """density_act (+ out_add) over the lattice slab ix in [x_begin, x_end): f32 [(x_end-x_begin)*R*R]
    (TSR.extract_mesh's dense query, system.py:171-183; out_add=-threshold folds system.py:184).
    events: optional (start, stop) torch.cuda.Event pair recorded around the fused MLP launch only.
    precision: "fp32" (exact fp32 MFMA; this function's default) or "bf16l3" (three exact bf16 limbs per operand, six products,
    fp32 accumulate: fp32-equivalent, what TSR.extract_meshes uses)."""
    if precision not in _DENSITY_FLAGS:
        raise SculptError("density_grid: precision must be one of %s" % sorted(_DENSITY_FLAGS))
    planes = _req(planes, torch.float32, "planes")
    R = int(resolution)
    x_end = R if x_end is None else int(x_end)
    nx = x_end - x_begin
    _, C, H, W = planes.shape
    axis = _axis_table(R, radius, planes.device)
    ws = _workspace(("dg", planes.device), lib.sculpt_density_grid_workspace_bytes(R, nx), planes.device)
    if out is None:
        out = torch.empty(nx * R * R, dtype=torch.float32, device=planes.device)
    check(lib.sculpt_plane_features(_ptr(planes), C, H, W, _ptr(mlp.blob), _ptr(axis), R, int(x_begin), x_end,
                                    float(radius), _ptr(ws), _stream()))
    if events is not None:
        events[0].record()
    check(lib.sculpt_density_grid_ex(_ptr(mlp.blob), mlp.n_hidden, R, int(x_begin), x_end, float(density_bias),
                                     float(out_add), _ptr(ws), _ptr(out),
                                     _DENSITY_FLAGS[precision], _stream()))
    if events is not None:
        events[1].record()
    return out


def density_grid_filtered(planes, mlp, resolution, margin, radius=0.87, density_bias=-1.0, x_begin=0, x_end=None, out=None,
                          out_add=0.0, events=None, coarse="fp16", mark_all=False, stats_host=None, passes="ABC", tables=True):
    """density_grid(precision="bf16l3") for marching cubes, filtered (sculpt_density_grid_filtered): every lattice point with one
    16-bit product per hidden layer (`coarse`: "fp16" or "bf16"; pass A), then the exact three-limb arithmetic at the points
    within `margin` (natural-log units of density_act) of the level -out_add (pass B: every sign certain) and at the values
    marching cubes reads -- end points of sign-changing lattice edges, all corners of ambiguous cells (pass C).  Returns (volume,
    stats): the volume holds the bits of the full evaluation wherever marching cubes reads a value and a value of the right sign
    elsewhere as long as no coarse error reaches the margin; stats = device int32[FILTER_STATS_WORDS] view of the call's
    statistics (include/sculpt_hip.h; filter_stats() decodes them, filter_guard_error() is the figure to hold against the
    margin), valid once the stream has passed the call -- stats_host (a pinned int32[FILTER_STATS_WORDS] tensor) receives an
    asynchronous copy.  mark_all=True re-evaluates every point and stats[1] is the largest coarse error (calibration).
    passes / tables: timing aids -- run only the named passes ("A", "B", "C" one after the other on the same workspace give what
    "ABC" gives), skip the plane tables when an earlier call with the same arguments has left them in the workspace."""
    if coarse not in ("fp16", "bf16"):
        raise SculptError("density_grid_filtered: coarse must be 'fp16' or 'bf16'")
    planes = _req(planes, torch.float32, "planes")
    R = int(resolution)
    x_end = R if x_end is None else int(x_end)
    nx = x_end - x_begin
    _, C, H, W = planes.shape
    axis = _axis_table(R, radius, planes.device)
    ws = _workspace(("dg", planes.device), lib.sculpt_density_grid_workspace_bytes(R, nx), planes.device)
    fws = _workspace(("dgf", planes.device), lib.sculpt_density_filter_workspace_bytes(R, nx), planes.device)
    if out is None:
        out = torch.empty(nx * R * R, dtype=torch.float32, device=planes.device)
    if tables:
        check(lib.sculpt_plane_features(_ptr(planes), C, H, W, _ptr(mlp.blob), _ptr(axis), R, int(x_begin), x_end,
                                        float(radius), _ptr(ws), _stream()))
    flags = _lib.DENSITY_BF16L3 | (_lib.FILTER_COARSE_FP16 if coarse == "fp16" else 0) | (_lib.FILTER_MARK_ALL if mark_all else 0)
    if passes != "ABC":
        flags |= sum({"A": _lib.FILTER_PASS_A, "B": _lib.FILTER_PASS_B, "C": _lib.FILTER_PASS_C}[c] for c in passes)
    if events is not None:
        events[0].record()
    check(lib.sculpt_density_grid_filtered(_ptr(mlp.blob), mlp.n_hidden, R, int(x_begin), x_end, float(density_bias),
                                           float(out_add), float(margin), _ptr(ws), _ptr(fws), _ptr(out), flags, _stream()))
    if events is not None:
        events[1].record()
    # whose sign planes the workspace now holds (filter_sign_planes / marching_cubes check it: a probe or a slab call in between
    # rewrites them)
    gen = _filter_last.get(planes.device, (0,))[0] + 1
    _filter_last[planes.device] = (gen, R, int(x_begin), x_end, "C" in passes and not mark_all)
    stats = fws[:4 * FILTER_STATS_WORDS].view(torch.int32)
    if stats_host is not None:
        stats_host.copy_(stats, non_blocking=True)
    return out, stats


_filter_last = {}   # device -> (generation, R, x_begin, x_end, complete) of the last density_grid_filtered call


def filter_sign_planes(resolution, device, x_begin=0, x_end=None):
    """The sign planes the LAST density_grid_filtered call on this device left in the filter workspace -- which must be a call
    of these arguments: int32 [nx * R][ceil(R / 32)], bit iz % 32 of word iz / 32 = (final volume value > 0), what
    marching_cubes(sign_planes=) takes for level 0.  A view, stamped with the call's generation: marching_cubes refuses it once
    another filtered call (a calibration probe, a slab) has rewritten the workspace."""
    R = int(resolution)
    x_end = R if x_end is None else int(x_end)
    nx = x_end - int(x_begin)
    fws = _ws_cache.get(("dgf", device))
    last = _filter_last.get(device)
    if fws is None or last is None or last[1:] != (R, int(x_begin), x_end, True):
        raise SculptError("filter_sign_planes: the last filtered density grid on %s was not a complete call of R=%d, x in [%d, %d)"
                          % (device, R, int(x_begin), x_end))
    off, nzb = int(lib.sculpt_density_filter_sign_offset(R, nx)), (R + 31) // 32
    view = fws[off:off + nx * R * nzb * 4].view(torch.int32).view(nx * R, nzb)
    view._sculpt_filter_generation = last[0]
    return view


def _check_sign_planes_current(sign_planes):
    gen = getattr(sign_planes, "_sculpt_filter_generation", None)
    if gen is not None and _filter_last.get(sign_planes.device, (None,))[0] != gen:
        raise SculptError("marching_cubes: these sign planes are a view of the filter workspace, and a later "
                          "density_grid_filtered call on %s has rewritten it" % sign_planes.device)


FILTER_STATS_WORDS = 12   # SCULPT_FILTER_STATS_WORDS


def filter_stats(stats):
    """int32[FILTER_STATS_WORDS] statistics of density_grid_filtered (host or device tensor; a device tensor is read back
    here) -> dict.  max_err: largest coarse error over every re-evaluated point (inf: an unmarked point's sign was wrong, or a
    NaN); audit_err: the same over the audit sample of otherwise untouched points; n_mismatch: unmarked points with a wrong
    coarse sign; n_sign_fixed: marked points whose sign pass B corrected (what the margin is for)."""
    s = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    return {"n_refined": int(s[0]), "max_err": float(s[1:2].view(np.float32)[0]), "n_marked": int(s[2]),
            "n_nonfinite": int(s[3]), "n_cells": int(s[4]), "n_points": int(s[5]), "n_first": int(s[6]), "n_second": int(s[7]),
            "audit_err": float(s[8:9].view(np.float32)[0]), "n_audit": int(s[9]), "n_mismatch": int(s[10]),
            "n_sign_fixed": int(s[11])}


def filter_guard_error(st):
    """The one figure of a filter_stats dict the run-time guard holds against the margin: the largest coarse error the call saw
    anywhere -- re-evaluated points and audit sample -- and inf when any unmarked sign was wrong."""
    if st["n_mismatch"]:
        return float("inf")
    return max(st["max_err"], st["audit_err"])


_axis_cache = {}


def _axis_table(R, radius, device):
    key = (R, float(radius), device)
    if key not in _axis_cache:
        _axis_cache[key] = grid_axis_coords(R, radius).to(device)
    return _axis_cache[key]


# ----------------------------------------------------------------------------------------------
# marching cubes
# ----------------------------------------------------------------------------------------------
def marching_cubes(vol, level=0.0, reference_order=False, vert_div=1.0, vert_mul=1.0, vert_add=0.0,
                   use_classic=False, slab=None, sign_planes=None):
    """skimage.measure.marching_cubes(vol, level) on the GPU.

    reference_order=False: (verts f32[nv,3] voxel units, faces i32[nf,3]) exactly as skimage returns.
    reference_order=True : faces int64 with columns [1,0,2] and verts/(vert_div)*vert_mul+vert_add
                           (MarchingCubeHelper.forward + scale_tensor, isosurface.py:49-53, system.py:185-189).
    Raises ValueError / RuntimeError like skimage for an out-of-range level / empty surface.
    slab=dict(axis0_offset=int, halo_low=bool): slab mode for the axis-0 split (sculptmate_amd/slab.py);
        returns (verts, faces, top_plane_map int32[2,n1,n2], (min, max)) and never raises on an empty slab.
    sign_planes (uint32 / int32 [n0*n1][words >= ceil(n2/32)], bit i2%32 of word i2/32 = vol > level, bits past n2 zero; not in
        slab mode): the count phase takes the signs from them and reads the volume only where a cell is active
        (sculpt_mc_count_launch_signed) -- what density_grid_filtered leaves behind for level 0.  Same mesh; an empty result is
        re-run without the planes so that skimage's two errors stay apart.
    """
    vol = _req(vol, torch.float32, "vol")
    assert vol.dim() == 3
    n0, n1, n2 = vol.shape
    # The workspace holds 8 bytes per ACTIVE cell in a record pool (default: one active cell per 8 cells).  A shape whose count
    # phase ran out of pool once (SCULPT_ERR_MC_WORKSPACE: a noisy volume) keeps a larger capacity.
    rec_cap = _MC_REC_CAPACITY.get((vol.device, n0, n1, n2), 0)
    ws = _workspace(("mc", vol.device), lib.sculpt_mc_workspace_bytes_for(n0, n1, n2, rec_cap), vol.device)
    flags = 0
    if reference_order:
        flags |= _lib.MC_REFERENCE_ORDER | _lib.MC_FACES_I64
    if use_classic:
        flags |= _lib.MC_USE_CLASSIC
    off = 0
    if slab is not None:
        flags |= _lib.MC_SLAB
        if slab.get("halo_low"):
            flags |= _lib.MC_SLAB_HALO_LOW
        off = int(slab.get("axis0_offset", 0))
    nv, nf = ctypes.c_int64(), ctypes.c_int64()
    mm = (ctypes.c_float * 2)()
    fdt = torch.int64 if reference_order else torch.int32
    # Speculative emit: a call of a shape / flag combination seen before sizes its outputs by the largest mesh so far + 25 % and
    # queues count AND emit before it reads the counts back, so the stream does not idle through the host's read-allocate-launch
    # round trip; the emit kernels write nothing when the mesh does not fit, and the exact path below runs instead.
    key = (vol.device, n0, n1, n2, flags)
    cap = _MC_CAPACITY.get(key) if (slab is None and _MC_SPECULATE) else None
    verts = faces = None
    rflags = flags
    if sign_planes is not None:
        assert slab is None and sign_planes.dim() == 2 and sign_planes.shape[0] == n0 * n1 and sign_planes.stride(1) == 1
        assert sign_planes.element_size() == 4 and sign_planes.shape[1] >= (n2 + 31) // 32
        _check_sign_planes_current(sign_planes)
        rflags = flags | _lib.MC_SIGNED

    def launch_count():
        if sign_planes is not None:
            check(lib.sculpt_mc_count_launch_for(_ptr(vol), _ptr(sign_planes), sign_planes.stride(0), n0, n1, n2, float(level), rflags,
                                                 rec_cap, _ptr(ws), _stream()))
        else:
            check(lib.sculpt_mc_count_launch_for(_ptr(vol), None, 0, n0, n1, n2, float(level), flags, rec_cap, _ptr(ws), _stream()))

    launch_count()
    if cap is not None:
        verts = torch.empty((cap[0], 3), dtype=torch.float32, device=vol.device)
        faces = torch.empty((cap[1], 3), dtype=fdt, device=vol.device)
        check(lib.sculpt_mc_emit_capped(_ptr(vol), n0, n1, n2, float(level), flags, _ptr(ws), float(vert_div), float(vert_mul),
                                        float(vert_add), off, _ptr(verts), cap[0], _ptr(faces), cap[1], None, _stream()))
    nact = ctypes.c_int64()
    rc = lib.sculpt_mc_count_read_ex(n0, n1, n2, float(level), rflags, _ptr(ws), ctypes.byref(nv), ctypes.byref(nf),
                                     ctypes.cast(mm, ctypes.c_void_p), ctypes.byref(nact), _stream())
    if rc == _lib.ERR_MC_WORKSPACE:
        # more active cells than the pool holds (the speculative emit above wrote nothing).  A pool named for at least that many
        # cannot overflow (sculpt_hip.h), so the count runs once more in such a workspace; a second overflow raises (check below).
        # Later calls of the shape start with that capacity and some headroom (the cache only grows).
        rec_cap = max(int(nact.value), rec_cap)
        key_rc = (vol.device, n0, n1, n2)
        _MC_REC_CAPACITY[key_rc] = max(_MC_REC_CAPACITY.get(key_rc, 0), rec_cap + rec_cap // 4)
        ws = _workspace(("mc", vol.device), lib.sculpt_mc_workspace_bytes_for(n0, n1, n2, rec_cap), vol.device)
        cap = None
        launch_count()
        rc = lib.sculpt_mc_count_read_ex(n0, n1, n2, float(level), rflags, _ptr(ws), ctypes.byref(nv), ctypes.byref(nf),
                                         ctypes.cast(mm, ctypes.c_void_p), ctypes.byref(nact), _stream())
    if sign_planes is not None and rc == _lib.ERR_MC_EMPTY:
        # no surface: whether that is skimage's ValueError (level outside the data range) or its RuntimeError needs the range
        return marching_cubes(vol, level, reference_order, vert_div, vert_mul, vert_add, use_classic, slab)
    if rc == _lib.ERR_MC_LEVEL:
        raise ValueError(_lib.last_error())
    if rc == _lib.ERR_MC_EMPTY:
        raise RuntimeError(_lib.last_error())
    check(rc)
    if slab is None and _MC_SPECULATE:
        old = _MC_CAPACITY.get(key, (0, 0))
        _MC_CAPACITY[key] = (max(old[0], nv.value + nv.value // 4 + 1024), max(old[1], nf.value + nf.value // 4 + 1024))
    if cap is not None and nv.value <= cap[0] and nf.value <= cap[1]:
        return verts[:nv.value], faces[:nf.value]      # views of the capacity-sized buffers (fresh per call)
    verts = torch.empty((nv.value, 3), dtype=torch.float32, device=vol.device)
    faces = torch.empty((nf.value, 3), dtype=fdt, device=vol.device)
    top = torch.empty((2, n1, n2), dtype=torch.int32, device=vol.device) if slab is not None else None
    if nv.value > 0 or slab is not None:
        # dummy non-null pointers for empty outputs
        vp = verts if nv.value else torch.empty(3, device=vol.device)
        fp = faces if nf.value else torch.empty(3, dtype=faces.dtype, device=vol.device)
        check(lib.sculpt_mc_emit(_ptr(vol), n0, n1, n2, float(level), flags, _ptr(ws), float(vert_div),
                                 float(vert_mul), float(vert_add), off, _ptr(vp), _ptr(fp), _ptr(top), _stream()))
    if slab is not None:
        return verts, faces, top, (float(mm[0]), float(mm[1]))
    return verts, faces


_MC_CAPACITY = {}     # (device, n0, n1, n2, flags) -> (vertex capacity, face capacity) of the speculative emit
_MC_REC_CAPACITY = {} # (device, n0, n1, n2) -> active-cell records of the workspace once the default pool was too small
_MC_SPECULATE = not _lib.form_has("SCULPT_MC_FORM", "nospeculate")   # A/B: the two-phase path every time


ISOSURFACES = ("marching_cubes", "surface_nets")


def isosurface_rule(isosurface):
    """The extractor names TSR.extract_meshes(isosurface=...) takes; anything else is a ValueError."""
    if not isinstance(isosurface, str) or isosurface not in ISOSURFACES:
        raise ValueError("isosurface must be one of %s, got %r" % (", ".join(repr(s) for s in ISOSURFACES), isosurface))
    return isosurface


def surface_nets(vol, level=0.0, vert_div=1.0, vert_mul=1.0, vert_add=0.0, faces_i64=False, sign_planes=None):
    """Surface nets on the device (sculpt_surface_nets_*; include/sculpt_hip.h states the rule, tests/_snref.py restates it):
    one vertex inside every cell of vol f32 [n0, n1, n2] whose corners lie on both sides of `level` (inside = vol > level), one
    quad across every sign-changing lattice edge whose four cells exist -> (verts f32 [Nv, 3], quads [Nq, 4], faces [2 Nq, 3]),
    indices int32 or, with faces_i64, int64.  verts are the lattice-unit positions through marching_cubes' affine map
    (/ vert_div, * vert_mul, + vert_add); faces[2q], faces[2q + 1] split quad q along its shorter diagonal; with a positive
    inside every quad and triangle winds counter-clockwise seen from outside.  The mesh is open where the surface meets the
    box, and a cell with an ambiguous sign pattern still has one vertex, so a noisy field gives non-manifold edges.
    sign_planes: as marching_cubes takes them (what density_grid_filtered leaves behind for level 0): the count phase then
    reads no value of the volume.  Raises RuntimeError when no cell is active; Nv > 0 with Nq == 0 is a valid result."""
    vol = _req(vol, torch.float32, "vol")
    if vol.dim() != 3:
        raise SculptError("surface_nets: vol must be [n0, n1, n2], got %s" % (tuple(vol.shape),))
    n0, n1, n2 = vol.shape
    nbytes = lib.sculpt_surface_nets_workspace_bytes(n0, n1, n2)
    if nbytes == 0:
        raise SculptError(_lib.last_error(), 2)
    ws = _workspace(("sn", vol.device), nbytes, vol.device)
    planes, ld = None, 0
    if sign_planes is not None:
        if not (isinstance(sign_planes, torch.Tensor) and sign_planes.device == vol.device and sign_planes.dim() == 2
                and sign_planes.shape[0] == n0 * n1 and sign_planes.stride(1) == 1 and sign_planes.element_size() == 4
                and not sign_planes.dtype.is_floating_point and sign_planes.shape[1] >= (n2 + 31) // 32):
            raise SculptError("surface_nets: sign_planes must be int32 / uint32 [n0 * n1][>= ceil(n2 / 32)] on the volume's device")
        _check_sign_planes_current(sign_planes)
        planes, ld = sign_planes, sign_planes.stride(0)
    flags = _lib.SN_INDEX_I64 if faces_i64 else 0
    nv, nq = ctypes.c_int64(), ctypes.c_int64()
    rc = lib.sculpt_surface_nets_count(_ptr(vol), _ptr(planes), ld, n0, n1, n2, float(level), flags, _ptr(ws), ctypes.byref(nv),
                                       ctypes.byref(nq), _stream())
    if rc == _lib.ERR_SN_EMPTY:
        raise RuntimeError(_lib.last_error())
    check(rc)
    idt = torch.int64 if faces_i64 else torch.int32
    verts = torch.empty((nv.value, 3), dtype=torch.float32, device=vol.device)
    quads = torch.empty((nq.value, 4), dtype=idt, device=vol.device)
    faces = torch.empty((2 * nq.value, 3), dtype=idt, device=vol.device)
    check(lib.sculpt_surface_nets_emit(_ptr(vol), n0, n1, n2, float(level), flags, _ptr(ws), float(vert_div), float(vert_mul),
                                       float(vert_add), _ptr(verts), _ptr(quads) if nq.value else None,
                                       _ptr(faces) if nq.value else None, _stream()))
    return verts, quads, faces


def _is_count(n, lo, hi=math.inf):
    """n is an integer in lo .. hi and no bool: what the rules below ask of a count."""
    return not isinstance(n, (bool, np.bool_)) and isinstance(n, numbers.Integral) and lo <= int(n) <= hi


def _is_real(x):
    """x is a real number and no bool."""
    return not isinstance(x, (bool, np.bool_)) and isinstance(x, numbers.Real)


# ----------------------------------------------------------------------------------------------
# connected components of a mesh (csrc/mesh_components.hip)
# ----------------------------------------------------------------------------------------------
def keep_rule(keep):
    """`keep` of mesh_keep_components -> (rule, min_faces, fraction) of sculpt_mesh_components_launch: "largest", an int >= 1
    (at least that many faces) or a float in (0, 1) (at least that fraction of the largest component's faces).  Anything else,
    bool included, is a ValueError -- raised here, before anything is launched."""
    if isinstance(keep, str):
        if keep == "largest":
            return _lib.CC_KEEP_LARGEST, 0, 0.0
    elif _is_count(keep, 1):
        return _lib.CC_KEEP_MIN_FACES, int(keep), 0.0
    elif _is_real(keep) and 0.0 < float(keep) < 1.0:
        return _lib.CC_KEEP_FRACTION, 0, float(keep)
    raise ValueError("keep must be 'largest', an int >= 1 (minimum faces) or a float in (0, 1) (fraction of the largest "
                     "component), got %r" % (keep,))


def _cc_faces(faces, n_vertices):
    if not (isinstance(faces, torch.Tensor) and faces.is_cuda):
        raise SculptError("faces must be a CUDA/HIP tensor (no CPU fallback)")
    if faces.dtype not in (torch.int32, torch.int64) or faces.dim() != 2 or faces.shape[1] != 3:
        raise SculptError("faces must be int32 or int64 [Nf, 3], got %s %s" % (faces.dtype, tuple(faces.shape)))
    if not 0 <= int(n_vertices) < 2 ** 31 - 1 or faces.shape[0] >= 2 ** 31 - 1:
        raise SculptError("mesh components: %d vertices, %d faces (each below 2^31 - 1)" % (n_vertices, faces.shape[0]))
    return faces.contiguous()


def _cc_launch(f, nv, rule, min_faces, fraction):
    """Label + count + select + scan totals, and the one wait for the counts -> (workspace, [C, largest, root, Nv', Nf'])."""
    nf = f.shape[0]
    ws = _workspace(("cc", f.device), lib.sculpt_mesh_components_workspace_bytes(nv, nf), f.device)
    check(lib.sculpt_mesh_components_launch(_ptr(f), int(f.dtype == torch.int64), nf, nv, rule, min_faces, fraction, _ptr(ws), _stream()))
    counts = (ctypes.c_int64 * 5)()
    check(lib.sculpt_mesh_components_read(_ptr(ws), counts))
    return ws, [int(c) for c in counts]


def mesh_component_labels(faces, n_vertices):
    """labels i32 [Nv] alone (sculpt_mesh_component_labels): labels[v] = the smallest vertex index of v's component."""
    f, nv = _cc_faces(faces, n_vertices), int(n_vertices)
    if f.shape[0] == 0 or nv == 0:
        return torch.arange(nv, dtype=torch.int32, device=f.device)
    ws = _workspace(("cc", f.device), lib.sculpt_mesh_components_workspace_bytes(nv, f.shape[0]), f.device)
    labels = torch.empty(nv, dtype=torch.int32, device=f.device)
    check(lib.sculpt_mesh_component_labels(_ptr(f), int(f.dtype == torch.int64), f.shape[0], nv, _ptr(labels), _ptr(ws), _stream()))
    return labels


def mesh_components(faces, n_vertices):
    """Connected components of an indexed mesh with shared vertices (what marching_cubes returns): faces int32 / int64 [Nf, 3]
    over n_vertices vertices -> dict of int32 device tensors
        labels         [Nv]  the smallest vertex index of the vertex's component (exact; independent of the order of the faces)
        roots          [C]   every component's label, ascending -- a vertex no face names is a component with 0 faces
        face_counts    [C]   in the order of roots (a face with repeated indices counts)
        vertex_counts  [C]
    Nf == 0: nothing is launched; labels = arange(Nv) and no component is reported (none has a face)."""
    f, nv = _cc_faces(faces, n_vertices), int(n_vertices)
    dev = f.device
    if f.shape[0] == 0 or nv == 0:
        e = torch.empty(0, dtype=torch.int32, device=dev)
        return {"labels": torch.arange(nv, dtype=torch.int32, device=dev), "roots": e, "face_counts": e.clone(), "vertex_counts": e.clone()}
    ws, (C, _, _, _, _) = _cc_launch(f, nv, _lib.CC_KEEP_NONE, 0, 0.0)
    labels = torch.empty(nv, dtype=torch.int32, device=dev)
    roots, fc, vc = (torch.empty(C, dtype=torch.int32, device=dev) for _ in range(3))
    check(lib.sculpt_mesh_components_report(_ptr(ws), nv, f.shape[0], C, _ptr(labels), _ptr(roots), _ptr(fc), _ptr(vc), _stream()))
    return {"labels": labels, "roots": roots, "face_counts": fc, "vertex_counts": vc}


def mesh_keep_components(vertices, faces, keep):
    """The mesh without its small connected components ("floaters"), on the device.
    vertices f32 [Nv, 3], faces int32 / int64 [Nf, 3]; keep: "largest" (most faces; a tie goes to the smaller root), an int >= 1
    (components of at least that many faces) or a float x in (0, 1) ((double)faces >= x * (double)faces of the largest).
    -> (vertices' [Nv', 3], faces' [Nf', 3] re-indexed, in faces' dtype, vertex_index i64 [Nv'], face_index i64 [Nf']): the input
    with rows deleted, order preserved; the index lists name the input row of every output row.  Vertices no face names are
    dropped.  One wait for five integers between the two phases (sculpt_mesh_components_read), like marching_cubes."""
    rule, min_faces, fraction = keep_rule(keep)
    v = _req(vertices.contiguous() if isinstance(vertices, torch.Tensor) else vertices, torch.float32, "vertices")
    if v.dim() != 2 or v.shape[1] != 3:
        raise SculptError("vertices must be [Nv, 3], got %s" % (tuple(v.shape),))
    f, nv = _cc_faces(faces, v.shape[0]), v.shape[0]
    dev = v.device
    if f.shape[0] == 0 or nv == 0:
        return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=f.dtype, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev))
    ws, (_, _, _, knv, knf) = _cc_launch(f, nv, rule, min_faces, fraction)
    out_v = torch.empty((knv, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((knf, 3), dtype=f.dtype, device=dev)
    vi = torch.empty(knv, dtype=torch.int64, device=dev)
    fi = torch.empty(knf, dtype=torch.int64, device=dev)
    check(lib.sculpt_mesh_components_compact(_ptr(v), _ptr(f), int(f.dtype == torch.int64), f.shape[0], nv, _ptr(ws),
                                             _ptr(out_v) if knv else None, knv, _ptr(out_f) if knf else None, knf,
                                             _ptr(vi) if knv else None, _ptr(fi) if knf else None, _stream()))
    return out_v, out_f, vi, fi


# ----------------------------------------------------------------------------------------------
# mesh simplification: quadric-error edge collapse (csrc/mesh_simplify.hip, sf3d/remesh_device.py simplify_device)
# ----------------------------------------------------------------------------------------------
def simplify_rule(simplify):
    """`simplify` of mesh_simplify -> ("faces", n) for an int n >= 1 (a target face count) or ("ratio", x) for a float x in
    (0, 1) (the target is floor(x * Nf)).  Anything else, bool included, is a ValueError -- raised here, before anything is
    launched."""
    if _is_count(simplify, 1):
        return "faces", int(simplify)
    if _is_real(simplify) and 0.0 < float(simplify) < 1.0:
        return "ratio", float(simplify)
    raise ValueError("simplify must be an int >= 1 (target faces) or a float in (0, 1) (ratio of the faces), got %r" % (simplify,))


def _device_mesh(vertices, faces, who):
    """What mesh_simplify and mesh_smooth ask of their tensors: device tensors, float [Nv, 3] and int32 / int64 [Nf, 3]."""
    for t, name in ((vertices, "vertices"), (faces, "faces")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise SculptError("%s: %s must be a CUDA/HIP tensor (no CPU fallback)" % (who, name))
    if vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.dtype.is_floating_point:
        raise SculptError("vertices must be float [Nv, 3], got %s %s" % (vertices.dtype, tuple(vertices.shape)))
    if faces.dtype not in (torch.int32, torch.int64) or faces.dim() != 2 or faces.shape[1] != 3:
        raise SculptError("faces must be int32 or int64 [Nf, 3], got %s %s" % (faces.dtype, tuple(faces.shape)))


def simplify_target(simplify, n_faces):
    """The target face count of `simplify` (simplify_rule) on a mesh of n_faces faces."""
    kind, x = simplify_rule(simplify)
    return x if kind == "faces" else int(math.floor(x * int(n_faces)))


def mesh_simplify(vertices, faces, simplify):
    """The mesh reduced by quadric-error edge collapses (Garland & Heckbert; the rules of Fast-Quadric-Mesh-Simplification), on
    the device.  vertices float [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors; CPU tensors are refused); simplify: an
    int >= 1 (target faces) or a float in (0, 1) (target = floor(ratio * Nf)).
    -> (vertices' f32 [Nv', 3], faces' [Nf', 3] in faces' dtype, vertex_index i64 [Nv']).
    Contract:
      - at most `target` faces, unless a round collapses nothing (a closed component of 4 faces cannot go lower; border and
        fold-over rules can hold more): the call then returns what it reached;
      - target >= Nf: nothing is launched, the input tensors come back as they are (their dtype included) and
        vertex_index = arange(Nv);
      - surviving faces and vertices keep their relative order; orientation is kept;
      - vertex_index[i] is the input vertex that output vertex i descends from: the kept end of its collapses (it has moved:
        its position is the collapses' target point);
      - deterministic: two calls give the same bits;
      - per round the host reads back what a decimation round reads (the edge count, the round's result); the counts are in
        sf3d.remesh_device.last_stats()."""
    simplify_rule(simplify)
    from .sf3d import remesh_device as rmd

    _device_mesh(vertices, faces, "mesh_simplify")   # here too: a target already met returns before simplify_device
    nf = faces.shape[0]
    target = simplify_target(simplify, nf)
    if target >= nf:
        return vertices, faces, torch.arange(vertices.shape[0], dtype=torch.int64, device=vertices.device)
    v, f, index = rmd.simplify_device(vertices, faces, target)
    return v, f.to(faces.dtype), index


# ----------------------------------------------------------------------------------------------
# mesh smoothing: Taubin's lambda|mu filter (csrc/mesh_smooth.hip, sf3d/remesh_device.py smooth_device)
# ----------------------------------------------------------------------------------------------
SMOOTH_LAMBDA, SMOOTH_MU = 0.5, -0.53   # Taubin's customary pair: a shrink step, then a slightly larger inflate step
SMOOTH_MAX_ITERATIONS = 1000


def smooth_rule(smooth):
    """`smooth` of mesh_smooth -> (iterations, lam, mu): an int n, 1 <= n <= 1000 (n iterations with lam = 0.5, mu = -0.53), or
    a 3-tuple (n, lam, mu) with 0 < lam <= 1 and either mu == 0 (plain Laplacian smoothing: it shrinks) or -1 <= mu < -lam
    (Taubin's pass-band condition).  Anything else -- bool, str, a bare float, NaN, another length -- is a ValueError, raised
    here, before anything is launched."""
    if _is_count(smooth, 1, SMOOTH_MAX_ITERATIONS):
        return int(smooth), SMOOTH_LAMBDA, SMOOTH_MU
    if (isinstance(smooth, tuple) and len(smooth) == 3 and _is_count(smooth[0], 1, SMOOTH_MAX_ITERATIONS)
            and _is_real(smooth[1]) and _is_real(smooth[2])):
        lam, mu = float(smooth[1]), float(smooth[2])
        if 0.0 < lam <= 1.0 and (mu == 0.0 or -1.0 <= mu < -lam):   # a NaN fails every comparison
            return int(smooth[0]), lam, mu
    raise ValueError("smooth must be an int in 1 .. %d (iterations) or (iterations, lam, mu) with 0 < lam <= 1 and mu == 0 or "
                     "-1 <= mu < -lam, got %r" % (SMOOTH_MAX_ITERATIONS, smooth))


def mesh_smooth(vertices, faces, smooth):
    """The vertices of the mesh after Taubin's lambda|mu filter, on the device: per iteration every vertex moves by lam towards
    the centroid of its distinct neighbours, then by mu (negative: away from it) -- a low-pass filter that takes out lattice
    steps and noise without the shrinkage of plain Laplacian smoothing.  vertices float [Nv, 3], faces int32 / int64 [Nf, 3]
    (device tensors; CPU tensors are refused); smooth: see smooth_rule.
    -> vertices' f32 [Nv, 3], a new tensor.  Contract:
      - the inputs are untouched; vertex and face indices mean what they meant;
      - a vertex on an edge that does not have exactly two faces (an open border, a non-manifold edge) and a vertex no face
        names keep their bits; a vertex of any valence is smoothed;
      - a face index out of range, a repeated index in a face and a non-finite position are a SculptError;
      - Nf == 0: a copy;
      - deterministic: a fixed-order gather in fp32 without contraction, two calls give the same bits
        (tests/_smoothref.py restates it bit for bit);
      - the host reads back the input check's status and the edge count of the one topology construction; the 2 x iterations
        half-steps are queued without a wait.  The counts are in sf3d.remesh_device.last_stats()."""
    n, lam, mu = smooth_rule(smooth)
    from .sf3d import remesh_device as rmd

    _device_mesh(vertices, faces, "mesh_smooth")
    return rmd.smooth_device(vertices, faces, n, lam, mu)


# ----------------------------------------------------------------------------------------------
# mesh subdivision: the Loop scheme (csrc/mesh_subdivide.hip, sf3d/remesh_device.py loop_subdivide_device)
# ----------------------------------------------------------------------------------------------
SUBDIVIDE_MAX_LEVELS = 6
SUBDIVIDE_SCHEMES = ("loop", "midpoint", "catmull_clark")


def subdivide_rule(subdivide):
    """`subdivide` of mesh_subdivide -> (levels, scheme): an int n, 1 <= n <= 6 (n levels of the Loop scheme), or a tuple
    (n, "loop" | "midpoint" | "catmull_clark").  Anything else -- bool, float, 0, 7, NaN, another string (the hyphenated
    "catmull-clark" too) or length -- is a ValueError, raised here, before anything is launched."""
    if _is_count(subdivide, 1, SUBDIVIDE_MAX_LEVELS):
        return int(subdivide), "loop"
    if (isinstance(subdivide, tuple) and len(subdivide) == 2 and _is_count(subdivide[0], 1, SUBDIVIDE_MAX_LEVELS)
            and isinstance(subdivide[1], str) and subdivide[1] in SUBDIVIDE_SCHEMES):
        return int(subdivide[0]), subdivide[1]
    raise ValueError("subdivide must be an int in 1 .. %d (levels of the Loop scheme) or (levels, 'loop' | 'midpoint' | "
                     "'catmull_clark'), got %r" % (SUBDIVIDE_MAX_LEVELS, subdivide))


def mesh_subdivide(vertices, faces, subdivide, attributes=None):
    """The mesh refined 1 -> 4 faces per level, on the device: a subdivision surface of the input taken as a control cage (the
    Loop scheme with Warren's weights), or its plain midpoint upsampling.  vertices float [Nv, 3], faces int32 / int64 [Nf, 3],
    attributes None or float [Nv, C] with 1 <= C <= 8 (device tensors; CPU tensors are refused); subdivide: see subdivide_rule.
    -> (vertices' f32 [Nv + Ne.., 3], faces' [4^levels Nf, 3] in faces' dtype, attributes' f32 [.., C] or None), new tensors.
    Contract, per level:
      - faces and numbering are those of sf3d.remesh_device.subdivide_device: the old vertices keep their indices, the vertex
        of an edge gets Nv + (rank of the edge's first appearance over the half-edges) - 1, and face (a, b, c) becomes
        (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca) at rows 4 f .. 4 f + 3; orientation is kept;
      - an edge is interior with two faces, a border edge with one, non-manifold with three or more; every component below is
        computed in fp64 from the fp32 values with exactly the operations written, and rounded once to fp32;
      - the new vertex of an interior edge {u, v} whose two faces have the third vertices a, b:
        0.375 * (P[u] + P[v]) + 0.125 * (P[a] + P[b]); of a border or non-manifold edge: the midpoint 0.5 * (P[u] + P[v]);
      - an old vertex u with n corners in the faces: no face, a non-manifold edge at u, or a number of border edges at u that
        is neither 0 nor 2 (a corner) -- it keeps its bits; exactly two border edges, with other ends a, b (a crease) --
        0.75 * P[u] + 0.125 * (P[a] + P[b]); otherwise beta = 0.1875 for n == 3, else 3.0 / (8.0 * n), S = the sum over the
        faces around u in face order of the face's next and then its last vertex after u (every neighbour enters twice), and
        (1.0 - n * beta) * P[u] + (0.5 * beta) * S.  A vertex of any valence follows these rules;
      - attributes go through the same masks, so values in [0, 1] stay there up to one ulp;
      - scheme "midpoint": subdivide_device itself -- every new vertex the fp32 midpoint, old vertices unmoved, attributes
        refined the same way (linearly);
      - scheme "catmull_clark": (vertices', triangles', attributes') of mesh_catmull_clark on the triangles given -- another
        rule, numbering and face count (6 x 4^(levels - 1) triangles per face); call mesh_catmull_clark for the quads;
      - the inputs are untouched; a face index out of range, a repeated index in a face and a non-finite position are a
        SculptError, and so is a level whose 3 x faces would leave int32;
      - Nf == 0: copies;
      - deterministic: integer atomics for the classification, a fixed-order gather in fp64 without contraction for the
        values; two calls give the same bits (tests/_loopref.py restates it bit for bit);
      - per level the host reads back the edge count of the level's one topology construction, and before the first level the
        input check's status.  The counts are in sf3d.remesh_device.last_stats()."""
    levels, scheme = subdivide_rule(subdivide)
    from .sf3d import remesh_device as rmd

    _device_mesh(vertices, faces, "mesh_subdivide")
    if scheme == "catmull_clark":
        v, _, t, a = mesh_catmull_clark(vertices, faces, levels, attributes)
        return v, t, a
    if scheme == "loop":
        v, f, a = rmd.loop_subdivide_device(vertices, faces, levels, attributes)
        return v, f.to(faces.dtype), a
    rmd._inputs(vertices, faces, "mesh_subdivide")   # the input check of the Loop route; subdivide_device itself skips it
    a = rmd._attributes(attributes, vertices.shape[0], "mesh_subdivide")
    if faces.shape[0] == 0:
        levels = 0
    v, f = rmd.subdivide_device(vertices, faces, levels)
    if a is not None and levels:
        # the fp32 midpoint of three columns at a time is the linear refinement of those columns
        cols = [torch.nn.functional.pad(a[:, c:c + 3], (0, max(0, c + 3 - a.shape[1]))) for c in range(0, a.shape[1], 3)]
        a = torch.cat([rmd.subdivide_device(x, faces, levels)[0] for x in cols], 1)[:, :a.shape[1]].contiguous()
    return v, f.to(faces.dtype), a


def mesh_catmull_clark(vertices, faces, levels, attributes=None):
    """Catmull-Clark subdivision on the device: the mesh of triangles or of quads taken as a control cage and refined into an
    ALL-QUAD mesh, the scheme of Blender's Subdivision Surface and Multires modifiers (csrc/mesh_catmull.hip).
    vertices float [Nv, 3], faces int32 / int64 [Nf, 3] or [Nf, 4] (one width per call; only the first level can see
    triangles), levels 1 .. 6, attributes None or float [Nv, C] with 1 <= C <= 8 (device tensors; CPU tensors are refused).
    -> (vertices' f32, quads' [.., 4] and triangles' [.., 3] in faces' dtype, attributes' f32 or None), new tensors.  Contract,
    per level on faces of k corners (include/sculpt_hip.h states the rule operation for operation):
      - old vertices keep their indices, the face point of f is Nv + f, the edge point of edge e -- e its rank by first
        appearance over the half-edges k f + c -- is Nv + Nf + e; corner c of face f becomes quad k f + c = (F[f, c], edge point
        of half-edge (f, c), face point, edge point of half-edge (f, c - 1)); orientation is kept; Nv' = Nv + Nf + Ne,
        Nq' = k Nf: a triangle becomes three quads, a quad four;
      - an edge is interior with two faces, a border edge with one, non-manifold with three or more; every component is
        computed in fp64 from the fp32 values with exactly the operations written, left to right, and rounded once to fp32
        (a face point inside another rule is its unrounded fp64 value);
      - face point: (((P[c0] + P[c1]) + P[c2]) [+ P[c3]]) / k;  edge point of an interior edge {u, v} with faces f0, f1:
        0.25 * ((P[u] + P[v]) + (Fp(f0) + Fp(f1))), of a border or non-manifold edge: 0.5 * (P[u] + P[v]);
      - an old vertex u with n corners in the faces: no face, a non-manifold edge at u, or a number of border edges at u that
        is neither 0 nor 2 (a corner) -- it keeps its bits; exactly two border edges with other ends a < b (a crease) --
        0.75 * P[u] + 0.125 * (P[a] + P[b]); otherwise ((n - 2.0) * P[u] + (0.5 * SN + SQ) / n) / n, SN the sum over u's corners
        in ascending order of the face's next and then its last vertex around u (every neighbour enters twice, so the result
        does not depend on how the faces wind), SQ the sum of their face points.  A vertex of any valence follows these rules;
      - attributes go through the same masks;
      - triangles' rows 2 q, 2 q + 1 split quad q along its shorter diagonal, the rule of ops.surface_nets on the refined fp32
        positions: d13 < d02 gives (q0, q1, q3), (q1, q2, q3), otherwise (a tie included) (q0, q1, q2), (q0, q2, q3);
      - the inputs are untouched; a CPU tensor, a face index out of range, a repeated index in a face, a non-finite position,
        another face width and a level whose 4 x quads would leave int32 are a SculptError;
      - Nf == 0: copies, empty quads and empty triangles;
      - deterministic: integer atomics for the classification, a fixed-order gather in fp64 without contraction for the
        values; two calls give the same bits (tests/_catmullref.py restates it bit for bit);
      - two launches per level (classify, then one fused launch for positions, attributes, quads and triangles) behind the
        sorts; per level the host reads back the edge count of the level's one topology construction, and before the first
        level the input check's status.  The counts are in sf3d.remesh_device.last_stats()."""
    from .sf3d import remesh_device as rmd

    if not _is_count(levels, 1, SUBDIVIDE_MAX_LEVELS):
        raise SculptError("mesh_catmull_clark: levels must be an int in 1 .. %d, got %r" % (SUBDIVIDE_MAX_LEVELS, levels))
    v, q, t, a = rmd.catmull_clark_device(vertices, faces, int(levels), attributes)
    return v, q.to(faces.dtype), t.to(faces.dtype), a


# ----------------------------------------------------------------------------------------------
# distance between surfaces: area-uniform samples, closest points, Chamfer / Hausdorff / F-score (csrc/mesh_distance.hip,
# DESIGN.md 3.3e)
# ----------------------------------------------------------------------------------------------
DISTANCE_SAMPLES = 100_000


def sample_rule(n, seed):
    """(n, seed) of mesh_sample_surface -> (int n >= 0, int 0 <= seed < 2^64).  Anything else, bool included, is a ValueError --
    raised here, before anything is launched."""
    if _is_count(n, 0) and _is_count(seed, 0, 2 ** 64 - 1):
        return int(n), int(seed)
    raise ValueError("n must be an int >= 0 and seed an int in 0 .. 2^64 - 1, got n=%r, seed=%r" % (n, seed))


def _threshold_rule(threshold):
    if threshold is None:
        return None
    if _is_real(threshold) and float(threshold) > 0.0 and float(threshold) < math.inf:   # a NaN fails the comparison
        return float(threshold)
    raise ValueError("threshold must be None or a finite number > 0, got %r" % (threshold,))


def _surface(vertices, faces, who):
    """(P f32 [Nv, 3], F int32 [Nf, 3]) of a device mesh after the remesher's input check: a face index out of range and a
    non-finite vertex are a SculptError; a face that names a vertex twice passes (it is a degenerate triangle like any other)."""
    from .sf3d import remesh_device as rmd

    _device_mesh(vertices, faces, who)
    return rmd._inputs(vertices, faces, who, allow_repeated=True)


def _out(n, dev, *spec):
    """One uninitialised tensor [n, *shape] per (shape, dtype) of spec: a query's outputs, and with n == 0 its empty result."""
    return tuple(torch.empty((n,) + shape, dtype=dtype, device=dev) for shape, dtype in spec)


_CLOSEST_OUT = (((), torch.float64), ((), torch.int32), ((3,), torch.float32))      # d2, face, closest
_RAY_OUT = (((), torch.float64), ((), torch.int32), ((2,), torch.float32))          # t, face, uv
_THICKNESS_OUT = (((), torch.float32), ((), torch.float32), ((), torch.int32))      # thickness, thinnest, valid


class _SurfaceIndex:
    """The remesher's uniform grid over a surface, and the packed face records of the sorted query form (built on first use):
    one index serves the closest-point, ray and occlusion queries of a call.  Every query method is an output allocation and one
    C call whose surface arguments come from _args."""

    def __init__(self, P, F):
        from .sf3d import remesh_device as rmd

        self.P, self.F = P, F
        self.ctx = rmd._Ctx()
        self.grid = rmd._Grid(self.ctx, P, F)
        self._records = None

    def records(self):
        if self._records is None:
            self._records = torch.empty((max(self.F.shape[0], 1), 16), dtype=torch.float32, device=self.P.device)
            check(lib.sculpt_surface_pack(_ptr(self.P), _ptr(self.F), self.F.shape[0], _ptr(self._records), _stream()))
        return self._records

    def closest(self, points):
        """points f32 [N, 3] contiguous, N > 0 -> (d2 f64 [N], face int32 [N], closest f32 [N, 3])."""
        n = points.shape[0]
        out = _out(n, points.device, *_CLOSEST_OUT)
        order, surface = self._args(self._sorted(points))
        check(lib.sculpt_surface_closest(_ptr(points), n, _opt(order), *surface, *map(_ptr, out), _stream()))
        return out

    def winding(self, points):
        """points f32 [N, 3] contiguous, N > 0 -> w int32 [N, 3], the axis winding counts (csrc/mesh_winding.hip)."""
        n = points.shape[0]
        w = torch.empty((n, 3), dtype=torch.int32, device=points.device)
        order, surface = self._args(self._sorted(points), amax=False)
        check(lib.sculpt_surface_winding(_ptr(points), n, _opt(order), *surface, _ptr(w), _stream()))
        return w

    def winding_lattice(self, lo, h, n, want_counts=False):
        """The lattice of n = (n0, n1, n2) points lo + i h -> (sign planes int32 [n0 n1][ceil(n2 / 32)], counts int32
        [n0, n1, n2, 3] or None); no coordinate tensor is made.  The counts are the kernels' meeting place, 12 bytes a point,
        and are made either way."""
        dev = self.P.device
        planes = torch.empty((n[0] * n[1], (n[2] + 31) // 32), dtype=torch.int32, device=dev)
        counts = torch.empty((n[0], n[1], n[2], 3), dtype=torch.int32, device=dev)
        _, surface = self._args(amax=False)
        check(lib.sculpt_surface_winding_lattice((ctypes.c_double * 3)(*lo), float(h), n[0], n[1], n[2], *surface, _ptr(planes),
                                                 _ptr(counts), _stream()))
        return planes, counts if want_counts else None

    def _sorted(self, points=None, always=False):
        """(order, records) of the sorted query form for points f32 [N, 3] -- None: the faces themselves, by their boxes' least
        corners -- or (None, None) for the plain form (unless `always`) and for a surface without faces."""
        if (_lib.form_has("SCULPT_DISTANCE_FORM", "plain") and not always) or not self.F.shape[0]:
            return None, None
        if points is None:
            points = self.records()[:, :3].contiguous()
        n = points.shape[0]
        key = torch.empty(n, dtype=torch.int32, device=points.device)
        check(lib.sculpt_surface_cells(_ptr(points), n, self.grid.params, _ptr(key), _stream()))
        # stable: one permutation, though any would give the same results
        return torch.sort(key, stable=True).indices, self.records()

    def _grid_args(self):
        g, nf = self.grid, self.F.shape[0]
        return (_ptr(self.P) if nf else None, _ptr(self.F) if nf else None, nf), (_ptr(g.items) if nf else None,
                                                                                   _ptr(g.start) if nf else None, g.params, float(g.amax))

    def _args(self, form=None, amax=True):
        """What every C query takes of the surface -> (order, [P, F, Nf, records, items, start, params(, amax)]): the order as
        the tensor (the caller holds it until its launch is issued, and passes _opt(order)), the rest as pointers, None for
        whatever the form does not have and for every array of a surface without faces.  form: _sorted's (order, records);
        None: no order and the packed records, for the kernels that have one form and an order of their own."""
        order, records = form if form is not None else (None, self.records() if self.F.shape[0] else None)
        mesh, grid = self._grid_args()
        return order, [*mesh, _opt(records), *(grid if amax else grid[:3])]

    def ray_cast(self, origins, directions, t_min=0.0, t_max=math.inf):
        """origins, directions f32 [N, 3] contiguous, N > 0 -> (t f64 [N], face int32 [N], uv f32 [N, 2])."""
        n = origins.shape[0]
        out = _out(n, origins.device, *_RAY_OUT)
        order, surface = self._args(self._sorted(origins))   # by the cell of the origin
        check(lib.sculpt_surface_ray_cast(_ptr(origins), _ptr(directions), n, _opt(order), *surface, float(t_min), float(t_max),
                                          *map(_ptr, out), _stream()))
        return out

    def longest_side(self):
        """The longest side of the surface's bounds (0 without faces): the grid has read them back."""
        return float(self.grid.longest)

    def occlusion(self, points, normals, dirs, offset, max_distance):
        """points, normals f32 [N, 3], dirs f32 [K, 3], all contiguous on the device, N > 0 -> ao f32 [N] in ONE launch; the
        points are sorted by cell whatever SCULPT_DISTANCE_FORM says (the fused kernel has one form)."""
        n = points.shape[0]
        ao = torch.empty(n, dtype=torch.float32, device=points.device)
        order, surface = self._args(self._sorted(points, always=True))
        check(lib.sculpt_surface_occlusion(_ptr(points), _ptr(normals), n, _opt(order), _ptr(dirs), dirs.shape[0], float(offset),
                                           float(max_distance), *surface, _ptr(ao), _stream()))
        return ao

    def thickness(self, points, normals, cone_dirs, offset, max_distance, outward):
        """points, normals f32 [N, 3], cone_dirs f32 [K, 3], all contiguous on the device, N > 0 -> (thickness f32 [N], thinnest
        f32 [N], valid int32 [N]) in ONE launch (sculpt_surface_thickness); the points are always sorted by cell."""
        n = points.shape[0]
        out = _out(n, points.device, *_THICKNESS_OUT)
        order, surface = self._args(self._sorted(points, always=True))
        check(lib.sculpt_surface_thickness(_ptr(points), _ptr(normals), n, _opt(order), _ptr(cone_dirs), cone_dirs.shape[0], float(offset),
                                           float(max_distance), float(outward), *surface, *map(_ptr, out), _stream()))
        return out


def _query_points(points, who):
    if not (isinstance(points, torch.Tensor) and points.is_cuda):
        raise SculptError("%s: points must be a CUDA/HIP tensor (no CPU fallback)" % who)
    if points.dim() != 2 or points.shape[1] != 3 or not points.dtype.is_floating_point:
        raise SculptError("points must be float [N, 3], got %s %s" % (points.dtype, tuple(points.shape)))
    return points.detach().to(torch.float32).contiguous()


def _closest(index, points):
    d2, face, closest = index.closest(points) if points.shape[0] else _out(0, points.device, *_CLOSEST_OUT)
    return d2, face.long(), closest


def mesh_closest_points(points, vertices, faces):
    """The closest point of a triangle mesh to each of N query points, on the device.  points float [N, 3], vertices float
    [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors; CPU tensors are refused).
    -> (d2 f64 [N] squared distance, face i64 [N] the winning face, closest f32 [N, 3] its closest point rounded once).
    Contract (csrc/mesh_distance.hip; tests/_distref.py restates it by brute force, bit for bit):
      - positions are fp32 (other float dtypes are converted first), the arithmetic is fp64 without contraction;
      - per face f: q_f = Ericson's closest point, d2_f = |q_f - p|^2; the answer is the lexicographic minimum of (d2_f, f)
        over ALL faces whose d2_f is not NaN -- of several faces at the same distance the lowest index wins;
      - no face, or every face NaN (collinear corners can give NaN): d2 = +inf, face = -1, closest = the query;
      - a non-finite query: d2 = NaN, face = -1, closest = the query;
      - a face index out of range and a non-finite vertex are a SculptError; N == 0 launches nothing;
      - the uniform grid only accelerates; SCULPT_DISTANCE_FORM=plain selects the one-thread-per-query-in-input-order form,
        the default sorts the queries by grid cell and culls faces by their boxes: the same bits on every input;
      - the host reads back the input check's status and the grid's two small results (bounds, list length)."""
    pts = _query_points(points, "mesh_closest_points")
    P, F = _surface(vertices, faces, "mesh_closest_points")
    return _closest(_SurfaceIndex(P, F) if pts.shape[0] else None, pts)


def _weights(P, F):
    nf = F.shape[0]
    w = torch.zeros(nf, dtype=torch.int64, device=P.device)
    if nf:
        area2 = torch.empty(nf, dtype=torch.float64, device=P.device)
        mbits = torch.empty(1, dtype=torch.int64, device=P.device)
        check(lib.sculpt_surface_weights(_ptr(P), _ptr(F), nf, _ptr(area2), _ptr(mbits), _ptr(w), _stream()))
    return w


def _sample(P, F, n, seed):
    dev, nf = P.device, F.shape[0]
    W = 0
    if nf:
        cdf = torch.cumsum(_weights(P, F), 0)   # int64: exact in any order
        W = int(cdf[-1].item())
    if W <= 0:
        raise SculptError("mesh_sample_surface: the mesh has no face with area to sample")
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    uv = torch.empty((n, 2), dtype=torch.float32, device=dev)
    check(lib.sculpt_surface_sample(_ptr(P), _ptr(F), nf, _ptr(cdf), n, seed, _ptr(points), _ptr(face), _ptr(uv), _stream()))
    return points, face.long(), uv


def surface_weights(vertices, faces):
    """The integer area weights mesh_sample_surface draws faces by: w i64 [Nf] (csrc/mesh_distance.hip: twice the area in fp64,
    scaled by a power of two so that the largest is at most 2^B, rounded to nearest even)."""
    return _weights(*_surface(vertices, faces, "surface_weights"))


def mesh_sample_surface(vertices, faces, n, seed=0):
    """n points distributed uniformly over the area of a triangle mesh, on the device.  vertices float [Nv, 3], faces int32 /
    int64 [Nf, 3] (device tensors); n an int >= 0, seed an int in 0 .. 2^64 - 1 (sample_rule).
    -> (points f32 [n, 3], face i64 [n], uv f32 [n, 2]): point = (a + u (b - a)) + v (c - a) of its face's corners.
    The rule is integer wherever order could matter (csrc/mesh_distance.hip header; tests/_distref.py restates it bit for bit):
    quantised area weights, their exact prefix sum, the splitmix64 stream of `seed`, three words per sample.  A face without area
    is never drawn; a mesh without any (or without faces) is a SculptError when n > 0.  n == 0 launches nothing.  One readback:
    the total weight (after the input check's status)."""
    n, seed = sample_rule(n, seed)
    _device_mesh(vertices, faces, "mesh_sample_surface")
    if n == 0:
        dev = vertices.device
        return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty((0, 2), dtype=torch.float32, device=dev))
    P, F = _surface(vertices, faces, "mesh_sample_surface")
    return _sample(P, F, n, seed)


def _one_way(d2, tau):
    d = torch.sqrt(d2)
    below = (d < tau).sum().to(torch.float64) if tau is not None else d.new_zeros(())
    return [d.mean(), torch.sqrt(d2.mean()), d.max(), below]


def mesh_distance(vertices_a, faces_a, vertices_b, faces_b, samples=DISTANCE_SAMPLES, seed=0, threshold=None):
    """How far two triangle surfaces are from each other, whatever their topology: the distances from points on A to the
    closest point of B and back.  samples: an int >= 1 -- that many area-uniform points per mesh (mesh_sample_surface with
    `seed` on A and seed + 1 mod 2^64 on B) -- or None: the meshes' own vertices (deterministic and free of sampling noise: "how
    far did this option move the surface").  threshold: None or tau > 0.
    -> dict of Python floats:
        a_to_b, b_to_a   {"mean", "rms", "max"} of d = sqrt(d2) in fp64
        chamfer          (mean a->b + mean b->a) / 2
        hausdorff        the larger max
        precision, recall, fscore   (with a threshold) the share of a->b / b->a distances below tau, and 2 P R / (P + R)
                                    (0 when P + R == 0)
    The queries are mesh_closest_points; the reductions are torch calls and one small tensor is read back."""
    tau = _threshold_rule(threshold)
    if samples is not None:
        samples, seed = sample_rule(samples, seed)
        if samples < 1:
            raise ValueError("samples must be None or an int >= 1, got %r" % (samples,))
    A = _surface(vertices_a, faces_a, "mesh_distance")
    B = _surface(vertices_b, faces_b, "mesh_distance")
    if samples is None:
        qa, qb = A[0], B[0]
        if qa.shape[0] == 0 or qb.shape[0] == 0:
            raise SculptError("mesh_distance: a mesh without vertices has no distance")
    else:
        qa = _sample(A[0], A[1], samples, seed)[0]
        qb = _sample(B[0], B[1], samples, (seed + 1) % 2 ** 64)[0]
    ab = _SurfaceIndex(*B).closest(qa)[0]
    ba = _SurfaceIndex(*A).closest(qb)[0]
    r = torch.stack(_one_way(ab, tau) + _one_way(ba, tau)).tolist()
    out = {"a_to_b": {"mean": r[0], "rms": r[1], "max": r[2]}, "b_to_a": {"mean": r[4], "rms": r[5], "max": r[6]},
           "chamfer": 0.5 * (r[0] + r[4]), "hausdorff": max(r[2], r[6])}
    if tau is not None:
        p, q = r[3] / ab.shape[0], r[7] / ba.shape[0]
        out.update(precision=p, recall=q, fscore=2.0 * p * q / (p + q) if p + q > 0 else 0.0)
    return out


# ----------------------------------------------------------------------------------------------
# inside / outside: axis winding counts, signed distance, voxel remesh (csrc/mesh_winding.hip)
# ----------------------------------------------------------------------------------------------
VOXEL_PAD = 2            # lattice cells around the bounds on every side
VOXEL_BAND_CELLS = 2     # the default width of the distance band, in cells
VOXEL_MAX_SIDE = 1024    # lattice points along a side


def _inside(w):
    """The majority vote over the three axis counts (a non-finite query's INT32_MIN marks count as outside)."""
    return ((w != 0) & (w != -2 ** 31)).sum(1) >= 2


def mesh_winding(points, vertices, faces):
    """The integer winding counts of a triangle mesh around each of N query points along the three coordinate axes, on the
    device.  points float [N, 3], vertices float [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors; CPU tensors are refused).
    -> w int32 [N, 3]: w[i, a] = the sum over ALL faces of the signed crossings of the ray from points[i] along +a.
    Contract (csrc/mesh_winding.hip states the rule; tests/_windref.py restates it by brute force, bit for bit):
      - positions are fp32 (other float dtypes are converted first), the arithmetic is fp64 without contraction;
      - a face is crossed when the three edge signs seen along the axis agree (ties broken by a symbolic perturbation that is
        antisymmetric in the edge's direction, so an edge or vertex under the ray is counted once, not twice or never) and the
        face lies strictly ahead; the box clause (the query's two other coordinates within the face's bounds) is part of the rule;
      - a closed surface wound counter-clockwise seen from outside gives +1 inside and 0 outside on every axis, an inward one -1,
        a surface traversed twice +-2; on an open surface the axes may disagree;
      - a non-finite query: INT32_MIN three times; no faces: zeros;
      - a face index out of range and a non-finite vertex are a SculptError; N == 0 launches nothing;
      - the uniform grid only accelerates; SCULPT_DISTANCE_FORM=plain selects the one-thread-per-query-in-input-order form, the
        default sorts the queries by grid cell and reads packed face records: the same integers on every input."""
    pts = _query_points(points, "mesh_winding")
    P, F = _surface(vertices, faces, "mesh_winding")
    if pts.shape[0] == 0:
        return torch.empty((0, 3), dtype=torch.int32, device=pts.device)
    return _SurfaceIndex(P, F).winding(pts)


def mesh_contains(points, vertices, faces):
    """inside bool [N]: at least two of the three counts of mesh_winding are nonzero -- the majority vote, which ignores the
    orientation of the faces and outvotes one axis whose ray leaves through a hole.  A non-finite query is outside."""
    return _inside(mesh_winding(points, vertices, faces))


def mesh_signed_distance(points, vertices, faces):
    """The signed distance of each of N query points to a triangle mesh, on the device: mesh_closest_points' result with the
    distance negated inside, from ONE surface index.  -> (sd f64 [N], face i64 [N], closest f32 [N, 3]): sd = torch.sqrt(d2),
    negated where mesh_contains holds; d2 = +inf (no face) and NaN (a non-finite query) pass through the square root."""
    pts = _query_points(points, "mesh_signed_distance")
    P, F = _surface(vertices, faces, "mesh_signed_distance")
    if pts.shape[0] == 0:
        return _closest(None, pts)
    index = _SurfaceIndex(P, F)
    d2, face, closest = _closest(index, pts)
    sd = torch.sqrt(d2)
    return torch.where(_inside(index.winding(pts)), -sd, sd), face, closest


def mesh_winding_lattice(vertices, faces, lo, h, n, want_counts=False):
    """mesh_contains at the points of a lattice, generated in the kernel (no [N, 3] tensor is made): lattice point (i0, i1, i2) of
    n = (n0, n1, n2) lies at (float)(lo_k + i_k h), the product and the sum in fp64.  -> (sign planes int32 [n0 n1][ceil(n2 / 32)]
    as marching_cubes(sign_planes=) takes them -- bit i2 % 32 of word i2 / 32, bits past n2 zero -- and, with want_counts,
    mesh_winding's counts int32 [n0, n1, n2, 3], else None).  The same integers as mesh_winding at those coordinates."""
    if not (len(lo) == 3 and len(n) == 3 and all(_is_real(x) for x in lo) and _is_real(h) and all(_is_count(k, 1, VOXEL_MAX_SIDE) for k in n)):
        raise ValueError("lo must be three numbers, h a number and n three ints in 1 .. %d, got lo=%r, h=%r, n=%r" % (VOXEL_MAX_SIDE, lo, h, n))
    P, F = _surface(vertices, faces, "mesh_winding_lattice")
    return _SurfaceIndex(P, F).winding_lattice([float(x) for x in lo], float(h), [int(k) for k in n], want_counts)


def voxel_rule(voxel_remesh):
    """`voxel_remesh` of mesh_sdf_grid / mesh_voxel_remesh -> (R, band_cells): an int R in 8 .. 1024, the number of cells along
    the longest side of the bounds, or a tuple (R, band_cells) with band_cells an int in 1 .. 16 (default 2), the width of the
    distance band on either side of the surface.  Anything else, bool included, is a ValueError -- raised here, before anything is
    launched."""
    v = voxel_remesh
    if _is_count(v, 8, 1024):
        return int(v), VOXEL_BAND_CELLS
    if isinstance(v, tuple) and len(v) == 2 and _is_count(v[0], 8, 1024) and _is_count(v[1], 1, 16):
        return int(v[0]), int(v[1])
    raise ValueError("voxel_remesh must be an int in 8 .. 1024 (cells along the longest side) or a tuple (that, band cells in "
                     "1 .. 16), got %r" % (voxel_remesh,))


def lattice_active_corners(sign_planes, n):
    """The lattice points of sign planes int32 / uint32 [n0 n1][ceil(n2 / 32)] that are a corner of a cell whose 8 bits are not
    all equal -- the points whose value marching cubes reads -- as ascending linear indices int32 [K].  One readback: K."""
    n0, n1, n2 = n
    dev = sign_planes.device
    nb = int(lib.sculpt_lattice_active_blocks(n0, n1, n2))
    if nb == 0:
        raise SculptError(_lib.last_error() or "lattice_active_corners: lattice sides must be 1 .. %d" % VOXEL_MAX_SIDE, 2)
    offsets = torch.empty(nb + 1, dtype=torch.int32, device=dev)
    check(lib.sculpt_lattice_active_corners(_ptr(sign_planes), n0, n1, n2, _ptr(offsets), None, 0, _stream()))
    k = int(offsets[-1].item())
    listed = torch.empty(k, dtype=torch.int32, device=dev)
    if k:
        check(lib.sculpt_lattice_active_corners(_ptr(sign_planes), n0, n1, n2, _ptr(offsets), _ptr(listed), k, _stream()))
    return listed


def _lattice_points(listed, lo, h, n):
    """f32 [K, 3]: the coordinates of the listed lattice points, (float)(lo_k + i_k h) with the product and the sum in fp64."""
    idx = listed.long()
    ijk = torch.stack([idx // (n[1] * n[2]), (idx // n[2]) % n[1], idx % n[2]], 1).to(torch.float64)
    return (torch.tensor(lo, dtype=torch.float64, device=listed.device) + ijk * h).to(torch.float32).contiguous()


def _voxel_lattice(index, R, who):
    """(lo [3], h, n [3]) of the lattice of R cells along the longest side of the index's surface, VOXEL_PAD cells around it."""
    if index.F.shape[0] == 0:
        raise SculptError("%s: a mesh without faces has no inside" % who)
    mn, ext = index.grid.bounds
    longest = max(ext)
    if not longest > 0.0:
        raise SculptError("%s: the mesh's bounds have no extent" % who)
    h = longest / R
    lo = [mn[k] - VOXEL_PAD * h for k in range(3)]
    n = [int(math.ceil(ext[k] / h)) + 1 + 2 * VOXEL_PAD for k in range(3)]
    if max(n) > VOXEL_MAX_SIDE:
        raise SculptError("%s: a lattice of %d x %d x %d points (at most %d a side)" % (who, n[0], n[1], n[2], VOXEL_MAX_SIDE))
    return lo, h, n


def _sdf_fill(planes, listed, d2, n, band):
    """vol f32 [n0, n1, n2] of sculpt_sdf_fill: +-band by the planes' bits, the clamped signed distance at the listed points."""
    vol = torch.empty(tuple(n), dtype=torch.float32, device=planes.device)
    k = listed.shape[0]
    check(lib.sculpt_sdf_fill(_ptr(vol), _ptr(planes), n[0], n[1], n[2], _ptr(listed) if k else None, _ptr(d2) if k else None, k,
                              float(band), _stream()))
    return vol


def _sdf_grid(P, F, R, band_cells, who):
    index = _SurfaceIndex(P, F)
    lo, h, n = _voxel_lattice(index, R, who)
    planes, _ = index.winding_lattice(lo, h, n)
    listed = lattice_active_corners(planes, n)
    d2 = index.closest(_lattice_points(listed, lo, h, n))[0] if listed.shape[0] else None
    return _sdf_fill(planes, listed, d2, n, band_cells * h), planes, listed, lo, h


def mesh_sdf_grid(vertices, faces, voxel_remesh):
    """A banded signed-distance volume of a triangle mesh over a voxel lattice, positive INSIDE, on the device.  vertices float
    [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors); voxel_remesh: voxel_rule's R or (R, band_cells).
    -> (vol f32 [n0, n1, n2], sign_planes int32 [n0 n1][ceil(n2 / 32)], lo [3] Python floats, h):
      - h = longest side of the bounds / R in fp64; two cells of padding: lo_k = min_k - 2 h, n_k = ceil(extent_k / h) + 5;
        lattice point (i0, i1, i2) lies at (float)(lo_k + i_k h);
      - sign_planes: bit i2 % 32 of word i2 / 32 = mesh_contains at that point (generated in the kernel, no coordinate tensor),
        what marching_cubes(sign_planes=) takes;
      - vol: +band / -band by the bit, band = band_cells h; at the corners of the cells the surface passes through (the only
        values marching cubes reads) the distance of mesh_closest_points, clamped to the band and signed by the bit, and never
        zero inside: (vol > 0) == bit at EVERY lattice point;
      - a mesh without faces, bounds without extent and a lattice side above 1024 points are a SculptError.
    The closest-point query runs over the listed corners only.  Readbacks: the input check's status, the grid's two small results
    and the length of the corner list."""
    R, band_cells = voxel_rule(voxel_remesh)
    P, F = _surface(vertices, faces, "mesh_sdf_grid")
    vol, planes, _, lo, h = _sdf_grid(P, F, R, band_cells, "mesh_sdf_grid")
    return vol, planes, lo, h


def mesh_voxel_remesh(vertices, faces, voxel_remesh):
    """Voxel remesh on the device: the mesh's inside, sampled on a lattice of R cells along the longest side (mesh_sdf_grid), and
    marching cubes of that volume at level 0 -- overlapping parts fuse into one surface, holes narrower than the majority vote
    can see through close, and the result is one clean surface at the lattice's resolution.
    -> (vertices f32 [Nv', 3], faces i64 [Nf', 3]): marching_cubes(vol, 0.0, reference_order=True, sign_planes=planes) in lattice
    units, then v h + lo in fp32 (the product, then the sum).  The volume is positive inside, as extract_meshes feeds marching
    cubes, so the faces wind outward.  A mesh the lattice sees no inside of raises marching cubes' RuntimeError."""
    R, band_cells = voxel_rule(voxel_remesh)
    P, F = _surface(vertices, faces, "mesh_voxel_remesh")
    vol, planes, _, lo, h = _sdf_grid(P, F, R, band_cells, "mesh_voxel_remesh")
    v, f = marching_cubes(vol, 0.0, reference_order=True, sign_planes=planes)
    h32 = torch.tensor(h, dtype=torch.float64, device=v.device).to(torch.float32)
    lo32 = torch.tensor(lo, dtype=torch.float64, device=v.device).to(torch.float32)
    return (v * h32) + lo32, f


# ----------------------------------------------------------------------------------------------
# the mesh report: edge census, area and volume, self-intersections (csrc/mesh_report.hip)
# ----------------------------------------------------------------------------------------------
SELF_MAX_PAIRS = 1 << 26   # the default bound on an emitted pair list (8 bytes a pair)


def _self_intersections(P, F, pairs, max_pairs):
    """(count, flagged faces, flag uint8 [Nf], pairs int64 [count, 2] or None) of a checked surface with Nf > 0: count, scan, ONE
    readback of the two totals, emit."""
    dev, nf = P.device, F.shape[0]
    index = _SurfaceIndex(P, F)
    order, surface = index._args(index._sorted(), amax=False)   # the faces in the order of their boxes' least corners
    surface[3:3] = [_opt(order)]                                     # these two take the order between the mesh and the records
    n = torch.empty(nf, dtype=torch.int32, device=dev)
    flag = torch.zeros(nf, dtype=torch.uint8, device=dev)
    check(lib.sculpt_surface_self_count(*surface, _ptr(n), _ptr(flag), _stream()))
    offsets = torch.zeros(nf + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(n, 0, dtype=torch.int64)
    total, flagged = torch.stack([offsets[-1], flag.sum()]).tolist()
    if not pairs:
        return total, flagged, flag, None
    if total > max_pairs:
        raise SculptError("mesh_self_intersections: %d intersecting pairs exceed max_pairs=%d" % (total, max_pairs))
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    if total:
        check(lib.sculpt_surface_self_emit(*surface, _ptr(offsets), _ptr(keys), total, _stream()))
        keys = torch.sort(keys).values
    return total, flagged, flag, torch.stack([keys >> 32, keys & 0xFFFFFFFF], 1)


def mesh_self_intersections(vertices, faces, pairs=False, max_pairs=SELF_MAX_PAIRS):
    """Which faces of a triangle mesh pass through each other, on the device.  vertices float [Nv, 3], faces int32 / int64
    [Nf, 3] (device tensors; CPU tensors are refused).
    -> {"count": the number of intersecting pairs i < j, "faces": bool [Nf] -- the face is in at least one pair, "pairs": int64
    [count, 2] in lexicographic order with pairs=True, else None}.
    Contract (csrc/mesh_report.hip states the rule; tests/_reportref.py restates it by brute force over all pairs):
      - positions are fp32 (other float dtypes are converted first), the arithmetic is fp64 without contraction;
      - orient of four vertex INDICES is 0 when two are equal, else the sign of a 3 x 3 determinant; a segment meets a closed
        triangle when its ends lie strictly on opposite sides of the plane and the three edge signs agree (zeros allowed, not
        all zero); two faces intersect when their fp32 boxes overlap (closed) and an edge of one meets the other.  Faces that
        share a vertex or an edge therefore do not count by that alone, and there is no adjacency special case;
      - coplanar overlaps are not reported; a soup that repeats positions under different indices is judged by the arithmetic
        alone; geometric truth holds where the arithmetic is exact (small-integer coordinates);
      - pairs=True with more than max_pairs pairs is a SculptError, raised before the pair list is allocated;
      - a face index out of range and a non-finite vertex are a SculptError; Nf == 0 launches nothing;
      - the uniform grid only skips pairs, and each pair is tested once; SCULPT_DISTANCE_FORM=plain selects the
        one-thread-per-face-in-input-order form, the default walks the faces in the order of their first cell and reads the
        boxes from packed records: the same integers on every input, and the same tensors on every run;
      - the host reads back the input check (the index range and the status), the grid's two small results (bounds, list
        length) and the pair total with the number of flagged faces."""
    if not (_is_count(max_pairs, 0) and isinstance(pairs, (bool, np.bool_))):
        raise ValueError("pairs must be a bool and max_pairs an int >= 0, got pairs=%r, max_pairs=%r" % (pairs, max_pairs))
    P, F = _surface(vertices, faces, "mesh_self_intersections")
    if F.shape[0] == 0:
        return {"count": 0, "faces": torch.zeros(0, dtype=torch.bool, device=P.device),
                "pairs": torch.zeros((0, 2), dtype=torch.int64, device=P.device) if pairs else None}
    total, _, flag, plist = _self_intersections(P, F, bool(pairs), int(max_pairs))
    return {"count": total, "faces": flag.bool(), "pairs": plist}


def mesh_face_measures(vertices, faces):
    """(area2 f64 [Nf], vol6 f64 [Nf]) of a device mesh: twice the area and six times the signed volume under the origin of every
    face, in fp64 on the fp32 positions (csrc/mesh_report.hip): area = sum(area2) / 2, volume = sum(vol6) / 6."""
    P, F = _surface(vertices, faces, "mesh_face_measures")
    return _face_measures(P, F, torch.zeros(1, dtype=torch.int64, device=P.device))[:2]


def _face_measures(P, F, n_degenerate):
    nf = F.shape[0]
    area2 = torch.empty(nf, dtype=torch.float64, device=P.device)
    vol6 = torch.empty(nf, dtype=torch.float64, device=P.device)
    check(lib.sculpt_mesh_face_measures(_ptr(P) if nf else None, _ptr(F) if nf else None, nf, _ptr(area2) if nf else None,
                                        _ptr(vol6) if nf else None, _ptr(n_degenerate), _stream()))
    return area2, vol6


def mesh_report(vertices, faces, self_intersections=True):
    """What a triangle mesh is, asked on the device: the figures a caller wants before sculpting, printing or choosing
    voxel_remesh=.  vertices float [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors; CPU tensors are refused).
    -> a plain dict of Python numbers and bools:
        vertices, faces          Nv, Nf
        referenced_vertices      vertices named by at least one face
        edges, border_edges, nonmanifold_edges, inconsistent_edges
                                 over the undirected edges: 1 face, >= 3 faces, exactly 2 faces that traverse it in the SAME
                                 direction (a face with a repeated index contributes its half-edges like any other)
        degenerate_faces         a repeated index, or area2 == 0
        components               connected components that have a face (ops.mesh_components' labelling)
        euler                    referenced_vertices - edges + faces
        is_watertight            faces > 0 and border_edges == 0 and nonmanifold_edges == 0
        is_winding_consistent    inconsistent_edges == 0 and nonmanifold_edges == 0
        genus                    (2 components - euler) // 2 when watertight, consistent and that is a non-negative integer, else None
        area, volume             sum |cross(b - a, c - a)| / 2 and sum det(a, b, c) / 6, per face in fp64 (csrc/mesh_report.hip),
                                 summed by torch.sum in fp64 (the order of the sum is not pinned)
        is_volume                watertight, consistent and volume > 0
      and with self_intersections=True (mesh_self_intersections' rule):
        self_intersections       the number of intersecting pairs of faces
        self_intersecting_faces  the number of faces in at least one pair
    Nf == 0 launches nothing after the input check.  Host readbacks: the input check's three (the index range's two ends and the
    status), the topology's edge count, one for the census with the degenerate count and the two sums, one for the components'
    counts, and with self_intersections the grid's two (bounds, list length) and the pair total."""
    from .sf3d import remesh_device as rmd

    P, F = _surface(vertices, faces, "mesh_report")
    nv, nf, dev = P.shape[0], F.shape[0], P.device
    r = {"vertices": nv, "faces": nf, "referenced_vertices": 0, "edges": 0, "border_edges": 0, "nonmanifold_edges": 0,
         "inconsistent_edges": 0, "degenerate_faces": 0, "components": 0}
    area2_sum = vol6_sum = 0.0
    if nf:
        topo = rmd._Topo(rmd._Ctx(), F, nv)
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        check(lib.sculpt_mesh_edge_census(topo.ref(), _ptr(counts), _stream()))
        area2, vol6 = _face_measures(P, F, counts[5:6])   # after the census, which zeroes all eight words
        sums = torch.stack([area2.sum(), vol6.sum()])
        words = torch.cat([counts, sums.view(torch.int64)]).tolist()   # ONE readback: six integers and the bits of two doubles
        (r["edges"], r["border_edges"], r["nonmanifold_edges"], r["inconsistent_edges"], r["referenced_vertices"],
         r["degenerate_faces"]) = words[:6]
        area2_sum, vol6_sum = struct.unpack("<2d", struct.pack("<2q", *words[8:10]))
        # a vertex no face names is a component of its own without a face: the others all have one
        r["components"] = _cc_launch(F, nv, _lib.CC_KEEP_NONE, 0, 0.0)[1][0] - (nv - r["referenced_vertices"])
    r["euler"] = r["referenced_vertices"] - r["edges"] + nf
    r["is_watertight"] = nf > 0 and r["border_edges"] == 0 and r["nonmanifold_edges"] == 0
    r["is_winding_consistent"] = r["inconsistent_edges"] == 0 and r["nonmanifold_edges"] == 0
    g2 = 2 * r["components"] - r["euler"]
    r["genus"] = g2 // 2 if r["is_watertight"] and r["is_winding_consistent"] and g2 >= 0 and g2 % 2 == 0 else None
    r["area"] = area2_sum / 2.0
    r["volume"] = vol6_sum / 6.0
    r["is_volume"] = bool(r["is_watertight"] and r["is_winding_consistent"] and r["volume"] > 0)
    if self_intersections:
        r["self_intersections"], r["self_intersecting_faces"] = _self_intersections(P, F, False, 0)[:2] if nf else (0, 0)
    return r


# ----------------------------------------------------------------------------------------------
# fill holes: border loops capped with fans (csrc/mesh_holes.hip)
# ----------------------------------------------------------------------------------------------
HOLES_MAX_EDGES = 2 ** 22 - 1   # the longest loop the fixed-point centroid sum cannot overflow at (csrc/fixsum.h)
_HOLES_COUNTS = ("pinched_vertices", "loops", "open_half_edges", "filled_loops", "filled_edges", "skipped_loops", "new_vertices", "new_faces")


def holes_rule(fill_holes):
    """`fill_holes` of mesh_fill_holes -> max_edges of sculpt_mesh_border_decide: True -> 0 (every loop), an int n >= 3 -> n (loops
    of at most n edges).  Anything else -- False, 0, 1, 2, a negative, a float, a bool in the int's place -- is a ValueError,
    raised here, before anything is launched."""
    if fill_holes is True:
        return 0
    if _is_count(fill_holes, 3):
        return int(fill_holes)
    raise ValueError("fill_holes must be True (every border loop) or an int >= 3 (loops of at most that many edges), got %r" % (fill_holes,))


def _holes_input(vertices, faces, attributes, who):
    from .sf3d import remesh_device as rmd

    _device_mesh(vertices, faces, who)
    P, F = rmd._inputs(vertices, faces, who)
    return P, F, rmd._attributes(attributes, P.shape[0], who)


def _holes_topology(P, F):
    """The topology of a checked mesh with Nf > 0, the border flags and the border count -> a state dict; two readbacks (the edge
    count, the border count)."""
    from .sf3d import remesh_device as rmd

    dev, nv, nf = P.device, P.shape[0], F.shape[0]
    ctx = rmd._Ctx()
    topo = rmd._Topo(ctx, F, nv)
    flag = torch.empty(3 * nf, dtype=torch.int32, device=dev)
    vout, vin, start_of = (torch.empty(nv, dtype=torch.int32, device=dev) for _ in range(3))
    check(lib.sculpt_mesh_border_mark(topo.ref(), _ptr(flag), _ptr(vout), _ptr(vin), _ptr(start_of), _stream()))
    incl = torch.cumsum(flag, 0, dtype=torch.int32)
    return dict(ctx=ctx, topo=topo, flag=flag, vout=vout, vin=vin, start_of=start_of, incl=incl, nb=int(ctx.read(incl[-1:])))


def _holes_loops(s, max_edges):
    """next, the labels, the lengths, the per-loop decision and its scans on the state of _holes_topology (nb > 0); ONE readback,
    of the eight totals -> the state, with `counts` a dict."""
    dev, nb, topo = s["flag"].device, s["nb"], s["topo"]

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)

    s.update(list=i32(nb), next=i32(nb), leader=i32(nb), length=i32(nb), flags=i32(3, nb))
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    state = torch.empty((2, nb), dtype=torch.int64, device=dev)
    check(lib.sculpt_mesh_border_next(topo.ref(), _ptr(s["flag"]), _ptr(s["incl"]), nb, _ptr(s["vout"]), _ptr(s["vin"]), _ptr(s["start_of"]),
                                      _ptr(s["list"]), _ptr(s["next"]), _ptr(counts), _stream()))
    check(lib.sculpt_mesh_border_label(_ptr(s["next"]), nb, _ptr(state[0]), _ptr(state[1]), _ptr(s["leader"]), _ptr(s["length"]), _stream()))
    emits, centre, heads = s["flags"]
    check(lib.sculpt_mesh_border_decide(_ptr(s["leader"]), _ptr(s["length"]), nb, max_edges, _ptr(emits), _ptr(centre), _ptr(heads),
                                        _ptr(counts), _stream()))
    s["scans"] = torch.cumsum(s["flags"], 1, dtype=torch.int32)
    s["ctx"].stats["readbacks"] += 1
    s["counts"] = dict(zip(_HOLES_COUNTS, counts.tolist()), border_half_edges=nb)
    return s


def _holes_fill(s, P, F, A):
    """The centroids and the new faces on the state of _holes_loops -> (vertices', faces' int32, attributes'); no readback."""
    dev, nb, topo, c = P.device, s["nb"], s["topo"], s["counts"]
    nv, nf, n_new, n_faces = P.shape[0], F.shape[0], c["new_vertices"], c["new_faces"]
    if n_faces == 0:
        return P, F, A
    channels = 0 if A is None else A.shape[1]
    emits, centre, _ = s["flags"]
    emits_incl, centre_incl, _ = s["scans"]
    Fo = torch.empty((nf + n_faces, 3), dtype=torch.int32, device=dev)
    Fo[:nf] = F
    Po, Ao = P, A
    if n_new:
        Po = torch.empty((nv + n_new, 3), dtype=torch.float32, device=dev)
        Po[:nv] = P
        if A is not None:
            Ao = torch.empty((nv + n_new, channels), dtype=torch.float32, device=dev)
            Ao[:nv] = A
        mag = torch.empty(n_new * (3 + channels), dtype=torch.int32, device=dev)
        acc = torch.empty(n_new * (3 + channels), dtype=torch.int64, device=dev)
        check(lib.sculpt_mesh_holes_centroids(topo.ref(), _ptr(P), _ptr(A) if channels else None, channels, _ptr(s["list"]),
                                              _ptr(s["leader"]), _ptr(s["length"]), _ptr(centre), _ptr(centre_incl), nb, n_new, _ptr(mag),
                                              _ptr(acc), _ptr(Po[nv:]), _ptr(Ao[nv:]) if channels else None, _stream()))
    check(lib.sculpt_mesh_holes_emit(topo.ref(), _ptr(s["list"]), _ptr(s["next"]), _ptr(s["leader"]), _ptr(s["length"]), _ptr(emits),
                                     _ptr(emits_incl), _ptr(centre), _ptr(centre_incl), nb, n_new, n_faces, _ptr(Fo[nf:]), _stream()))
    return Po, Fo, Ao


def mesh_border_loops(vertices, faces):
    """The border loops of a triangle mesh, on the device (the rule stands at the top of csrc/mesh_holes.hip; tests/_holesref.py
    restates it).  vertices float [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors; CPU tensors are refused).  Half-edge
    h = 3 f + k runs from faces[f, k] to faces[f, (k + 1) % 3]; it is a border half-edge when its undirected edge has no other.
    -> a dict:
        half_edges         int32 [Nb]  the border half-edges, ascending
        labels             int32 [Nb]  the loop of each: its leader (the loop's smallest half-edge), or -1 when it is open -- its
                                       chain of `next` reaches a vertex where the border half-edges do not go one in, one out
        leaders, lengths   int32 [L]   every loop's leader and number of edges, in ascending leader order
        border_half_edges, loops, open_half_edges, pinched_vertices    Python ints
    A face index out of range, a repeated index in a face and a non-finite position are a SculptError.  Nf == 0, or no border
    half-edge, launches nothing after the topology.  Host readbacks: the input check's three (the index range's two ends and the
    status), the topology's edge count, the border count (it sizes the lists and the doubling rounds), one tensor with the
    totals."""
    P, F, _ = _holes_input(vertices, faces, None, "mesh_border_loops")
    dev = P.device
    out = {"half_edges": torch.empty(0, dtype=torch.int32, device=dev), "border_half_edges": 0, "loops": 0, "open_half_edges": 0,
           "pinched_vertices": 0}
    out.update(labels=out["half_edges"].clone(), leaders=out["half_edges"].clone(), lengths=out["half_edges"].clone())
    if F.shape[0] == 0:
        return out
    s = _holes_topology(P, F)
    if s["nb"]:
        s = _holes_loops(s, 0)
        nb, n_loops = s["nb"], s["counts"]["loops"]
        labels = torch.empty(nb, dtype=torch.int32, device=dev)
        leaders, lengths = (torch.empty(n_loops, dtype=torch.int32, device=dev) for _ in range(2))
        check(lib.sculpt_mesh_border_loops(_ptr(s["list"]), _ptr(s["leader"]), _ptr(s["length"]), _ptr(s["scans"][2]), nb, n_loops,
                                           _ptr(labels), _ptr(leaders) if n_loops else None, _ptr(lengths) if n_loops else None, _stream()))
        out.update(half_edges=s["list"], labels=labels, leaders=leaders, lengths=lengths,
                   **{k: s["counts"][k] for k in ("border_half_edges", "loops", "open_half_edges", "pinched_vertices")})
    s["ctx"].done()
    return out


def mesh_fill_holes(vertices, faces, fill_holes=True, attributes=None):
    """The mesh with its border loops capped by fans, on the device: what trimesh's fill_holes and Blender's Clean Up > Fill Holes
    (sides=) do between "report" and "remesh".  vertices float [Nv, 3], faces int32 / int64 [Nf, 3], attributes None or float
    [Nv, C] with 1 <= C <= 8 (device tensors; CPU tensors are refused); fill_holes: True (every loop) or an int max_edges >= 3
    (holes_rule).
    -> (vertices' f32 [Nv + new_vertices, 3], faces' [Nf + new_faces, 3] in faces' dtype, attributes' f32 or None, info).
    Contract (the rule stands at the top of csrc/mesh_holes.hip; tests/_holesref.py restates it bit for bit):
      - every existing vertex and face stays exactly as it is: rows are only appended;
      - a border half-edge is the one half-edge of an edge that has no other (the census of mesh_report); a vertex where they do
        not go one in, one out is pinched (a bow-tie, inconsistent winding beside a hole), and a half-edge that touches one, or
        whose chain of `next` reaches one, is open and stays open; the others form loops;
      - a loop of n <= max_edges edges (and n <= 2^22 - 1 in any case) is filled: n >= 4 gets one new vertex, the centroid of its
        n vertices, and n faces (b, a, centroid) over its half-edges (a -> b); n == 3 gets the one face (b, a, c) from its
        smallest half-edge and no vertex.  New vertices follow in ascending order of the loops' smallest half-edges, new faces in
        ascending order of the half-edge that emits them; they traverse the border edges in the opposite direction, so the
        winding stays consistent, and every new edge ends at a new vertex, so no non-manifold edge arises;
      - the centroid is an order-independent fixed-point sum (csrc/fixsum.h) divided by n in fp64 and rounded once to fp32; the
        attributes of the new rows are the same mean over the loop's rows (a non-finite term gives NaN);
      - info: border_half_edges, loops, open_half_edges, pinched_vertices, filled_loops, filled_edges, skipped_loops,
        new_vertices, new_faces (Python ints);
      - a face index out of range, a repeated index in a face and a non-finite position are a SculptError;
      - Nf == 0, or no border half-edge: the input's values come back, and nothing is launched after the topology;
      - deterministic: integer atomics and exact integer sums only; two calls give the same bits;
      - host readbacks: the input check's three (the index range's two ends and the status), the topology's edge count, the border
        count (it sizes the lists and the doubling rounds), one tensor with the totals.
    NOT claimed: a fan is a good cap for a short or roughly planar, star-shaped loop, and nothing more.  A long loop that wraps round
    an edge or a corner of the extraction box gets a fan that cuts through the mesh: max_edges is the control, mesh_report (its
    self-intersections) the check, and mesh_voxel_remesh remains the answer for such loops."""
    max_edges = holes_rule(fill_holes)
    P, F, A = _holes_input(vertices, faces, attributes, "mesh_fill_holes")
    info = dict.fromkeys(("border_half_edges",) + _HOLES_COUNTS, 0)
    if F.shape[0]:
        s = _holes_topology(P, F)
        if s["nb"]:
            s = _holes_loops(s, max_edges)
            info.update(s["counts"])
            P, F, A = _holes_fill(s, P, F, A)
        s["ctx"].done()
    return P, F.to(faces.dtype), A, info


# ----------------------------------------------------------------------------------------------
# rays against a surface: closest hit, ambient occlusion (csrc/mesh_ray.hip)
# ----------------------------------------------------------------------------------------------
OCCLUSION_DIRECTIONS = 64          # what occlusion=True means
OCCLUSION_MAX_DIRECTIONS = 1024
OCCLUSION_OFFSET = 2.0 ** -13      # the default origin offset along the normal, in longest sides of the surface's bounds
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


def _ray_range(t_min, t_max):
    if _is_real(t_min) and _is_real(t_max) and 0.0 <= float(t_min) <= float(t_max):   # a NaN fails the comparison
        return float(t_min), float(t_max)
    raise ValueError("the ray range must satisfy 0 <= t_min <= t_max (t_max may be inf), got t_min=%r, t_max=%r" % (t_min, t_max))


def _rays(origins, directions, who):
    o, d = _query_points(origins, who), _query_points(directions, who)
    if o.shape != d.shape:
        raise SculptError("%s: origins %s and directions %s differ in shape" % (who, tuple(o.shape), tuple(d.shape)))
    return o, d


def mesh_ray_cast(origins, directions, vertices, faces, t_min=0.0, t_max=math.inf):
    """The closest face of a triangle mesh that each of N rays hits, on the device.  origins, directions float [N, 3], vertices
    float [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors; CPU tensors are refused); 0 <= t_min <= t_max, t_max may be inf
    (anything else is a ValueError before any launch).  The direction need not be a unit vector: t is in units of it.
    -> (t f64 [N], face i64 [N] the face hit, uv f32 [N, 2] its (u, v): the hit is (1 - u - v) a + u b + v c).
    Contract (csrc/mesh_ray.hip; tests/_rayref.py restates it by brute force, bit for bit):
      - positions are fp32 (other float dtypes are converted first), the arithmetic is fp64 without contraction;
      - per face: Moeller-Trumbore, two-sided, with a relative determinant test (a ray in the plane of a face misses it) and
        the box clause (the computed hit point lies within 2^-40 of the coordinates' magnitude of the face's bounding box);
        the answer is the lexicographic minimum of (t_f, f) over ALL faces that hit -- of several faces at the same t the
        lowest index wins;
      - no hit, or a zero direction: t = +inf, face = -1, uv = 0; a non-finite origin or direction: t = NaN, face = -1, uv = 0;
      - watertightness along shared edges is NOT promised: the barycentric tests are rounded per face, so a ray through an
        edge or a vertex may pass between the faces that meet there;
      - a face index out of range and a non-finite vertex are a SculptError; N == 0 launches nothing;
      - the uniform grid only accelerates; SCULPT_DISTANCE_FORM=plain selects the one-thread-per-ray-in-input-order form, the
        default sorts the rays by the grid cell of their origin and culls faces by their boxes: the same bits on every input;
      - the host reads back the input check's status and the grid's two small results (bounds, list length)."""
    t_min, t_max = _ray_range(t_min, t_max)
    o, d = _rays(origins, directions, "mesh_ray_cast")
    P, F = _surface(vertices, faces, "mesh_ray_cast")
    return _ray_cast(_SurfaceIndex(P, F) if o.shape[0] else None, o, d, t_min, t_max)


def _ray_cast(index, o, d, t_min, t_max):
    t, face, uv = index.ray_cast(o, d, t_min, t_max) if o.shape[0] else _out(0, o.device, *_RAY_OUT)
    return t, face.long(), uv


def _spiral(k, seed, z):
    """The golden-angle spiral with the heights z(i, k) of an fp64 index vector i: unit rows np.float32 [k, 3], rounded once."""
    if not (_is_count(k, 1, OCCLUSION_MAX_DIRECTIONS) and _is_count(seed, 0, 2 ** 31 - 1)):
        raise ValueError("k must be an int in 1 .. %d and seed an int in 0 .. 2^31 - 1, got k=%r, seed=%r"
                         % (OCCLUSION_MAX_DIRECTIONS, k, seed))
    i = np.arange(int(k), dtype=np.float64)
    z = z(i, float(int(k)))
    r = np.sqrt(1.0 - z * z)
    phi = i * GOLDEN_ANGLE + float(int(seed))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    return (d / np.sqrt((d * d).sum(1, keepdims=True))).astype(np.float32)


def _ray_count_rule(x, default, name, rays):
    """occlusion_rule and thickness_rule: True -> (default, None), k -> (k, None), (k, max_distance or None) -> itself."""
    if x is True or (isinstance(x, np.bool_) and bool(x)):
        return default, None
    if _is_count(x, 1, OCCLUSION_MAX_DIRECTIONS):
        return int(x), None
    if isinstance(x, tuple) and len(x) == 2 and _is_count(x[0], 1, OCCLUSION_MAX_DIRECTIONS):
        far = x[1]
        if far is None:
            return int(x[0]), None
        if _is_real(far) and float(far) > 0.0:   # a NaN fails the comparison
            return int(x[0]), float(far)
    raise ValueError("%s must be True, an int in 1 .. %d (%s) or (%s, max_distance) with max_distance > 0, got %r"
                     % (name, OCCLUSION_MAX_DIRECTIONS, rays, rays, x))


def _offset_rule(offset):
    if offset is not None and not (_is_real(offset) and math.isfinite(float(np.float32(offset)))):
        raise ValueError("offset must be None or a finite number, got %r" % (offset,))


def _far32(far):
    return math.inf if far is None else float(np.float32(far))


def occlusion_directions(k, seed=0):
    """The k directions of the ambient occlusion: the golden-angle spiral on the unit sphere, z_i = 1 - (2 i + 1) / k,
    phi_i = i x the golden angle + seed radians (`seed`, an int in 0 .. 2^31 - 1, rotates the set about z), computed on the host
    in NumPy fp64 and rounded once -> np.float32 [k, 3].  k in 1 .. 1024.  Deterministic; needs no device."""
    return _spiral(k, seed, lambda i, k: 1.0 - (2.0 * i + 1.0) / k)


def occlusion_rule(occlusion):
    """`occlusion` of the ambient occlusion -> (k, max_distance): True (64 directions, rays of any length), an int k in
    1 .. 1024 or a tuple (k, max_distance) with max_distance > 0 (inf allowed) or None (any length) -- so a rule's own result is
    a rule.  Anything else -- False, None, a str, a bare float, NaN, another length -- is a ValueError, raised here, before
    anything is launched."""
    return _ray_count_rule(occlusion, OCCLUSION_DIRECTIONS, "occlusion", "directions")


def _occlusion_rules(occlusion, offset, seed):
    """The rules of an occlusion call (ValueError, nothing launched) -> (directions np.float32 [k, 3], far)."""
    k, far = occlusion_rule(occlusion)
    _offset_rule(offset)
    return occlusion_directions(k, seed), _far32(far)      # checks the seed


def _offset32(index, offset):
    """The origin offset of a ray query rounded to fp32; None: 2^-13 of the longest side of the index's surface."""
    return float(np.float32(OCCLUSION_OFFSET * index.longest_side() if offset is None else offset))


def _point_query_args(who, points, normals, vertices, faces, dirs, offset):
    """The tensors of a query of points with normals, checked (SculptError) after the caller's rules, then the index with the
    defaults that depend on its bounds -> (index or None when N == 0, pts, nrm, dirs on the device, offset rounded to fp32)."""
    pts, nrm = _query_points(points, who), _query_points(normals, who)
    if pts.shape != nrm.shape:
        raise SculptError("%s: points %s and normals %s differ in shape" % (who, tuple(pts.shape), tuple(nrm.shape)))
    P, F = _surface(vertices, faces, who)
    if pts.shape[0] == 0:
        return None, pts, nrm, None, 0.0
    index = _SurfaceIndex(P, F)
    return index, pts, nrm, torch.from_numpy(dirs).to(pts.device), _offset32(index, offset)


def _mesh_occlusion(who, fused, points, normals, vertices, faces, occlusion, offset, seed):
    dirs, far = _occlusion_rules(occlusion, offset, seed)
    index, pts, nrm, dirs, offset = _point_query_args(who, points, normals, vertices, faces, dirs, offset)
    if index is None:
        return torch.empty(0, dtype=torch.float32, device=pts.device)
    return index.occlusion(pts, nrm, dirs, offset, far) if fused else _occlusion_composed(index, pts, nrm, dirs, offset, far)


def mesh_occlusion(points, normals, vertices, faces, occlusion=True, offset=None, seed=0):
    """The ambient occlusion of N points with normals against a triangle mesh, on the device, in ONE launch
    (sculpt_surface_occlusion): the cosine-weighted share of the directions above a point's tangent plane along which a ray
    leaves without hitting the mesh.  points, normals float [N, 3], vertices float [Nv, 3], faces int32 / int64 [Nf, 3] (device
    tensors); occlusion: True, k or (k, max_distance) (occlusion_rule); offset: how far along the normal the rays start (None:
    2^-13 of the longest side of the surface's bounds), rounded to fp32; seed rotates the direction set (occlusion_directions).
    -> ao f32 [N] in [0, 1]: 1 sees everything, 0 is fully occluded.  In fp32 without contraction, with D the directions:
    w_k = (n.x D_k.x + n.y D_k.y) + n.z D_k.z; direction k takes part iff w_k > 0; its ray runs from p + offset n over
    [0, max_distance] and is occluded iff mesh_ray_cast would report a face; ao = (sum of w_k of the free rays) / (sum of all
    taking-part w_k), both in the order of k; 1 when no direction takes part (a zero normal); NaN for a non-finite p or n.  The
    normals are used as given (not normalised: ao is a ratio).  Bit for bit what mesh_occlusion_composed computes with one
    mesh_ray_cast per direction (tests/test_gpu_mesh_ray.py).  N == 0 launches nothing."""
    return _mesh_occlusion("mesh_occlusion", True, points, normals, vertices, faces, occlusion, offset, seed)


def mesh_occlusion_composed(points, normals, vertices, faces, occlusion=True, offset=None, seed=0):
    """mesh_occlusion by the composed route: one closest-hit query of every point per direction (mesh_ray_cast's kernels on one
    shared grid) and torch reductions in the kernel's order.  The yardstick the fused kernel is tested (same bits) and timed
    against (tools/time_occlusion.py); K launches and K sorts instead of one."""
    return _mesh_occlusion("mesh_occlusion_composed", False, points, normals, vertices, faces, occlusion, offset, seed)


def _occlusion_composed(index, pts, nrm, dirs, offset, far):
    origin = pts + nrm * offset                # fp32: the product rounded, then the sum
    open_, all_ = torch.zeros_like(pts[:, 0]), torch.zeros_like(pts[:, 0])
    for k in range(dirs.shape[0]):
        d = dirs[k]
        w = (nrm[:, 0] * d[0] + nrm[:, 1] * d[1]) + nrm[:, 2] * d[2]
        part = w > 0
        face = index.ray_cast(origin, d.expand(pts.shape[0], 3).contiguous(), 0.0, far)[1]
        all_ = torch.where(part, all_ + w, all_)
        open_ = torch.where(part & (face < 0), open_ + w, open_)
    ao = torch.where(all_ == 0, torch.ones_like(all_), open_ / all_)
    bad = ~(torch.isfinite(pts).all(1) & torch.isfinite(nrm).all(1))
    return torch.where(bad, torch.full_like(ao, math.nan), ao)


# ----------------------------------------------------------------------------------------------
# ambient occlusion baked over an atlas (csrc/mesh_ray.hip sculpt_bake_occlusion)
# ----------------------------------------------------------------------------------------------
OCCLUSION_CAGE = 2.0 ** -6         # the default snap distance of a bake against a source, in longest sides of the source's bounds


def _mesh_args(who, v_pos, faces):
    """The mesh every atlas bake takes, checked: v_pos f32 [Nv, 3], faces i32 / i64 [Nf, 3], device tensors -> (v, f) contiguous."""
    v = _req(v_pos.contiguous() if isinstance(v_pos, torch.Tensor) else v_pos, torch.float32, "v_pos")
    if not (isinstance(faces, torch.Tensor) and faces.is_cuda):
        raise SculptError("faces must be a CUDA/HIP tensor (no CPU fallback)")
    if faces.dtype not in (torch.int32, torch.int64):
        raise SculptError("%s: faces must be int32 or int64, got %s" % (who, faces.dtype))
    f = faces.contiguous()
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise SculptError("%s: v_pos %s must be [Nv, 3] and faces %s [Nf, 3]" % (who, tuple(v.shape), tuple(f.shape)))
    return v, f


def _covered_texels(r, v, f):
    """The coverage of texel_position (csrc/bake_texel.h) in torch: a texel is covered when its tri is in [0, Nf) (a NaN is
    not) and the three vertex rows of that face are in [0, Nv) -> (covered bool [res, res], rast with (0, 0, 0, -1) wherever it
    is not covered, so that bake_interpolate, which guards nothing, reads through checked rows only)."""
    nv, nf = v.shape[0], f.shape[0]
    tri = r[..., 3]
    covered = (tri >= 0) & (tri < 2147483648.0)                     # a NaN fails both
    if nf == 0 or nv == 0:
        covered = torch.zeros_like(covered)
    else:
        t = torch.where(covered, tri, torch.zeros_like(tri)).to(torch.int64)
        covered = covered & (t < nf)
        rows = f[t.clamp(max=nf - 1)].to(torch.int64)               # [res, res, 3]
        covered = covered & ((rows >= 0) & (rows < nv)).all(-1)
    return covered, torch.where(covered[..., None], r, r.new_tensor([0.0, 0.0, 0.0, -1.0])).contiguous()


def _bake_occlusion_args(who, v_pos, faces, normals, rast, occlusion, offset, seed, source, cage):
    """Rules first (ValueError, nothing launched), then the tensors (SculptError), then the index over S.
    -> (index or None when res == 0, v, f, nrm, rast, dirs, offset, far, cage)."""
    dirs, far = _occlusion_rules(occlusion, offset, seed)
    _source_rule(who, source, cage)
    index, v, f, nrm, r, offset, cage = _atlas_query_args(who, v_pos, faces, normals, rast, offset, source, cage)
    return index, v, f, nrm, r, torch.from_numpy(dirs).to(v.device) if index is not None else None, offset, far, cage


def _source_rule(who, source, cage):
    """The rule of `source` / `cage` of a bake against a surface: a ValueError before anything is launched."""
    if source is None:
        if cage is not None:
            raise ValueError("%s: cage snaps the texels onto a source surface; without a source it must be None, got %r" % (who, cage))
    else:
        if not (isinstance(source, (tuple, list)) and len(source) == 2):
            raise ValueError("%s: source must be None or (vertices, faces), got %r" % (who, type(source).__name__))
        if cage is not None and not (_is_real(cage) and 0.0 < float(np.float32(cage)) < math.inf):   # a NaN fails the comparison
            raise ValueError("cage must be None or a finite number > 0, got %r" % (cage,))


def _atlas_tensors(who, v_pos, faces, normals, rast):
    """The tensors of a bake over an atlas, checked (SculptError) -> (v, f, nrm, rast), contiguous."""
    v, f = _mesh_args(who, v_pos, faces)
    nrm = _req(normals.contiguous() if isinstance(normals, torch.Tensor) else normals, torch.float32, "normals")
    r = _req(rast.contiguous() if isinstance(rast, torch.Tensor) else rast, torch.float32, "rast")
    if nrm.shape != v.shape:
        raise SculptError("%s: normals %s must be per vertex %s" % (who, tuple(nrm.shape), tuple(v.shape)))
    if r.ndim != 3 or r.shape[0] != r.shape[1] or r.shape[2] != 4:
        raise SculptError("%s: rast %s must be [res, res, 4]" % (who, tuple(r.shape)))
    return v, f, nrm, r


def _atlas_query_args(who, v_pos, faces, normals, rast, offset, source, cage):
    """The tensors of a ray bake over an atlas, checked (SculptError), and the index over S with the defaults that depend on its
    bounds -> (index or None when res == 0, v, f, nrm, rast, offset, cage), offset and cage rounded to fp32 (cage 0: no snap)."""
    v, f, nrm, r = _atlas_tensors(who, v_pos, faces, normals, rast)
    P, F = _surface(v, f, who) if source is None else _surface(source[0], source[1], who)
    if r.shape[0] == 0:
        return None, v, f, nrm, r, 0.0, 0.0
    index = _SurfaceIndex(P, F)
    if source is None:
        cage = 0.0
    elif cage is None:
        cage = OCCLUSION_CAGE * index.longest_side()
    return index, v, f, nrm, r, _offset32(index, offset), float(np.float32(cage))


def bake_occlusion(v_pos, faces, normals, rast, occlusion=True, offset=None, seed=0, source=None, cage=None):
    """The ambient occlusion of a surface S at every covered texel of a rasterised atlas of a (low-poly) mesh, in ONE launch
    (sculpt_bake_occlusion): no position or normal image, no index list, no sort.  v_pos f32 [Nv, 3], faces i32 / i64 [Nf, 3],
    normals f32 [Nv, 3] per vertex, rast f32 [res, res, 4] from bake_rasterize (device tensors; CPU tensors are refused);
    occlusion, offset, seed: as for mesh_occlusion (offset=None: 2^-13 of the longest side of S's bounds).
    source=None: S is the mesh itself, cage must be None.  source=(vertices, faces): S is that surface -- the high-poly mesh the
    low one was simplified from -- and every texel is first SNAPPED onto it: the closest hit of the ray from p + cage n towards
    p - cage n replaces p, and that face's unit normal (on n's side) replaces n; a texel whose ray hits nothing keeps (p, n).
    cage=None: 2^-6 of the longest side of S's bounds; else a finite number > 0, rounded to fp32.
    -> (ao f32 [res, res] in [0, 1], exactly 0 where not covered, NaN where the interpolated position or normal is not finite;
    mask bool [res, res], the coverage).  Per texel the rule at the top of csrc/mesh_ray.hip ("the atlas bake"): a property of
    the inputs alone, bit for bit what bake_occlusion_composed computes (tests/test_gpu_bake_occlusion.py; tests/_aomapref.py
    restates it in NumPy).  A rast row whose triangle is negative, NaN or out of range, or names a vertex out of range, is not
    covered.  res == 0 launches nothing."""
    index, v, f, nrm, r, dirs, offset, far, cage = _bake_occlusion_args("bake_occlusion", v_pos, faces, normals, rast, occlusion,
                                                                        offset, seed, source, cage)
    return _bake_occlusion_fused(index, v, f, nrm, r, dirs, offset, far, cage)


def _bake_occlusion_fused(index, v, f, nrm, r, dirs, offset, far, cage):
    res = r.shape[0]
    ao = torch.empty((res, res), dtype=torch.float32, device=r.device)
    mask = torch.empty((res, res), dtype=torch.uint8, device=r.device)
    if index is None:
        return ao, mask.view(torch.bool)
    _, surface = index._args()
    check(lib.sculpt_bake_occlusion(_ptr(r), res, _ptr(v), v.shape[0], _ptr(f), int(f.dtype == torch.int64), f.shape[0], _ptr(nrm),
                                    _ptr(dirs), dirs.shape[0], offset, far, cage, *surface, _ptr(ao), _ptr(mask), _stream()))
    return ao, mask.view(torch.bool)


def bake_occlusion_composed(v_pos, faces, normals, rast, occlusion=True, offset=None, seed=0, source=None, cage=None):
    """bake_occlusion by the pieces that were there before it: bake_interpolate of the positions and of the normals (two
    [res, res, 3] images), nonzero of the coverage, with a source one closest-hit query (mesh_ray_cast's kernels) and the snap in
    torch fp64 / fp32 elementwise operations, then the point-list occlusion kernel (a cell sort) and a scatter.  The yardstick the
    fused kernel is tested (same bits) and timed against (tools/time_occlusion_map.py)."""
    index, v, f, nrm, r, dirs, offset, far, cage = _bake_occlusion_args("bake_occlusion_composed", v_pos, faces, normals, rast,
                                                                        occlusion, offset, seed, source, cage)
    return _bake_occlusion_composed(index, v, f, nrm, r, dirs, offset, far, cage)


def _atlas_points(index, v, f, nrm, r, cage, want_face=False):
    """The composed atlas route up to its point query: the coverage in torch, nonzero, bake_interpolate of the positions and of
    the normals, the snap -> (cov bool [res, res], at i64 [M] the covered texels' flat indices, pts f32 [M, 3], nr f32 [M, 3]);
    at, pts and nr are None when nothing is covered or the index is None (res == 0).  want_face: one more value, the face of the
    index's surface every texel was snapped onto (int32 [M], -1 where the snap ray hit nothing; None when nothing was snapped)."""
    cov, clean = _covered_texels(r, v, f)
    at = torch.nonzero(cov.reshape(-1))[:, 0] if index is not None else None
    if at is None or at.numel() == 0:
        return (cov, None, None, None) + ((None,) if want_face else ())
    pts = bake_interpolate(v, clean, f).reshape(-1, 3)[at].contiguous()
    nr = bake_interpolate(nrm, clean, f).reshape(-1, 3)[at].contiguous()
    face = None
    if cage > 0.0 and index.F.shape[0]:
        pts, nr, face = _snap_composed(index, pts, nr, cage, want_face=True)
    return (cov, at, pts, nr) + ((face,) if want_face else ())


def _bake_occlusion_composed(index, v, f, nrm, r, dirs, offset, far, cage):
    res = r.shape[0]
    ao = torch.zeros(res * res, dtype=torch.float32, device=r.device)
    cov, at, pts, nr = _atlas_points(index, v, f, nrm, r, cage)
    if at is not None:
        ao[at] = index.occlusion(pts, nr, dirs, offset, far)
    return ao.view(res, res), cov


def bake_occlusion_route():
    """What TSR.bake_occlusion_map calls: bake_occlusion_composed, unless SCULPT_DISTANCE_FORM holds the token `fusedbake`
    (then bake_occlusion).  The two give the same bits; on the atlas the map is baked over -- the box-projection unwrap of a
    simplified 256^3 mesh at 2048^2, a fragmented atlas with 12 % coverage -- the composed route's global list fills every wave
    and is the faster one (tools/time_occlusion_map.py), so it is the default."""
    return bake_occlusion if _lib.form_has("SCULPT_DISTANCE_FORM", "fusedbake") else bake_occlusion_composed


def _face_cross64(P64, i0, i1, i2):
    """cross(b - a, c - a) of the corners a, b, c = P64[i0], P64[i1], P64[i2] of n faces, in fp64 -> (gx, gy, gz), each [n]: P64 f64
    [Nv, 3], i0, i1, i2 i64 [n] (the columns of F[fi]: the render has them already, so they are not gathered here a second time);
    every component is a difference of two products, each its own elementwise kernel, so nothing is contracted."""
    a, b, c = P64[i0], P64[i1], P64[i2]
    e1, e2 = b - a, c - a
    return (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
            e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])


def _snap_composed(index, pts, nr, cage, want_stats=False, want_face=False):
    """Step 4 of the atlas bake in torch: every operation is one elementwise kernel, so nothing is contracted.  want_face: the
    face every ray hit (int32 [M], -1 where it hit nothing) comes back as one more value."""
    c = nr * cage                                # fp32
    o, d = pts + c, -c
    t, face, _ = index.ray_cast(o.contiguous(), d.contiguous(), 0.0, 2.0)
    hit = face >= 0
    fi = face.clamp(min=0).long()
    q = (o.double() + t[:, None] * d.double()).float()          # a product, a sum, one rounding to fp32
    F = index.F.long()
    g = torch.stack(_face_cross64(index.P.double(), F[fi, 0], F[fi, 1], F[fi, 2]), 1)
    nd = nr.double()
    flip = ((g[:, 0] * nd[:, 0] + g[:, 1] * nd[:, 1]) + g[:, 2] * nd[:, 2]) < 0
    g = torch.where(flip[:, None], -g, g)
    ln = torch.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    good = hit & (ln > 0) & (ln < math.inf)
    m = (g / ln[:, None]).float()
    out = torch.where(hit[:, None], q, pts).contiguous(), torch.where(good[:, None], m, nr).contiguous()
    out = out + (hit,) if want_stats else out
    return out + (face,) if want_face else out


# ----------------------------------------------------------------------------------------------
# wall thickness: the shape diameter per point, the thickness map (csrc/mesh_ray.hip sculpt_surface_thickness)
# ----------------------------------------------------------------------------------------------
THICKNESS_DIRECTIONS = 32          # what thickness=True means
THICKNESS_CONE = 60.0              # the half-angle of the cone about the inward normal, in degrees


def thickness_rule(thickness):
    """`thickness` of the wall-thickness queries -> (k, max_distance): True (32 rays, of any length), an int k in 1 .. 1024 or a
    tuple (k, max_distance) with max_distance > 0 (inf allowed) or None (any length) -- so a rule's own result is a rule.
    Anything else -- False, None, a str, a bare float, NaN, another length -- is a ValueError, raised here, before anything is
    launched."""
    return _ray_count_rule(thickness, THICKNESS_DIRECTIONS, "thickness", "rays")


def thickness_directions(k, cone=THICKNESS_CONE, seed=0):
    """The k directions of the thickness cone about +z: z_i = 1 - (1 - cos(cone)) (2 i + 1) / (2 k), an area-uniform spiral over
    the spherical cap of half-angle `cone` degrees (0 < cone <= 90), phi_i = i x the golden angle + seed radians (`seed`, an int
    in 0 .. 2^31 - 1, rotates the set about z), computed on the host in NumPy fp64, the rows normalised and rounded once ->
    np.float32 [k, 3], every z in (cos(cone), 1).  k in 1 .. 1024.  Deterministic; needs no device.  The kernel turns the set
    onto each point's own inward normal."""
    def z(i, k):   # after the spiral's own check of k and seed, as ever
        if not (_is_real(cone) and 0.0 < float(cone) <= 90.0):   # a NaN fails the comparison
            raise ValueError("cone must be a half-angle in degrees with 0 < cone <= 90, got %r" % (cone,))
        return 1.0 - (1.0 - math.cos(math.radians(float(cone)))) * (2.0 * i + 1.0) / (2.0 * k)

    return _spiral(k, seed, z)


def _thickness_rules(thickness, cone, offset, seed, outward):
    """The rules of a thickness call (ValueError, nothing launched) -> (cone set np.float32 [k, 3], far, outward)."""
    k, far = thickness_rule(thickness)
    dirs = thickness_directions(k, cone, seed)      # checks the cone and the seed
    _offset_rule(offset)
    if not (_is_real(outward) and float(outward) in (1.0, -1.0)):
        raise ValueError("outward must be +1 or -1, got %r" % (outward,))
    return dirs, _far32(far), float(outward)


def _mesh_thickness(who, fused, points, normals, vertices, faces, thickness, cone, offset, seed, outward):
    dirs, far, outward = _thickness_rules(thickness, cone, offset, seed, outward)
    index, pts, nrm, dirs, offset = _point_query_args(who, points, normals, vertices, faces, dirs, offset)
    if index is None:
        return _out(0, pts.device, *_THICKNESS_OUT)
    if fused:
        return index.thickness(pts, nrm, dirs, offset, far, outward)
    return _thickness_composed(index, pts, nrm, dirs, offset, far, outward)


def mesh_thickness(points, normals, vertices, faces, thickness=True, cone=THICKNESS_CONE, offset=None, seed=0, outward=1.0):
    """The wall thickness -- the shape diameter (Shapira et al.) -- of a triangle mesh at N points with OUTWARD normals, on the
    device, in ONE launch (sculpt_surface_thickness): how far the rays of a cone about the inward normal travel before they
    leave the body.  points, normals float [N, 3], vertices float [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors; CPU
    tensors are refused); thickness: True (32 rays), k or (k, max_distance) (thickness_rule); cone: the half-angle in degrees,
    0 < cone <= 90, and seed: thickness_directions; offset: how far below the surface the rays start (None: 2^-13 of the longest
    side of the surface's bounds), rounded to fp32; outward: +1 when the faces wind counter-clockwise seen from outside, -1
    otherwise.  A bad rule is a ValueError before any launch.
    -> (thickness f32 [N], thinnest f32 [N], valid int32 [N]).  Per point (the rule at the top of csrc/mesh_ray.hip,
    "thickness"; fp32 without contraction): m = unit(n); the frame (T, B) of Duff et al. about m; o = p - offset m; for each
    cone direction C_j in order d = (C_j.x T + C_j.y B) - C_j.z m and the closest hit (t, f) of (o, d) over [0, max_distance] as
    mesh_ray_cast reports it; the hit is valid iff the ray leaves through the back of f: dot(cross(b - a, c - a), d) outward > 0
    in fp64 -- a ray that enters another body through a front face, or hits nothing, contributes nothing.  thickness = the mean
    of fp32(t) over the valid rays weighted by C_j.z, thinnest their minimum, valid their number; no valid ray: +inf, +inf, 0.
    A non-finite p or n: NaN, NaN, 0.  A zero or overflowing normal, and a surface without faces: +inf, +inf, 0.  The outlier
    rejection of the shape-diameter paper is left to the caller (thinnest and valid are there to judge by).  Bit for bit what
    mesh_thickness_composed computes with one mesh_ray_cast per direction (tests/test_gpu_mesh_thickness.py; tests/_thickref.py
    restates it in NumPy).  N == 0 launches nothing."""
    return _mesh_thickness("mesh_thickness", True, points, normals, vertices, faces, thickness, cone, offset, seed, outward)


def mesh_thickness_composed(points, normals, vertices, faces, thickness=True, cone=THICKNESS_CONE, offset=None, seed=0, outward=1.0):
    """mesh_thickness by the composed route: the per-point directions in torch in the kernel's expression order, one closest-hit
    query of every point per cone direction (mesh_ray_cast's kernels on one shared grid, each with its own sort), the back-face
    test as a torch fp64 gather and the reductions in the kernel's order.  The yardstick the fused kernel is tested (same bits)
    and timed against (tools/time_thickness.py)."""
    return _mesh_thickness("mesh_thickness_composed", False, points, normals, vertices, faces, thickness, cone, offset, seed, outward)


def _thickness_composed(index, pts, nrm, dirs, offset, far, outward):
    """Every line is one elementwise kernel, so nothing is contracted."""
    n, inf = pts.shape[0], math.inf
    bad = ~(torch.isfinite(pts).all(1) & torch.isfinite(nrm).all(1))
    m, ok = _unit3(nrm)
    ok = ok & ~bad
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    sg = torch.copysign(torch.ones_like(mz), mz)
    a = torch.full_like(mz, -1.0) / (sg + mz)   # a true division of two tensors (a scalar numerator would go through reciprocal)
    b = (mx * my) * a
    T = (1.0 + (sg * (mx * mx)) * a, sg * b, -(sg * mx))
    B = (b, sg + (my * my) * a, -my)
    o = pts - m * offset                        # fp32: the product rounded, then the difference
    o = torch.where(ok[:, None], o, torch.full_like(o, math.nan)).contiguous()   # a point that casts nothing: NaN hits nothing
    sw, swt = torch.zeros_like(mx), torch.zeros_like(mx)
    thin = torch.full_like(mx, inf)
    count = torch.zeros(n, dtype=torch.int32, device=pts.device)
    P, F = index.P.double(), index.F.long()
    for j in range(dirs.shape[0]):
        c = dirs[j]
        d = torch.stack([(T[k] * c[0] + B[k] * c[1]) - m[:, k] * c[2] for k in range(3)], 1).contiguous()
        t, face, _ = index.ray_cast(o, d, 0.0, far)
        hit = face >= 0
        if F.shape[0]:
            fi = face.clamp(min=0).long()
            g = _face_cross64(P, F[fi, 0], F[fi, 1], F[fi, 2])
            dd = d.double()
            hit = hit & ((((g[0] * dd[:, 0] + g[1] * dd[:, 1]) + g[2] * dd[:, 2]) * outward) > 0)
        dist = torch.where(hit, t, torch.zeros_like(t)).float()
        sw = torch.where(hit, sw + c[2], sw)
        swt = torch.where(hit, swt + c[2] * dist, swt)
        thin = torch.where(hit, torch.minimum(thin, dist), thin)
        count = count + hit.to(torch.int32)
    thick = torch.where(count > 0, swt / sw, torch.full_like(sw, inf))
    nan = torch.full_like(thick, math.nan)
    return torch.where(bad, nan, thick), torch.where(bad, nan, thin), count


def mesh_thickness_route():
    """What Mesh.thickness and TSR.bake_thickness_map's point kernel go through: mesh_thickness (one launch), unless
    SCULPT_DISTANCE_FORM holds the token `composedthickness` (then mesh_thickness_composed).  The two give the same bits; the
    timings of tools/time_thickness.py are in DESIGN.md 3.3p."""
    return mesh_thickness_composed if _lib.form_has("SCULPT_DISTANCE_FORM", "composedthickness") else mesh_thickness


def bake_thickness(v_pos, faces, normals, rast, thickness=True, cone=THICKNESS_CONE, offset=None, seed=0, outward=1.0, source=None,
                   cage=None):
    """The wall thickness of a surface S at every covered texel of a rasterised atlas of a (low-poly) mesh: the thickness map a
    baker ships beside normal and AO.  v_pos f32 [Nv, 3], faces i32 / i64 [Nf, 3], normals f32 [Nv, 3] per vertex (outward),
    rast f32 [res, res, 4] from bake_rasterize (device tensors; CPU tensors are refused); thickness, cone, offset, seed, outward:
    as for mesh_thickness (offset=None: 2^-13 of the longest side of S's bounds).  source / cage: as for bake_occlusion -- None:
    S is the mesh itself; (vertices, faces): S is that surface and every texel is first snapped onto it (step 4 of the occlusion
    bake), taking that face's unit normal on n's side.
    -> (thickness f32, thinnest f32, valid int32, mask bool), each [res, res]: mesh_thickness's values at the covered texels
    (NaN, NaN, 0 where the interpolated position or normal is not finite), exactly 0, 0, 0 and mask 0 where not covered.
    The shape of the composed occlusion bake, which these atlases measured as the faster one: the coverage in
    torch, nonzero, bake_interpolate of the positions and of the normals, the snap, the point kernel over the global cell-sorted
    list of texels, and a scatter -- no fused tile kernel.  tests/_thickref.py restates the texel rule in NumPy, bit for bit.
    res == 0 launches nothing."""
    who = "bake_thickness"
    dirs, far, outward = _thickness_rules(thickness, cone, offset, seed, outward)
    _source_rule(who, source, cage)
    index, v, f, nrm, r, offset, cage = _atlas_query_args(who, v_pos, faces, normals, rast, offset, source, cage)
    res, dev = r.shape[0], r.device
    thick = torch.zeros(res * res, dtype=torch.float32, device=dev)
    thin = torch.zeros(res * res, dtype=torch.float32, device=dev)
    valid = torch.zeros(res * res, dtype=torch.int32, device=dev)
    cov, at, pts, nr = _atlas_points(index, v, f, nrm, r, cage)
    if at is not None:
        query = _thickness_composed if _lib.form_has("SCULPT_DISTANCE_FORM", "composedthickness") else _SurfaceIndex.thickness
        thick[at], thin[at], valid[at] = query(index, pts, nr, torch.from_numpy(dirs).to(dev), offset, far, outward)
    return thick.view(res, res), thin.view(res, res), valid.view(res, res), cov


# ----------------------------------------------------------------------------------------------
# discrete curvature: mean and Gaussian per vertex, the curvature map (csrc/mesh_curvature.hip)
# ----------------------------------------------------------------------------------------------
CURVATURE_MAX_RINGS = 8
ATTRIBUTE_MAX_CHANNELS = 8


def curvature_rule(curvature):
    """`curvature` of the curvature queries -> rings: True (0 rings: the one-ring operator itself) or an int r in 0 .. 8 (r
    rounds of sums over the neighbours).  Anything else -- False, None, a float, NaN, a str, 9 -- is a ValueError, raised here,
    before anything is launched."""
    if curvature is True:
        return 0
    if _is_count(curvature, 0, CURVATURE_MAX_RINGS):
        return int(curvature)
    raise ValueError("curvature must be True or an int in 0 .. %d (rings), got %r" % (CURVATURE_MAX_RINGS, curvature))


def _outward_rule(outward):
    if not (_is_real(outward) and float(outward) in (1.0, -1.0)):   # a NaN is in neither
        raise ValueError("outward must be +1 or -1, got %r" % (outward,))
    return float(outward)


def mesh_curvature_terms(vertices, faces, outward=1.0):
    """The raw terms of the discrete curvature operators of Meyer, Desbrun, Schroeder and Barr (2003) per vertex, on the device
    (sculpt_curvature_terms, one gather).  vertices float [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors; CPU tensors are
    refused); outward: +1 when the faces wind counter-clockwise seen from outside, -1 otherwise.
    -> (area f64 [Nv], the mixed (Voronoi, or barycentric at obtuse triangles) area; deficit f64 [Nv] = 2 pi - the angle sum, the
    integrated Gaussian curvature; hint f64 [Nv], the integrated mean curvature H A, positive on a convex surface; valid bool
    [Nv]).  The rule, corner by corner in fp64 without contraction, is at the top of csrc/mesh_curvature.hip; tests/_curvref.py
    restates it in NumPy (bit for bit but for atan2).  valid is False -- and the three terms 0 -- where an edge at the vertex does
    not have exactly two faces (a border, a fin), where no face names the vertex and where the area is not > 0.  A pinched
    (bow-tie) vertex whose edges all have two faces is VALID and gets the deficit of its full angle sum: pinches are what
    mesh_report finds.  A face index out of range, a repeated index in a face and a non-finite position are a SculptError;
    Nf == 0 gives zeros and launches nothing."""
    outward = _outward_rule(outward)
    from .sf3d import remesh_device as rmd

    _device_mesh(vertices, faces, "mesh_curvature")
    area, deficit, hint, valid = rmd.curvature_device(vertices, faces, 0, outward, finish=False)
    return area, deficit, hint, valid.view(torch.bool)


def curvature_ring(terms, start, nb, rounds):
    """`rounds` (0 .. 8) rounds of X'_u = X_u + the sum of X_v over the valid v of row u, in row order, on the three f64 channels
    of terms = (area, deficit, hint, valid) as mesh_curvature_terms returns them; (start i32 [Nv + 1], nb i32) is the neighbour
    CSR of the smoothing filter (distinct neighbours in ascending order).  An invalid u stays zero and invalid.  -> new (area,
    deficit, hint, valid).  This is a walk-count-weighted average of the integrated curvature over the r-ring, not a geodesic
    disc: a neighbour reached by more walks of length <= r counts more often, in numerator and denominator alike."""
    if not _is_count(rounds, 0, CURVATURE_MAX_RINGS):
        raise ValueError("rounds must be an int in 0 .. %d, got %r" % (CURVATURE_MAX_RINGS, rounds))
    from .sf3d import remesh_device as rmd

    area, deficit, hint = (_req(t, torch.float64, "terms") for t in terms[:3])
    valid = terms[3]
    if not (isinstance(valid, torch.Tensor) and valid.is_cuda and valid.dtype in (torch.bool, torch.uint8) and valid.is_contiguous()):
        raise SculptError("terms: valid must be a contiguous bool / uint8 device tensor")
    start, nb = _req(start, torch.int32, "start"), _req(nb, torch.int32, "nb")
    nv = area.shape[0]
    if not (deficit.shape == hint.shape == valid.shape == area.shape == (nv,) and start.shape == (nv + 1,) and nb.dim() == 1):
        raise SculptError("curvature_ring: terms must be four [Nv] tensors and start [Nv + 1]")
    ctx = rmd._Ctx()
    out = rmd._curvature_ring(ctx, (area, deficit, hint, valid.view(torch.uint8)), start, nb, int(rounds))
    ctx.done()
    return out[:3] + (valid.view(torch.bool),)


def mesh_curvature(vertices, faces, curvature=True, outward=1.0):
    """Mean and Gaussian curvature per vertex of a triangle mesh, on the device: the discrete operators of Meyer, Desbrun,
    Schroeder and Barr (2003).  vertices float [Nv, 3], faces int32 / int64 [Nf, 3] (device tensors; CPU tensors are refused);
    curvature: True or the number of rings r in 0 .. 8 (curvature_rule); outward: +1 when the faces wind counter-clockwise seen
    from outside, -1 otherwise (it only sets the sign of the mean curvature).  A bad rule is a ValueError before any launch.
    -> (mean f32 [Nv], positive where the surface is convex; gauss f32 [Nv]; valid bool [Nv]).  Three steps, all fp64 in a fixed
    order (csrc/mesh_curvature.hip): the raw terms (mesh_curvature_terms); r rounds of curvature_ring over the neighbour table of
    the smoothing filter -- a walk-count-weighted average of the integrated curvature over the r-ring, not a geodesic disc, which
    is what takes the lattice-scale noise of a marching-cubes mesh out; then mean = hint / area and gauss = deficit / area,
    each rounded once to fp32.  Contract:
      - an invalid vertex (on an edge without exactly two faces, named by no face, without area) has NaN in both and never
        contributes to a neighbour; a pinched vertex whose edges all have two faces is valid (see mesh_curvature_terms);
      - a face without area contributes nothing; a right angle takes the Voronoi area;
      - a face index out of range, a repeated index in a face and a non-finite position are a SculptError;
      - Nf == 0: NaN, NaN, False and nothing is launched;
      - deterministic: gathers in a fixed order, no atomics; tests/_curvref.py restates every step in NumPy -- bit for bit but
        for the angle sum, which goes through atan2;
      - the host reads back the input check's status and the edge count of the one topology construction, nothing else."""
    rings = curvature_rule(curvature)
    outward = _outward_rule(outward)
    from .sf3d import remesh_device as rmd

    _device_mesh(vertices, faces, "mesh_curvature")
    mean, gauss, valid = rmd.curvature_device(vertices, faces, rings, outward)
    return mean, gauss, valid.view(torch.bool)


def principal_curvatures(mean, gauss):
    """(k1, k2) = H +- sqrt(max(H^2 - K, 0)) from mean = H and gauss = K (float32 tensors of one shape, on any device): computed
    in fp64 and rounded once, k1 >= k2; plain elementwise torch.  A NaN in either gives NaN in both."""
    if not (isinstance(mean, torch.Tensor) and isinstance(gauss, torch.Tensor) and mean.dtype == gauss.dtype == torch.float32
            and mean.shape == gauss.shape):
        raise SculptError("principal_curvatures: mean and gauss must be float32 tensors of one shape")
    h, k = mean.double(), gauss.double()
    d = h * h - k
    root = torch.sqrt(torch.where(d < 0.0, torch.zeros_like(d), d))   # a NaN stays a NaN
    return (h + root).float(), (h - root).float()


def surface_attribute_at(points, face, vertices, faces, values):
    """A per-vertex field read at points on a surface (sculpt_surface_attribute_at): points float [M, 3], face int32 / int64 [M]
    (the face each point lies on, as a closest-point or ray query reports it; < 0: none), vertices float [Nv, 3], faces int32 /
    int64 [Nf, 3], values f32 [Nv] or [Nv, C] with C <= 8 (device tensors) -> f32 [M] or [M, C].  Per point the barycentric
    weights are ratios of sub-triangle cross products against the face's own cross product in fp64, each clamped to [0, 1], the
    third 1 - w0 - w1, clamped; the value is the weighted sum in corner order, rounded once.  A corner whose value is NaN is
    skipped and the remaining weights renormalised, so one border vertex does not blank a texel; all three NaN, a face < 0 and a
    face without area give NaN.  M == 0 launches nothing."""
    who = "surface_attribute_at"
    pts = _query_points(points, who)
    _device_mesh(vertices, faces, who)
    if not (isinstance(face, torch.Tensor) and face.is_cuda and face.dtype in (torch.int32, torch.int64) and face.shape == (pts.shape[0],)):
        raise SculptError("%s: face must be an int32 / int64 device tensor [M]" % who)
    vals = _req(values.contiguous() if isinstance(values, torch.Tensor) else values, torch.float32, "values")
    P = vertices.detach().reshape(-1, 3).to(torch.float32).contiguous()
    F = faces.detach().reshape(-1, 3).to(torch.int32).contiguous()
    flat = vals.dim() == 1
    if vals.dim() not in (1, 2) or vals.shape[0] != P.shape[0] or not (flat or 1 <= vals.shape[1] <= ATTRIBUTE_MAX_CHANNELS):
        raise SculptError("%s: values %s must be [Nv] or [Nv, C <= %d] with Nv = %d" % (who, tuple(vals.shape), ATTRIBUTE_MAX_CHANNELS,
                                                                                       P.shape[0]))
    return _attribute_at(pts, face.clamp(min=-1).to(torch.int32).contiguous(), P, F, vals)


def _attribute_at(pts, face, P, F, vals):
    """pts f32 [M, 3], face i32 [M], P f32 [Nv, 3], F i32 [Nf, 3], vals f32 [Nv] or [Nv, C], all contiguous -> f32 [M] or [M, C]."""
    c = 1 if vals.dim() == 1 else vals.shape[1]
    m = pts.shape[0]
    out = torch.empty((m,) if vals.dim() == 1 else (m, c), dtype=torch.float32, device=pts.device)
    if m:
        nf, nv = F.shape[0], P.shape[0]
        check(lib.sculpt_surface_attribute_at(_ptr(pts), _ptr(face), m, _ptr(P) if nv else None, _ptr(F) if nf else None, nf, nv,
                                              _ptr(vals) if nv else None, c, _ptr(out), _stream()))
    return out


def _curvature_texels(v, f, clean, at, mean, gauss):
    """The mesh's own per-vertex (mean, gauss) at the covered texels `at`: bake_interpolate of the rows (H, K, ok) with ok = 1
    where neither is NaN and (0, 0, 0) elsewhere, then per texel by the number of its face's corners with ok: three -- the
    interpolated value as it is; none -- NaN; one or two -- the value divided by the interpolated ok (the weights that count,
    renormalised) -> (mean f32 [M], gauss f32 [M])."""
    ok = ~(torch.isnan(mean) | torch.isnan(gauss))
    zero = torch.zeros_like(mean)
    attr = torch.stack([torch.where(ok, mean, zero), torch.where(ok, gauss, zero), ok.to(torch.float32)], 1).contiguous()
    img = bake_interpolate(attr, clean, f).reshape(-1, 3)[at]
    tri = clean.reshape(-1, 4)[at, 3].to(torch.int64)
    n = ok[f[tri].to(torch.int64)].sum(1)
    nan = torch.full_like(img[:, 0], math.nan)
    pick = lambda x: torch.where(n == 3, x, torch.where(n == 0, nan, x / img[:, 2]))
    return pick(img[:, 0]), pick(img[:, 1])


def bake_curvature(v_pos, faces, normals, rast, curvature=True, outward=1.0, source=None, cage=None):
    """Mean and Gaussian curvature at every covered texel of a rasterised atlas of a (low-poly) mesh: the curvature map a baker
    ships beside normal, AO and thickness.  v_pos f32 [Nv, 3], faces i32 / i64 [Nf, 3], normals f32 [Nv, 3] per vertex, rast f32
    [res, res, 4] from bake_rasterize (device tensors; CPU tensors are refused); curvature, outward: as for mesh_curvature.
    source=None (cage must be None): the mesh's own mesh_curvature, interpolated over each face by bake_interpolate; a corner
    whose value is NaN (a border vertex) is skipped and the other weights renormalised, all three NaN give NaN
    (_curvature_texels).  source=(vertices, faces): the curvature of THAT surface -- the high-poly mesh the low one was
    simplified from -- read where each texel lands on it: the texel is snapped as in bake_occlusion (the closest hit of the ray
    from p + cage n towards p - cage n; cage=None: 2^-6 of the longest side of the source's bounds) and the source's per-vertex
    values are read on the hit face by surface_attribute_at; a texel whose ray hits nothing falls back to the mesh's own value.
    -> (mean f32, gauss f32, mask bool), each [res, res]: exactly 0 and mask 0 where not covered.  The composed atlas route (the
    coverage in torch, nonzero, bake_interpolate, the snap, a scatter): no fused tile kernel.  A bad rule is a ValueError before
    any launch; the meshes are checked as mesh_curvature checks them; res == 0 launches nothing."""
    who = "bake_curvature"
    rings = curvature_rule(curvature)
    outward = _outward_rule(outward)
    _source_rule(who, source, cage)
    v, f, nrm, r = _atlas_tensors(who, v_pos, faces, normals, rast)
    if source is not None:
        _device_mesh(source[0], source[1], who)
    res, dev = r.shape[0], r.device
    mean = torch.zeros(res * res, dtype=torch.float32, device=dev)
    gauss = torch.zeros(res * res, dtype=torch.float32, device=dev)
    if res == 0:
        return mean.view(0, 0), gauss.view(0, 0), torch.zeros((0, 0), dtype=torch.bool, device=dev)
    own = mesh_curvature(v, f, rings, outward)
    cov, clean = _covered_texels(r, v, f)
    if source is None:
        at, face = torch.nonzero(cov.reshape(-1))[:, 0], None
    else:
        high = mesh_curvature(source[0], source[1], rings, outward)
        index, _, _, _, _, _, cage = _atlas_query_args(who, v, f, nrm, r, None, source, cage)
        _, at, pts, _, face = _atlas_points(index, v, f, nrm, r, cage, want_face=True)
    if at is not None and at.numel():
        m, g = _curvature_texels(v, f, clean, at, own[0], own[1])
        if face is not None:
            hk = _attribute_at(pts, face, index.P, index.F, torch.stack([high[0], high[1]], 1).contiguous())
            hit = face >= 0
            m, g = torch.where(hit, hk[:, 0], m), torch.where(hit, hk[:, 1], g)
        mean[at], gauss[at] = m, g
    return mean.view(res, res), gauss.view(res, res), cov


# ----------------------------------------------------------------------------------------------
# ray-cast views of a mesh with its attributes and baked maps (csrc/mesh_ray.hip sculpt_surface_render)
# ----------------------------------------------------------------------------------------------
MESH_RENDER_GREY = 0.8             # the albedo of a mesh that has neither a texture nor vertex colours
MESH_RENDER_AMBIENT = 0.3
# pass -> (trailing shape, dtype, background)
MESH_RENDER_PASSES = {"color": ((3,), torch.float32, 1.0), "shaded": ((3,), torch.float32, 1.0), "opacity": ((), torch.float32, 0.0),
                      "rgba": ((4,), torch.float32, 0.0), "depth": ((), torch.float32, 0.0), "normal": ((3,), torch.float32, 0.0),
                      "occlusion": ((), torch.float32, 1.0), "face": ((), torch.int32, -1)}
_MESH_RENDER_MAPS = ("texture", "normal_map", "occlusion_map")


def mesh_render_passes(passes):
    """-> the passes of mesh_render as a tuple without repeats, in the order given; ValueError when there is none or one is
    unknown (tsr/passes.py check_passes, over this renderer's names)."""
    if isinstance(passes, str):
        passes = (passes,)
    passes = tuple(dict.fromkeys(passes))
    unknown = [p for p in passes if p not in MESH_RENDER_PASSES]
    if unknown:
        raise ValueError("unknown pass %s (any of %s)" % (unknown, ", ".join(MESH_RENDER_PASSES)))
    if not passes:
        raise ValueError("passes is empty (any of %s)" % ", ".join(MESH_RENDER_PASSES))
    return passes


def mesh_render_light(light):
    """`light` of mesh_render -> None (a headlight) or the unit direction towards the light as np.float32 [3], normalised in
    fp64 and rounded once; anything but None or three finite numbers that are not all 0 is a ValueError."""
    if light is None:
        return None
    try:
        l = np.asarray(light, np.float64).reshape(-1)
    except (TypeError, ValueError):
        l = np.zeros(0)
    n = float(np.sqrt((l * l).sum())) if l.shape == (3,) and np.isfinite(l).all() else 0.0
    if not (0.0 < n < math.inf):
        raise ValueError("light must be None (a headlight) or a finite direction (x, y, z) that is not 0, got %r" % (light,))
    return (l / n).astype(np.float32)


class _RenderJob:
    """The checked arguments of one mesh_render call: rules first (ValueError, nothing launched), then the tensors (SculptError),
    then one index over the mesh, shared by all views."""

    def __init__(self, who, rays_o, rays_d, vertices, faces, passes, material, ambient, light, outward):
        self.passes = mesh_render_passes(passes)
        m = dict(material)
        space = m.pop("normal_map_space", None)
        if space not in (None, "tangent", "object"):
            raise ValueError("%s: normal_map_space must be 'tangent' or 'object', got %r" % (who, space))
        if m.get("normal_map") is not None:
            if space is None:
                raise ValueError("%s: a normal_map needs its normal_map_space ('tangent' or 'object')" % who)
            if space == "tangent" and (m.get("corner_normals") is None or m.get("corner_tangents") is None):
                raise ValueError("%s: a tangent-space normal_map needs the frame it was baked in (corner_normals and corner_tangents)" % who)
        for name in _MESH_RENDER_MAPS:
            if m.get(name) is not None and m.get("uvs") is None:
                raise ValueError("%s: a %s needs the uvs it is looked up through" % (who, name))
        if not (_is_real(ambient) and math.isfinite(float(np.float32(ambient)))):
            raise ValueError("ambient must be a finite number, got %r" % (ambient,))
        if not (_is_real(outward) and math.isfinite(float(outward))):
            raise ValueError("outward must be a finite number (+1 or -1), got %r" % (outward,))
        self.ambient, self.outward, self.light = float(np.float32(ambient)), float(outward), mesh_render_light(light)
        for r, name in ((rays_o, "rays_o"), (rays_d, "rays_d")):
            if not (isinstance(r, torch.Tensor) and r.is_cuda):
                raise SculptError("%s: %s must be a CUDA/HIP tensor (no CPU fallback)" % (who, name))
            if r.dim() not in (2, 4) or r.shape[-1] != 3 or not r.dtype.is_floating_point:
                raise SculptError("%s: %s must be float [N, 3] or [n_images, H, W, 3], got %s %s" % (who, name, r.dtype, tuple(r.shape)))
        if rays_o.shape != rays_d.shape:
            raise SculptError("%s: rays_o %s and rays_d %s differ in shape" % (who, tuple(rays_o.shape), tuple(rays_d.shape)))
        self.o, self.d = rays_o.detach().to(torch.float32).contiguous(), rays_d.detach().to(torch.float32).contiguous()
        self.lead = tuple(self.o.shape[:-1])
        self.images = (1, 1, self.lead[0]) if len(self.lead) == 1 else self.lead       # (n_images, H, W)
        P, F = _surface(vertices, faces, who)
        nv, nf = P.shape[0], F.shape[0]
        if m.get("normal_map") is None or space == "object":     # the frame belongs to a tangent-space map
            m["corner_normals"] = m["corner_tangents"] = None
        rows = {"uvs": (3 * nf, 2), "corner_normals": (3 * nf, 3), "corner_tangents": (3 * nf, 4), "vertex_normals": (nv, 3),
                "vertex_occlusion": (nv,)}
        self.m = {}
        for name in ("uvs", "texture", "normal_map", "corner_normals", "corner_tangents", "occlusion_map", "vertex_colors",
                     "vertex_normals", "vertex_occlusion"):
            t = m.pop(name, None)
            if t is not None:
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype.is_floating_point):
                    raise SculptError("%s: %s must be a float CUDA/HIP tensor (no CPU fallback)" % (who, name))
                t = t.detach().to(torch.float32).contiguous()
                shape = tuple(t.shape)
                if name in rows:
                    ok = shape == rows[name]
                elif name == "vertex_colors":
                    ok = len(shape) == 2 and shape[0] == nv and shape[1] in (3, 4)
                else:
                    ok = shape[:2] == (shape[0], shape[0]) and 1 <= shape[0] <= 32768 and shape[2:] == ((3,) if name != "occlusion_map" else ())
                if not ok:
                    raise SculptError("%s: %s has shape %s for a mesh of %d vertices and %d faces" % (who, name, shape, nv, nf))
            self.m[name] = t
        if m:
            raise TypeError("%s: unknown material entries %s" % (who, sorted(m)))
        self.n = self.o.shape[0] if len(self.lead) == 1 else self.lead[0] * self.lead[1] * self.lead[2]
        self.index = _SurfaceIndex(P, F) if self.n else None

    def empty(self):
        dev = self.o.device
        return {p: torch.empty(self.lead + MESH_RENDER_PASSES[p][0], dtype=MESH_RENDER_PASSES[p][1], device=dev) for p in self.passes}


def _render_material(uvs, texture, normal_map, normal_map_space, corner_normals, corner_tangents, occlusion_map, vertex_colors,
              vertex_normals, vertex_occlusion):
    return dict(uvs=uvs, texture=texture, normal_map=normal_map, normal_map_space=normal_map_space, corner_normals=corner_normals,
                corner_tangents=corner_tangents, occlusion_map=occlusion_map, vertex_colors=vertex_colors,
                vertex_normals=vertex_normals, vertex_occlusion=vertex_occlusion)


def mesh_render(rays_o, rays_d, vertices, faces, passes=("color",), uvs=None, texture=None, normal_map=None, normal_map_space=None,
                corner_normals=None, corner_tangents=None, occlusion_map=None, vertex_colors=None, vertex_normals=None,
                vertex_occlusion=None, ambient=MESH_RENDER_AMBIENT, light=None, outward=1.0):
    """Pictures of a triangle mesh with its attributes and baked maps, ray cast on the device in ONE launch after the index build
    (sculpt_surface_render): every ray is followed to its closest hit by mesh_ray_cast's rule and the hit is shaded.  rays_o,
    rays_d float [n_images, H, W, 3] (a wave takes an 8 x 8 tile of an image) or [N, 3] (one row); vertices float [Nv, 3], faces
    int32 / int64 [Nf, 3]; all device tensors, CPU tensors are refused.  The material, every entry optional: uvs f32 [3*Nf, 2]
    per corner (origin bottom-left), texture [R, R, 3], normal_map [R, R, 3] holding 0.5 + 0.5 n with normal_map_space "object" or
    "tangent" (then with corner_normals [3*Nf, 3] and corner_tangents [3*Nf, 4], the frame it was baked in), occlusion_map [R, R]
    (row 0 of a map at the top; each map needs uvs), vertex_colors [Nv, 3 or 4], vertex_normals [Nv, 3], vertex_occlusion [Nv].
    -> {pass: tensor} with the rays' leading shape; passes (value [background]):
      "color"     [..., 3]  the albedo, unlit: texture, else vertex colours, else MESH_RENDER_GREY [1, 1, 1]
      "shaded"    [..., 3]  albedo * (ambient * a + (1 - ambient) * max(0, n . l)); l = -d / |d| (a headlight) or the unit
                            vector of `light`, the direction towards a fixed light [1, 1, 1]
      "opacity"   [...]     1 [0]
      "rgba"      [..., 4]  colour and opacity, premultiplied [0, 0, 0, 0]
      "depth"     [...]     fp32(t), in units of the direction's length [0; NaN for a non-finite ray]
      "normal"    [..., 3]  the shading normal n in world space: the normal map decoded, else the vertex normals interpolated,
                            else the face's own normal times `outward` [0, 0, 0]
      "occlusion" [...]     a: the occlusion map, else the vertex occlusion interpolated, else 1 [1]
      "face"      [...]     int32, the face hit [-1]
    A miss, a zero direction and a non-finite ray get the background.  The per-ray rule is in the header of csrc/mesh_ray.hip
    ("the mesh render"): a property of the ray and the mesh alone, bit for bit what mesh_render_composed computes and what
    tests/_meshrenderref.py restates in NumPy.  Only the passes asked for are computed.  Unknown or no passes, a normal_map
    without its space or frame, a map without uvs: ValueError before anything is launched.  Zero rays launch nothing; a mesh
    without faces renders the background."""
    job = _RenderJob("mesh_render", rays_o, rays_d, vertices, faces, passes,
                     _render_material(uvs, texture, normal_map, normal_map_space, corner_normals, corner_tangents, occlusion_map,
                               vertex_colors, vertex_normals, vertex_occlusion), ambient, light, outward)
    return _mesh_render_fused(job)


def _mesh_render_fused(job):
    out = job.empty()
    if job.index is None:
        return out
    m, index = job.m, job.index
    res = {k: (m[k].shape[0] if m[k] is not None else 0) for k in _MESH_RENDER_MAPS}
    material = _lib.RenderMaterial(*[_ptr(m[k]) for k in ("uvs", "texture", "normal_map", "corner_normals", "corner_tangents",
                                                         "occlusion_map", "vertex_colors", "vertex_normals", "vertex_occlusion")],
                                   res["texture"], res["normal_map"], res["occlusion_map"],
                                   m["vertex_colors"].shape[1] if m["vertex_colors"] is not None else 0)
    outputs = _lib.RenderOutputs(*[_ptr(out.get(p)) for p in ("color", "shaded", "opacity", "rgba", "depth", "normal", "occlusion", "face")])
    light = None if job.light is None else job.light.ctypes.data_as(ctypes.c_void_p)
    n_images, height, width = job.images
    check(lib.sculpt_surface_render(_ptr(job.o), _ptr(job.d), n_images, height, width, *index._args()[1], ctypes.byref(material),
                                    job.ambient, light, job.outward, ctypes.byref(outputs), _stream()))
    return out


def mesh_render_composed(rays_o, rays_d, vertices, faces, passes=("color",), uvs=None, texture=None, normal_map=None,
                         normal_map_space=None, corner_normals=None, corner_tangents=None, occlusion_map=None, vertex_colors=None,
                         vertex_normals=None, vertex_occlusion=None, ambient=MESH_RENDER_AMBIENT, light=None, outward=1.0):
    """mesh_render by the pieces that were there before it: one closest-hit query of all rays (mesh_ray_cast's kernels, which
    write the hits to memory) and torch gathers and elementwise operations, each rounded on its own, in the kernel's order.  The
    yardstick the fused kernel is tested (same bits) and timed against (tools/time_mesh_render.py)."""
    job = _RenderJob("mesh_render_composed", rays_o, rays_d, vertices, faces, passes,
                     _render_material(uvs, texture, normal_map, normal_map_space, corner_normals, corner_tangents, occlusion_map,
                               vertex_colors, vertex_normals, vertex_occlusion), ambient, light, outward)
    return _mesh_render_composed(job)


def _interp3(rows0, rows1, rows2, w0, w1, w2):
    """(A0 w0 + A1 w1) + A2 w2 over rows [n, C] (or [n]) with weights [n]."""
    if rows0.dim() == 2:
        w0, w1, w2 = w0[:, None], w1[:, None], w2[:, None]
    return (rows0 * w0 + rows1 * w1) + rows2 * w2


def _map_lookup(image, U, V):
    """The lookup of the rule in torch: image f32 [R, R] or [R, R, C], U, V f32 [n] -> [n] or [n, C]."""
    R = image.shape[0]
    X, Y = U * float(R), (1.0 - V) * float(R)
    bad = ~(torch.isfinite(X) & torch.isfinite(Y))
    X, Y = torch.where(bad, torch.zeros_like(X), X), torch.where(bad, torch.zeros_like(Y), Y)
    xf, yf = torch.floor(X), torch.floor(Y)
    fx, fy = X - xf, Y - yf
    gx, gy = 1.0 - fx, 1.0 - fy
    top = float(R - 1)
    x0, x1 = xf.clamp(0.0, top).long(), (xf + 1.0).clamp(0.0, top).long()
    y0, y1 = yf.clamp(0.0, top).long(), (yf + 1.0).clamp(0.0, top).long()
    if image.dim() == 3:
        fx, fy, gx, gy = fx[:, None], fy[:, None], gx[:, None], gy[:, None]
    return ((image[y0, x0] * gx + image[y0, x1] * fx) * gy) + ((image[y1, x0] * gx + image[y1, x1] * fx) * fy)


def _unit3(x):
    """unit(x) of the rule over rows [n, 3] -> (x / len, where it applies bool [n]); the root is taken in fp64 and rounded, which
    is the correctly rounded fp32 root."""
    s = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
    ln = torch.sqrt(s.double()).float()
    ok = (ln > 0) & (ln < math.inf)
    return x / ln[:, None], ok


def _mesh_render_composed(job):
    out = job.empty()
    if job.index is None:
        return out
    m, index, passes = job.m, job.index, job.passes
    o, d = job.o.reshape(-1, 3), job.d.reshape(-1, 3)
    n, nf = o.shape[0], index.F.shape[0]
    finite = torch.isfinite(o).all(1) & torch.isfinite(d).all(1)
    flat = {p: out[p].view((n,) + MESH_RENDER_PASSES[p][0]) for p in passes}

    def store(p, value, hit):
        shape, dtype, bg = MESH_RENDER_PASSES[p]
        back = torch.full((n,) + shape, bg, dtype=dtype, device=o.device)
        if p == "depth":
            back = torch.where(finite, back, torch.full_like(back, math.nan))
        if value is None:
            flat[p].copy_(back)
        else:
            flat[p].copy_(torch.where(hit if not shape else hit[:, None], value, back))

    if nf == 0:
        for p in passes:
            store(p, None, None)
        return out
    t, face, uv = index.ray_cast(o, d, 0.0, math.inf)
    hit = face >= 0
    fi = face.clamp(min=0).long()
    w1, w2 = uv[:, 0], uv[:, 1]
    w0 = (1.0 - w1) - w2
    F = index.F.long()
    i0, i1, i2 = F[fi, 0], F[fi, 1], F[fi, 2]
    c0, c1, c2 = 3 * fi, 3 * fi + 1, 3 * fi + 2

    def per_vertex(a):
        return _interp3(a[i0], a[i1], a[i2], w0, w1, w2)

    def per_corner(a):
        return _interp3(a[c0], a[c1], a[c2], w0, w1, w2)

    U = V = None
    if m["uvs"] is not None:
        q = per_corner(m["uvs"])
        U, V = q[:, 0], q[:, 1]
    albedo = None
    if any(p in passes for p in ("color", "shaded", "rgba")):
        if m["texture"] is not None:
            albedo = _map_lookup(m["texture"], U, V)
        elif m["vertex_colors"] is not None:
            albedo = per_vertex(m["vertex_colors"][:, :3].contiguous())
        else:
            albedo = torch.full((n, 3), MESH_RENDER_GREY, dtype=torch.float32, device=o.device)
    normal = None
    if "normal" in passes or "shaded" in passes:
        g = torch.stack(_face_cross64(index.P.double(), i0, i1, i2), 1) * job.outward
        ln = torch.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = (ln > 0) & (ln < math.inf)
        normal = torch.where(ok[:, None], (g / ln[:, None]).float(), torch.zeros((n, 3), dtype=torch.float32, device=o.device))
        if m["vertex_normals"] is not None:
            x, ok = _unit3(per_vertex(m["vertex_normals"]))
            normal = torch.where(ok[:, None], x, normal)
        if m["normal_map"] is not None:
            mm = 2.0 * _map_lookup(m["normal_map"], U, V) - 1.0
            if m["corner_normals"] is not None:
                N, T = per_corner(m["corner_normals"]), per_corner(m["corner_tangents"][:, :3].contiguous())
                s = m["corner_tangents"][c0, 3]
                B = torch.stack([s * (N[:, 1] * T[:, 2] - N[:, 2] * T[:, 1]), s * (N[:, 2] * T[:, 0] - N[:, 0] * T[:, 2]),
                                 s * (N[:, 0] * T[:, 1] - N[:, 1] * T[:, 0])], 1)
                mm = (mm[:, 0:1] * T + mm[:, 1:2] * B) + mm[:, 2:3] * N
            x, ok = _unit3(mm)
            normal = torch.where(ok[:, None], x, normal)
    ao = None
    if "occlusion" in passes or "shaded" in passes:
        if m["occlusion_map"] is not None:
            ao = _map_lookup(m["occlusion_map"], U, V)
        elif m["vertex_occlusion"] is not None:
            ao = per_vertex(m["vertex_occlusion"])
        else:
            ao = torch.ones(n, dtype=torch.float32, device=o.device)
    for p in passes:
        if p == "color":
            store(p, albedo, hit)
        elif p == "shaded":
            if job.light is None:
                x, ok = _unit3(-d)
                l = torch.where(ok[:, None], x, torch.zeros_like(x))
            else:
                l = torch.from_numpy(job.light).to(o.device).expand(n, 3)
            ndl = (normal[:, 0] * l[:, 0] + normal[:, 1] * l[:, 1]) + normal[:, 2] * l[:, 2]
            amb = torch.tensor(job.ambient, dtype=torch.float32, device=o.device)
            k = amb * ao + (1.0 - amb) * torch.where(ndl > 0, ndl, torch.zeros_like(ndl))
            store(p, albedo * k[:, None], hit)
        elif p == "opacity":
            store(p, torch.ones(n, dtype=torch.float32, device=o.device), hit)
        elif p == "rgba":
            store(p, torch.cat([albedo, torch.ones((n, 1), dtype=torch.float32, device=o.device)], 1), hit)
        elif p == "depth":
            store(p, t.float(), hit)
        elif p == "normal":
            store(p, normal, hit)
        elif p == "occlusion":
            store(p, ao, hit)
        else:
            store(p, face, hit)
    return out


def mesh_render_route():
    """What Mesh.render and TSR.render_mesh call: mesh_render, the fused kernel, unless SCULPT_DISTANCE_FORM holds the token
    `composedrender` (then mesh_render_composed; `fusedrender` names the fused one).  The two give the same bits
    (tests/test_gpu_mesh_render.py); tools/time_mesh_render.py times one against the other."""
    if _lib.form_has("SCULPT_DISTANCE_FORM", "fusedrender"):
        return mesh_render
    return mesh_render_composed if _lib.form_has("SCULPT_DISTANCE_FORM", "composedrender") else mesh_render


# ----------------------------------------------------------------------------------------------
# projection onto the field's iso-surface: fused Newton kernel + fold guard (csrc/mesh_project.hip)
# ----------------------------------------------------------------------------------------------
PROJECT_STEPS, PROJECT_CELLS = 8, 1.0   # what project=True means: at most 8 steps inside a trust radius of one lattice cell
PROJECT_MAX_STEPS, PROJECT_MAX_CELLS = 64, 8.0
PROJECT_RES_TOL = 1e-3                  # raw density units: ten times the fp32 noise of the point query (E_ref_density 9.2e-5)
PROJECT_UNFOLD_ROUNDS = 4


def project_rule(project):
    """`project` of the mesh projection -> (steps, max_cells): True (8 steps, a trust radius of 1 lattice cell), an int n in
    1 .. 64 (n steps, 1 cell) or a tuple (n, cells) with 0 < cells <= 8.  Anything else -- False, None, a str, a bare float, NaN,
    another length -- is a ValueError, raised here, before anything is launched."""
    if project is True or (isinstance(project, np.bool_) and bool(project)):
        return PROJECT_STEPS, PROJECT_CELLS
    if _is_count(project, 1, PROJECT_MAX_STEPS):
        return int(project), PROJECT_CELLS
    if isinstance(project, tuple) and len(project) == 2 and _is_count(project[0], 1, PROJECT_MAX_STEPS):
        cells = project[1]
        if _is_real(cells) and 0.0 < float(cells) <= PROJECT_MAX_CELLS:
            return int(project[0]), float(cells)   # a NaN fails the comparison
    raise ValueError("project must be True, an int in 1 .. %d (steps) or (steps, cells) with 0 < cells <= %g, got %r"
                     % (PROJECT_MAX_STEPS, PROJECT_MAX_CELLS, project))


def _project_args(steps, max_dist, res_tol, target):
    if not _is_count(steps, 0, PROJECT_MAX_STEPS):
        raise ValueError("steps must be an int in 0 .. %d, got %r" % (PROJECT_MAX_STEPS, steps))
    for name, x in (("max_dist", max_dist), ("res_tol", res_tol)):
        if not (0.0 < float(np.float32(x)) < math.inf):   # as the kernel sees it; a NaN fails the comparison
            raise ValueError("%s must be positive and finite in fp32, got %r" % (name, x))
    if not math.isfinite(float(np.float32(target))):
        raise ValueError("target must be finite, got %r" % (target,))


_PROJECT_EXTRAS = (("residual", torch.float32), ("status", torch.int32), ("evals", torch.int32))   # what the searches can return


def _want_extras(who, want):
    want = tuple(want)
    unknown = set(want) - {k for k, _ in _PROJECT_EXTRAS}
    if unknown:
        raise SculptError("%s: unknown output %s" % (who, sorted(unknown)))
    return want


def project_to_isosurface(planes, mlp, points, target, max_dist, steps=PROJECT_STEPS, res_tol=PROJECT_RES_TOL, radius=0.87,
                          align_corners=False, want=()):
    """`points` moved onto the iso-surface d(p) = target of the raw density (the `density` of field_normals / triplane_query,
    before bias and exp), by at most `steps` Newton steps along the density's own gradient, in ONE launch
    (sculpt_triplane_project; the rule, numbered, is DESIGN.md section 3.1e): p <- p - (d - target) g / |g|^2, clamped to the box
    [-radius, radius]^3, until |d - target| <= res_tol.  A point never ends further than max_dist (world units) from where it
    started and comes back as the iterate with the smallest |d - target| it has seen -- never worse than its start.  An axis
    with |p0_a| >= radius is frozen (bits kept, gradient component 0): a vertex on a face of the box stays on that face.
    planes: [3,C,H,W] (converted to channel-last here, once) or a ChannelLastPlanes; points [..., 3].
    -> (points' f32 [..., 3], extras) with extras[k] for k in want:
       "residual" f32 [...]   d(points') - target: the point query's density there minus target, in fp32
       "status"   i32 [...]   0 converged, 1 out of steps, 2 the next step left the trust region, 3 no usable value or gradient
                              (not finite, or a zero gradient: a point outside all three planes)
       "evals"    i32 [...]   evaluations of (d, g) the point used, 1 .. steps + 1
    A point's result depends on that point alone.  steps == 0 evaluates once and returns the input points."""
    want = _want_extras("project_to_isosurface", want)
    _project_args(steps, max_dist, res_tol, target)
    if points.shape[-1] != 3:
        raise SculptError("project_to_isosurface: points %s must be [..., 3]" % (tuple(points.shape),))
    if not isinstance(planes, ChannelLastPlanes):
        planes = ChannelLastPlanes(planes)
    shape = tuple(points.shape[:-1])
    pts = _req(points.reshape(-1, 3).contiguous(), torch.float32, "points")
    N = pts.shape[0]
    out = torch.empty((N, 3), dtype=torch.float32, device=pts.device)
    ex = {k: torch.empty((N,), dtype=dt, device=pts.device) if k in want else None for k, dt in _PROJECT_EXTRAS}
    check(lib.sculpt_triplane_project(_ptr(planes.data), planes.C, planes.H, planes.W, _ptr(mlp.blob), mlp.n_hidden, _ptr(pts), N,
                                      float(radius), _lib.QUERY_ALIGN_CORNERS if align_corners else 0, float(target), int(steps),
                                      float(max_dist), float(res_tol), _ptr(out), _ptr(ex["residual"]), _ptr(ex["status"]),
                                      _ptr(ex["evals"]), _stream()))
    return out.view(*shape, 3), {k: v.view(*shape) for k, v in ex.items() if v is not None}


def mesh_unfold(v_orig, v_new, faces, rounds=PROJECT_UNFOLD_ROUNDS):
    """The fold guard of the projection (sculpt_mesh_unfold): v_orig f32 [Nv, 3] the vertices before they were moved, v_new
    f32 [Nv, 3] after, faces int32 / int64 [Nf, 3] (device tensors).  A face is inverted when its normal on v_new does not point
    into the half-space of its normal on v_orig (n0.n1 <= 0 with n0.n0 > 0; a degenerate original face is skipped); `rounds`
    (0 .. 16) times every vertex of an inverted face takes its v_orig row back.
    -> (v f32 [Nv, 3], a new tensor; stats i32 [2] on the device: vertices reverted, faces still inverted -- unfold_stats reads
    it).  Nothing waits for the device.  fp32 without contraction: tests/_projref.py unfold restates it bit for bit."""
    if not _is_count(rounds, 0, 16):
        raise ValueError("rounds must be an int in 0 .. 16, got %r" % (rounds,))
    _device_mesh(v_orig, faces, "mesh_unfold")
    _device_mesh(v_new, faces, "mesh_unfold")
    if tuple(v_orig.shape) != tuple(v_new.shape):
        raise SculptError("mesh_unfold: v_orig %s and v_new %s differ in shape" % (tuple(v_orig.shape), tuple(v_new.shape)))
    P0 = v_orig.to(torch.float32).contiguous()
    P = v_new.to(torch.float32).clone(memory_format=torch.contiguous_format)
    F = faces.to(torch.int64).contiguous()
    nv, nf = P.shape[0], F.shape[0]
    stats = torch.empty((2,), dtype=torch.int32, device=P.device)
    mark = torch.empty((nv,), dtype=torch.int32, device=P.device) if rounds > 0 and nv > 0 else None
    check(lib.sculpt_mesh_unfold(_ptr(P0), _ptr(P), _ptr(F), nv, nf, int(rounds), _ptr(mark), _ptr(stats), _stream()))
    return P, stats


def unfold_stats(stats):
    """mesh_unfold's statistics on the host (this waits for the device): {"reverted": vertices that took their original
    position back, "inverted": faces still inverted after the last round}."""
    s = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    return {"reverted": int(s[0]), "inverted": int(s[1])}


def mesh_project(planes, mlp, vertices, faces, target, max_dist, steps=PROJECT_STEPS, res_tol=PROJECT_RES_TOL, radius=0.87,
                 rounds=PROJECT_UNFOLD_ROUNDS, align_corners=False, want=()):
    """project_to_isosurface on the vertices of a mesh, then mesh_unfold against the vertices it started from: two calls, no
    host wait.  -> (vertices' f32 [Nv, 3], info): info["stats"] the guard's device statistics (unfold_stats), and
    info[k] for k in want (project_to_isosurface's extras, of the projection BEFORE the guard: a reverted vertex keeps the
    record of the projection it lost)."""
    _device_mesh(vertices, faces, "mesh_project")
    v0 = vertices.to(torch.float32).contiguous()
    v1, extras = project_to_isosurface(planes, mlp, v0, target, max_dist, steps=steps, res_tol=res_tol, radius=radius,
                                       align_corners=align_corners, want=want)
    v, stats = mesh_unfold(v0, v1, faces, rounds)
    return v, dict(extras, stats=stats)


# ----------------------------------------------------------------------------------------------
# transformer primitives (bf16 storage as torch.bfloat16 tensors; fp32 accumulate)
# ----------------------------------------------------------------------------------------------
BF16 = torch.bfloat16
LN_SLOT = 64  # columns per LayerNorm statistics slice (csrc/gemm.hip)


def gemm(A, W, bias=None, residual=None, out_f32=None, out_bf16=None, out_t=None, M=None, epilogue=0, n_split=0,
         ln_stats=None, ln_colsum=None, ln_eps=1e-5, stats_out=None):
    """out[m][n] = epi(A[m][:] . W[n][:] + bias[n]) (+ residual[m][n]); see sculpt_gemm_bf16.
    A [>=M][K] bf16, W [N or 2N][K] bf16 (row stride = K).  Outputs are caller-allocated.
    LayerNorm fold (sculpt_gemm_bf16_ln): ln_stats [K/64][rows][2] + ln_colsum [N] -> A holds the un-normalised rows, W / bias
    have gamma / beta folded in (fold_layernorm); stats_out [N/64][rows][2] receives the slice statistics of out_f32."""
    K = A.shape[1]
    N = W.shape[0] // 2 if epilogue == _lib.EPI_GEGLU else W.shape[0]
    M = A.shape[0] if M is None else M
    ldo = (out_f32 if out_f32 is not None else out_bf16).stride(0) if (out_f32 is not None or out_bf16 is not None) else 0
    if out_f32 is not None and out_bf16 is not None:
        assert out_f32.stride(0) == out_bf16.stride(0)
    ln = None
    if _TILE_ROWS[0] and ln_stats is None and stats_out is None:
        ln = _lib.LnFold(None, 0, None, float(ln_eps), None, 0, int(_TILE_ROWS[0]))
    if ln_stats is not None or stats_out is not None:
        # statistics arrays are slice-major: [K/64 or N/64][rows][2]
        # (a view of a band of rows, [:, r0:r1], keeps the plane stride of the whole array: ld comes from the stride)
        ref = ln_stats if ln_stats is not None else stats_out
        ld = ref.stride(0) // 2
        ln = _lib.LnFold(_ptr(ln_stats), K // LN_SLOT if ln_stats is not None else 0, _ptr(ln_colsum), float(ln_eps), _ptr(stats_out), ld,
                         int(_TILE_ROWS[0]))
        if ln_stats is not None:
            assert ln_stats.dtype == torch.float32 and ln_stats.shape[0] >= K // LN_SLOT and ln_stats.stride(0) == 2 * ld and ln_colsum is not None
            assert ln_stats.shape[1] >= M and ln_stats.stride(1) == 2
        if stats_out is not None:
            assert stats_out.dtype == torch.float32 and stats_out.shape[0] >= N // LN_SLOT and stats_out.stride(0) == 2 * ld
            assert stats_out.shape[1] >= M and stats_out.stride(1) == 2
    check(lib.sculpt_gemm_bf16_ln(_ptr(A), A.stride(0), _ptr(W), W.stride(0), _ptr(bias), _ptr(residual),
                                  residual.stride(0) if residual is not None else 0, _ptr(out_f32), _ptr(out_bf16),
                                  ldo, _ptr(out_t), out_t.stride(0) if out_t is not None else 0, int(n_split), 0, M, N, K,
                                  epilogue, ctypes.byref(ln) if ln is not None else None, _stream()))


def gemm_last_form():
    """The tile form of this thread's last bf16 GEMM / implicit-convolution launch (sculpt_gemm_last_form) as a dict:
    family ("g128" / "g256"), epi, bw, nw, bm, ks, res, conv, gm, nmaj, stage, grid (x, y), text; {} before the first launch."""
    text = (lib.sculpt_gemm_last_form() or b"none").decode()
    if text == "none":
        return {}
    words = text.split()
    form = {"family": words[0], "text": text}
    for w in words[1:]:
        k, v = w.split("=")
        form[k] = tuple(int(x) for x in v.split("x")) if k == "grid" else int(v)
    return form


class _TileRows(threading.local):
    def __init__(self):
        self.v = 0

    def __getitem__(self, i):
        return self.v

    def __setitem__(self, i, value):
        self.v = value


_TILE_ROWS = _TileRows()   # per thread: 0, or the rows of one image while a stacked pass is being issued


class single_image_tiles:
    """with ops.single_image_tiles(rows): every bf16 GEMM issued inside chooses its tile form as for `rows` activation rows
    (sculpt_ln_fold_t::rows_per_image) -- a batched pass over stacked token rows then gives each image the bits of its own pass."""

    def __init__(self, rows):
        self.rows = int(rows)

    def __enter__(self):
        self.prev = _TILE_ROWS[0]
        _TILE_ROWS[0] = self.rows

    def __exit__(self, *exc):
        _TILE_ROWS[0] = self.prev
        return False


def fold_layernorm(W, bias, gamma, beta):
    """Host-side (load-time) fold of y = LayerNorm(x) * gamma + beta into the Linear that consumes it (fp32 tensors):
       W' = W * gamma (rounded to bf16 by the caller's upload), bias' = bias + W . beta, colsum = sum_k bf16(W')[n][k].
    Returns (W' fp32, bias' fp32, colsum fp32)."""
    W = W.detach().to(torch.float32).cpu()
    Wp = W * gamma.detach().to(torch.float32).cpu()[None, :]
    bp = (W.double() @ beta.detach().double().cpu())
    if bias is not None:
        bp = bp + bias.detach().double().cpu()
    colsum = Wp.to(BF16).double().sum(1)  # of the values the GEMM really multiplies by: the mean term cancels exactly
    return Wp, bp.to(torch.float32), colsum.to(torch.float32)


def row_slice_stats(x, stats, x_bf16=None, rows=None):
    """(mean, M2) of every 64-column slice of the fp32 rows x -> stats [cols/64][rows][2] (+ the bf16 copy of x)."""
    rows = x.shape[0] if rows is None else rows
    check(lib.sculpt_row_slice_stats(_ptr(x), x.stride(0), rows, x.shape[1], _ptr(stats), stats.shape[1], _ptr(x_bf16),
                                     x_bf16.stride(0) if x_bf16 is not None else 0, _stream()))


def attention(Q, K, Vt, O, Tq, Tk, heads, scale, batch=1, q_bs=0, k_bs=0, vt_bs=0, o_bs=0):
    """O = softmax(Q K^T scale) V per head (D=64); Vt is V transposed [heads*64][ld >= round_up(Tk,64)].
    scale=None: the queries already carry softmax_scale * log2(e) (sculpt_attention_bf16_prescaled).
    batch > 1: that many independent attentions in one launch (sculpt_attention_bf16_batched); entry b reads Q / K rows
    b*q_bs / b*k_bs ELEMENTS further on, V^T b*vt_bs elements (a column offset inside one array, or a whole array) and writes
    O + b*o_bs."""
    if batch > 1:
        check(lib.sculpt_attention_bf16_batched(_ptr(Q), Q.stride(0), int(q_bs), _ptr(K), K.stride(0), int(k_bs), _ptr(Vt),
                                                Vt.stride(0), int(vt_bs), _ptr(O), O.stride(0), int(o_bs), Tq, Tk, heads, int(batch),
                                                1 if scale is None else 0, 0.0 if scale is None else float(scale), _stream()))
    elif scale is None:
        check(lib.sculpt_attention_bf16_prescaled(_ptr(Q), Q.stride(0), _ptr(K), K.stride(0), _ptr(Vt), Vt.stride(0), _ptr(O),
                                                  O.stride(0), Tq, Tk, heads, _stream()))
    else:
        check(lib.sculpt_attention_bf16(_ptr(Q), Q.stride(0), _ptr(K), K.stride(0), _ptr(Vt), Vt.stride(0), _ptr(O),
                                        O.stride(0), Tq, Tk, heads, float(scale), _stream()))


def attention_last_form():
    """The kernel this thread's last bf16 attention launch started (sculpt_attention_last_form) as a dict: kernel ("plain" /
    "pipe"), nqb, pre, batch, grid (x, y), text; {} before the first launch."""
    text = (lib.sculpt_attention_last_form() or b"none").decode()
    if text == "none":
        return {}
    form = {"text": text}
    for w in text.split()[1:]:
        k, v = w.split("=")
        form[k] = v if k == "kernel" else tuple(int(x) for x in v.split("x")) if k == "grid" else int(v)
    return form


def layernorm(x, gamma, beta, eps, y=None, y_f32=None, rows=None, y_lt=None):
    """y_lt (a Limbs, fp32 x only): the normalised rows as three bf16 limbs, limb-tiled (sculpt_layernorm_limbs); y_f32 optional."""
    rows = x.shape[0] if rows is None else rows
    if y_lt is not None:
        assert x.dtype == torch.float32 and y is None and y_lt.cols == x.shape[1] and y_lt.rows >= rows
        check(lib.sculpt_layernorm_limbs(_ptr(x), x.stride(0), _ptr(gamma), _ptr(beta), float(eps), _ptr(y_lt.data), y_lt.code, _ptr(y_f32),
                                         y_f32.stride(0) if y_f32 is not None else 0, rows, x.shape[1], _stream()))
        return
    xf = x if x.dtype == torch.float32 else None
    xb = x if x.dtype == BF16 else None
    ldy = (y if y is not None else y_f32).stride(0)
    check(lib.sculpt_layernorm(_ptr(xf), _ptr(xb), x.stride(0), _ptr(gamma), _ptr(beta), float(eps), _ptr(y), ldy,
                               _ptr(y_f32), rows, x.shape[1], _stream()))


def groupnorm_tokens(x_ct, groups, gamma, beta, eps, y_tc, stats_ws):
    C, T = x_ct.shape
    yb = y_tc if y_tc.dtype == BF16 else None
    yf = y_tc if y_tc.dtype == torch.float32 else None
    check(lib.sculpt_groupnorm_tokens(_ptr(x_ct), C, T, groups, _ptr(gamma), _ptr(beta), float(eps), _ptr(yb), _ptr(yf),
                                      _ptr(stats_ws), _stream()))


def transpose_add(x_tc, residual_ct, out_ct):
    T, C = x_tc.shape
    check(lib.sculpt_transpose_add(_ptr(x_tc), _ptr(residual_ct), _ptr(out_ct), T, C, _stream()))


def vit_patchify(image_hwc, patch, mean, std, patches):
    S = image_hwc.shape[0]
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    pb = patches if patches.dtype == BF16 else None
    pf = patches if patches.dtype == torch.float32 else None
    check(lib.sculpt_vit_patchify(_ptr(image_hwc), S, patch, ctypes.cast(m, ctypes.c_void_p),
                                  ctypes.cast(s, ctypes.c_void_p), _ptr(pb), _ptr(pf), patches.stride(0), _stream()))


def vit_assemble(patch_out, cls, pos, tokens):
    n_patches, hidden = patch_out.shape[0], patch_out.shape[1]
    check(lib.sculpt_vit_assemble(_ptr(patch_out), _ptr(cls), _ptr(pos), _ptr(tokens), n_patches, hidden, _stream()))


def vit_assemble_stats(patch_out, cls, pos, tokens, stats, tokens_bf16=None):
    """vit_assemble + row_slice_stats of the assembled rows in one launch (the same bits): tokens [n_patches + 1, hidden] fp32,
    stats [hidden/64][rows >= n_patches + 1][2], tokens_bf16 the bf16 copy."""
    n_patches, hidden = patch_out.shape[0], patch_out.shape[1]
    check(lib.sculpt_vit_assemble_stats(_ptr(patch_out), _ptr(cls), _ptr(pos), _ptr(tokens), tokens.stride(0), n_patches, hidden,
                                        _ptr(stats), stats.shape[1], _ptr(tokens_bf16),
                                        tokens_bf16.stride(0) if tokens_bf16 is not None else 0, _stream()))


def upsample_scatter(g, bias, planes, S, Co):
    check(lib.sculpt_upsample_scatter(_ptr(g), g.stride(0), _ptr(bias), _ptr(planes), S, Co, _stream()))


def cast_bf16(x, y):
    check(lib.sculpt_cast_bf16(_ptr(x), _ptr(y), x.numel(), _stream()))


# ----------------------------------------------------------------------------------------------
# UV-space texture baker (StableFast)
# ----------------------------------------------------------------------------------------------
def bake_rasterize(uv, face_indices, bake_resolution):
    """TextureBaker.rasterize (sf3d/texture_baker/baker.py:12-59) on the GPU -> f32 [res, res, 4]."""
    uv = _req(uv.contiguous(), torch.float32, "uv")
    idx = _req(face_indices.to(torch.int32).contiguous(), torch.int32, "face_indices")
    res = int(bake_resolution)
    ws = _workspace(("bake", uv.device), lib.sculpt_bake_workspace_bytes(res), uv.device)
    out = torch.empty((res, res, 4), dtype=torch.float32, device=uv.device)
    check(lib.sculpt_bake_rasterize(_ptr(uv), uv.shape[0], _ptr(idx), idx.shape[0], res, _ptr(ws), _ptr(out), _stream()))
    return out


def bake_interpolate(attr, rast, face_indices):
    """TextureBaker.interpolate (baker.py:71-120) on the GPU -> f32 [res, res, 3]."""
    attr = _req(attr.contiguous(), torch.float32, "attr")
    rast = _req(rast.contiguous(), torch.float32, "rast")
    idx = _req(face_indices.to(torch.int32).contiguous(), torch.int32, "face_indices")
    res = rast.shape[0]
    out = torch.empty((res, res, 3), dtype=torch.float32, device=attr.device)
    check(lib.sculpt_bake_interpolate(_ptr(attr), attr.shape[0], _ptr(idx), idx.shape[0], _ptr(rast), res, _ptr(out), _stream()))
    return out


def _bake_scene_args(who, planes, v_pos, faces, rast):
    """The arguments the atlas bakes of a scene code share, checked -> (channel-last planes, v, f, rast, res)."""
    if not isinstance(planes, ChannelLastPlanes):
        planes = ChannelLastPlanes(planes)
    v, f = _mesh_args(who, v_pos, faces)
    r = _req(rast.contiguous() if isinstance(rast, torch.Tensor) else rast, torch.float32, "rast")
    if r.ndim != 3 or r.shape[0] != r.shape[1] or r.shape[2] != 4:
        raise SculptError("%s: rast %s must be [res, res, 4]" % (who, tuple(r.shape)))
    return planes, v, f, r, r.shape[0]


def bake_scene_color(planes, mlp, v_pos, faces, rast, radius=0.87):
    """Colour of a TripoSR scene code at every covered texel of a rasterised atlas, one launch (sculpt_bake_scene_color):
    the position bake_interpolate gives and the colour triplane_query gives there from channel-last planes, bit for bit, with
    no position image in between and no decoder work on texels outside the charts.
    planes: [3,C,H,W] (converted to channel-last here, once) or a ChannelLastPlanes; v_pos f32 [Nv,3]; faces i32 / i64 [Nf,3]
    indexing v_pos; rast f32 [res,res,4] from bake_rasterize.  -> (color f32 [res,res,3], exactly 0 where not covered;
    mask bool [res,res])."""
    planes, v, f, r, res = _bake_scene_args("bake_scene_color", planes, v_pos, faces, rast)
    color = torch.empty((res, res, 3), dtype=torch.float32, device=r.device)
    mask = torch.empty((res, res), dtype=torch.uint8, device=r.device)
    check(lib.sculpt_bake_scene_color(_ptr(planes.data), planes.C, planes.H, planes.W, _ptr(mlp.blob), mlp.n_hidden, _ptr(v), v.shape[0],
                                      _ptr(f), int(f.dtype == torch.int64), f.shape[0], _ptr(r), res, float(radius), _ptr(color),
                                      _ptr(mask), _stream()))
    return color, mask.view(torch.bool)


def corner_tangents(v_pos, faces, uvs, corner_normals):
    """Per-corner tangent frames of a UV-mapped mesh (sculpt_corner_tangents, one thread per face): v_pos f32 [Nv,3]; faces
    i32 / i64 [Nf,3]; uvs f32 [3Nf,2] per face corner, origin bottom-left (Mesh.uvs); corner_normals f32 [3Nf,3] unit normals
    per face corner -> f32 [3Nf,4] = (T.xyz, w): T the face's dP/du made perpendicular to the corner's normal and normalised,
    w = +1 / -1 the handedness (cross(N, T) * w points along dP/dv; a chart mirrored in the atlas gets -1).  A face without UV
    area, or a corner whose normal is parallel to dP/du, gets a unit vector perpendicular to the normal (its cross product with
    the axis of its smallest component) and w = +1."""
    v, f = _mesh_args("corner_tangents", v_pos, faces)
    uv = _req(uvs.contiguous() if isinstance(uvs, torch.Tensor) else uvs, torch.float32, "uvs")
    cn = _req(corner_normals.contiguous() if isinstance(corner_normals, torch.Tensor) else corner_normals, torch.float32,
              "corner_normals")
    nf = f.shape[0]
    if tuple(uv.shape) != (3 * nf, 2) or tuple(cn.shape) != (3 * nf, 3):
        raise SculptError("corner_tangents: uvs %s must be [%d, 2] and corner_normals %s [%d, 3] (three rows per face)"
                          % (tuple(uv.shape), 3 * nf, tuple(cn.shape), 3 * nf))
    out = torch.empty((3 * nf, 4), dtype=torch.float32, device=v.device)
    check(lib.sculpt_corner_tangents(_ptr(v), v.shape[0], _ptr(f), int(f.dtype == torch.int64), nf, _ptr(uv), _ptr(cn), _ptr(out),
                                     _stream()))
    return out


def _frame_args(who, frame, nf):
    """`frame` of the normal bakes, checked -> (corner_normals, corner_tangents), or (None, None) without a frame."""
    if frame is None:
        return None, None
    if not (isinstance(frame, (tuple, list)) and len(frame) == 2):
        raise SculptError("%s: frame must be None or (corner_normals, corner_tangents)" % who)
    cn = _req(frame[0], torch.float32, "corner_normals")
    ct = _req(frame[1], torch.float32, "corner_tangents")
    if tuple(cn.shape) != (3 * nf, 3) or tuple(ct.shape) != (3 * nf, 4):
        raise SculptError("%s: corner_normals %s must be [%d, 3] and corner_tangents %s [%d, 4] (three rows per face)"
                          % (who, tuple(cn.shape), 3 * nf, tuple(ct.shape), 3 * nf))
    if nf == 0:   # no face, no frame rows: nothing is covered, and an empty tensor has no address
        return None, None
    return cn, ct


def bake_scene_normal(planes, mlp, v_pos, faces, rast, radius=0.87, frame=None):
    """Unit normal of a TripoSR scene code's density field at every covered texel of a rasterised atlas, one launch
    (sculpt_bake_scene_normal): the position bake_interpolate gives and the normal field_normals gives there, bit for bit, with
    no position image in between and no decoder work on texels outside the charts.
    planes, v_pos, faces, rast: as for bake_scene_color.  frame=None: object space, the world normal itself.
    frame=(corner_normals f32 [3Nf,3], corner_tangents f32 [3Nf,4] from ops.corner_tangents): tangent space in the MikkTSpace /
    Blender / glTF convention (frames interpolated un-normalised, B = w * cross(N, T)): the stored unit vector (x, y, z) decodes
    as normalize(x T + y B + z N); the flat (0, 0, 1) where the interpolated frame is singular.
    -> (normal f32 [res,res,3] in [-1, 1], not encoded, exactly 0 where not covered; mask bool [res,res])."""
    if isinstance(rast, torch.Tensor) and not rast.is_contiguous():   # a view of a larger image is a caller's mistake, not copied
        raise SculptError("bake_scene_normal: rast must be contiguous")
    planes, v, f, r, res = _bake_scene_args("bake_scene_normal", planes, v_pos, faces, rast)
    cn, ct = _frame_args("bake_scene_normal", frame, f.shape[0])
    normal = torch.empty((res, res, 3), dtype=torch.float32, device=r.device)
    mask = torch.empty((res, res), dtype=torch.uint8, device=r.device)
    if res == 0:
        return normal, mask.view(torch.bool)
    check(lib.sculpt_bake_scene_normal(_ptr(planes.data), planes.C, planes.H, planes.W, _ptr(mlp.blob), mlp.n_hidden, _ptr(v), v.shape[0],
                                       _ptr(f), int(f.dtype == torch.int64), f.shape[0], _ptr(r), res, float(radius), _ptr(cn),
                                       _ptr(ct), _ptr(normal), _ptr(mask), _stream()))
    return normal, mask.view(torch.bool)


# ----------------------------------------------------------------------------------------------
# bake at the surface: project each texel onto the iso-surface first (csrc/bake_surface.hip)
# ----------------------------------------------------------------------------------------------
def _bake_surface_args(who, planes, v_pos, faces, rast, target, max_dist, steps, res_tol, frame, want):
    """The checks the two routes of the surface bake share: _bake_scene_args, _project_args and the frame checks of
    bake_scene_normal -> (channel-last planes, v, f, rast, res, corner_normals or None, corner_tangents or None, want)."""
    want = _want_extras(who, want)
    _project_args(steps, max_dist, res_tol, target)
    planes, v, f, r, res = _bake_scene_args(who, planes, v_pos, faces, rast)
    cn, ct = _frame_args(who, frame, f.shape[0])
    return planes, v, f, r, res, cn, ct, want


def bake_scene_surface(planes, mlp, v_pos, faces, rast, target, max_dist, steps=PROJECT_STEPS, res_tol=PROJECT_RES_TOL, radius=0.87,
                       frame=None, want=()):
    """What a baker does, in ONE launch (sculpt_bake_scene_surface): every covered texel of a rasterised atlas goes from its
    point on the low-poly face to the high-poly surface -- here the iso-surface d(p) = target of the scene code's raw density,
    reached by project_to_isosurface's rule (at most `steps` Newton steps inside the trust radius max_dist) --
    and the field's unit normal is read there.  Per covered texel, bit for bit: point, and the extras, are what
    project_to_isosurface returns for the position bake_interpolate gives; normal is what field_normals gives at `point`,
    as it is (frame=None, object space) or through bake_scene_normal's tangent-space transform at the texel's own barycentrics
    (frame=(corner_normals, corner_tangents): the low-poly face and its frame do not move).  steps == 0 is bake_scene_normal.
    planes, v_pos, faces, rast, radius, frame: as for bake_scene_normal; target, max_dist, steps, res_tol: as for
    project_to_isosurface.
    -> (point f32 [res,res,3], normal f32 [res,res,3] not encoded, mask bool [res,res], extras) with extras[k] for k in want:
    "residual" f32 [res,res], "status" i32 [res,res] (0 .. 3 as project_to_isosurface; -1 where not covered), "evals" i32
    [res,res].  Where a texel is not covered point, normal and residual are exactly 0 and evals is 0.  A texel's outputs depend
    on that texel alone."""
    planes, v, f, r, res, cn, ct, want = _bake_surface_args("bake_scene_surface", planes, v_pos, faces, rast, target, max_dist, steps,
                                                             res_tol, frame, want)
    dev = r.device
    point = torch.empty((res, res, 3), dtype=torch.float32, device=dev)
    normal = torch.empty((res, res, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((res, res), dtype=torch.uint8, device=dev)
    ex = {k: torch.empty((res, res), dtype=dt, device=dev) if k in want else None for k, dt in _PROJECT_EXTRAS}
    if res > 0:
        check(lib.sculpt_bake_scene_surface(_ptr(planes.data), planes.C, planes.H, planes.W, _ptr(mlp.blob), mlp.n_hidden, _ptr(v),
                                            v.shape[0], _ptr(f), int(f.dtype == torch.int64), f.shape[0], _ptr(r), res, float(radius),
                                            _ptr(cn), _ptr(ct), float(target), int(steps), float(max_dist), float(res_tol), _ptr(point),
                                            _ptr(normal), _ptr(ex["residual"]), _ptr(ex["status"]), _ptr(ex["evals"]), _ptr(mask),
                                            _stream()))
    return point, normal, mask.view(torch.bool), {k: t for k, t in ex.items() if t is not None}


def _tangent_space_composed(n, bary, tri, cn, ct):
    """bake_scene_normal's tangent-space transform (csrc/tangent_frame.h) in torch, one fp32 call per operation in the kernel's
    order: world normals n [M,3], barycentrics [M,3], face index [M] (long) -> the stored vectors [M,3]."""
    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    def cross(a, b):
        return torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                            a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)

    cn3, ct4 = cn.view(-1, 3, 3)[tri], ct.view(-1, 3, 4)[tri]
    u, v, w = bary[:, 0:1], bary[:, 1:2], bary[:, 2:3]
    N = (cn3[:, 0] * u + cn3[:, 1] * v) + cn3[:, 2] * w
    T = (ct4[:, 0, :3] * u + ct4[:, 1, :3] * v) + ct4[:, 2, :3] * w
    B = ct4[:, 0, 3:4] * cross(N, T)
    gtt, gnn, gtn = dot(T, T), dot(N, N), dot(T, N)
    D = gtt * gnn - gtn * gtn
    nT, nN, nB = dot(n, T), dot(n, N), dot(n, B)
    x, y, z = nT * gnn - nN * gtn, nB, nN * gtt - nT * gtn
    length = torch.sqrt((x * x + y * y) + z * z)
    ok = (D > 0) & (length > 0) & (length < math.inf) & ~(n == 0).all(1)
    flat = torch.tensor([0.0, 0.0, 1.0], dtype=n.dtype, device=n.device)
    return torch.where(ok[:, None], torch.stack([x / length, y / length, z / length], 1), flat)


def bake_scene_surface_composed(planes, mlp, v_pos, faces, rast, target, max_dist, steps=PROJECT_STEPS, res_tol=PROJECT_RES_TOL,
                                radius=0.87, frame=None, want=()):
    """bake_scene_surface from ops that were there before it, the restatement the fused kernel is held to bit for bit and the
    route it is timed against: bake_interpolate -> the covered texels (nonzero: this waits for the device) ->
    project_to_isosurface -> field_normals at the projected points -> the tangent-space transform in torch, one call per
    operation -> scatter into images that are 0 (status -1) elsewhere.  Same arguments, same result: the coverage is
    texel_position's (a texel whose tri or vertex rows are out of range, or whose tri is a NaN, is not covered), worked out here
    in torch, and bake_interpolate, which guards nothing, reads through checked rows only."""
    planes, v, f, r, res, cn, ct, want = _bake_surface_args("bake_scene_surface_composed", planes, v_pos, faces, rast, target, max_dist,
                                                             steps, res_tol, frame, want)
    dev = r.device
    point = torch.zeros((res, res, 3), dtype=torch.float32, device=dev)
    normal = torch.zeros((res, res, 3), dtype=torch.float32, device=dev)
    ex = {"residual": torch.zeros((res, res), dtype=torch.float32, device=dev),
          "status": torch.full((res, res), -1, dtype=torch.int32, device=dev),
          "evals": torch.zeros((res, res), dtype=torch.int32, device=dev)}
    covered, r = _covered_texels(r, v, f)
    idx = covered.reshape(-1).nonzero()[:, 0]
    if idx.numel() > 0:
        pos = bake_interpolate(v, r, f).reshape(-1, 3)[idx].contiguous()
        p, got = project_to_isosurface(planes, mlp, pos, target, max_dist, steps=steps, res_tol=res_tol, radius=radius,
                                       want=("residual", "status", "evals"))
        n = field_normals(planes, mlp, p, radius=radius)["normal"]
        if cn is not None:
            texel = r.reshape(-1, 4)[idx]
            n = _tangent_space_composed(n, texel[:, :3], texel[:, 3].to(torch.int32).long(), cn, ct)
        point.view(-1, 3)[idx] = p
        normal.view(-1, 3)[idx] = n
        for k in ex:
            ex[k].view(-1)[idx] = got[k]
    return point, normal, covered, {k: ex[k] for k in want}


def bake_surface_route():
    """What TSR.bake_surface_maps calls: bake_scene_surface_composed, unless SCULPT_DISTANCE_FORM holds the token `fusedsurface`
    (then bake_scene_surface, the one fused launch).  The two give the same bits; the composed route is the default because it
    is the faster one on the flagship atlas (DESIGN.md 3.1g has the figures)."""
    return bake_scene_surface if _lib.form_has("SCULPT_DISTANCE_FORM", "fusedsurface") else bake_scene_surface_composed


# ----------------------------------------------------------------------------------------------
# displacement bake: each texel to the iso-surface along the low-poly normal (csrc/bake_displacement.hip)
# ----------------------------------------------------------------------------------------------
DISPLACEMENT_STEPS, DISPLACEMENT_CELLS = 8, 2.0   # what displacement=True means: at most 8 steps within 2 lattice cells


def displacement_rule(displacement):
    """`displacement` of the displacement bake -> (steps, max_cells): True (8 steps within 2 lattice cells on either side), an
    int n in 1 .. 64 (n steps, 2 cells) or a tuple (n, cells) with 0 < cells <= 8.  Anything else -- False, None, a str, a bare
    float, NaN, another length -- is a ValueError, raised here, before anything is launched."""
    if displacement is True or (isinstance(displacement, np.bool_) and bool(displacement)):
        return DISPLACEMENT_STEPS, DISPLACEMENT_CELLS
    if _is_count(displacement, 1, PROJECT_MAX_STEPS):
        return int(displacement), DISPLACEMENT_CELLS
    if isinstance(displacement, tuple) and len(displacement) == 2 and _is_count(displacement[0], 1, PROJECT_MAX_STEPS):
        cells = displacement[1]
        if _is_real(cells) and 0.0 < float(cells) <= PROJECT_MAX_CELLS:
            return int(displacement[0]), float(cells)   # a NaN fails the comparison
    raise ValueError("displacement must be True, an int in 1 .. %d (steps) or (steps, cells) with 0 < cells <= %g, got %r"
                     % (PROJECT_MAX_STEPS, PROJECT_MAX_CELLS, displacement))


def _project_along_launch(planes, mlp, pts, dirs, n, count, radius, align_corners, target, steps, max_dist, res_tol, scatter, rows,
                          height, ex):
    check(lib.sculpt_triplane_project_along(_ptr(planes.data), planes.C, planes.H, planes.W, _ptr(mlp.blob), mlp.n_hidden, _ptr(pts),
                                            _ptr(dirs), n, _ptr(count), float(radius), _lib.QUERY_ALIGN_CORNERS if align_corners else 0,
                                            float(target), int(steps), float(max_dist), float(res_tol), _ptr(scatter), rows,
                                            _ptr(height), _ptr(ex["residual"]), _ptr(ex["status"]), _ptr(ex["evals"]), _stream()))


def project_along(planes, mlp, points, directions, target, max_dist, steps=DISPLACEMENT_STEPS, res_tol=PROJECT_RES_TOL, radius=0.87,
                  align_corners=False, want=(), count=None, out=None):
    """Per point the signed height h along the unit direction n = directions / |directions| at which the raw density reaches
    `target`: d(points + h n) = target, found by a safeguarded Newton search along that line in ONE launch
    (sculpt_triplane_project_along; the rule, numbered, is DESIGN.md section 3.1h): the Newton step of the density along the
    line, kept within |h| <= max_dist and the box [-radius, radius]^3, replaced by the midpoint of the last sign change whenever
    it would leave it, until |d - target| <= res_tol.  The point never leaves the line, and the height that comes back is the
    one with the smallest |d - target| seen -- never worse than h = 0.
    planes: [3,C,H,W] (converted to channel-last here, once) or a ChannelLastPlanes; points, directions [..., 3].
    -> (height f32 [...], extras) with extras[k] for k in want:
       "residual" f32 [...]   d(points + height n) - target: the point query's density there minus target, in fp32
       "status"   i32 [...]   0 converged, 1 out of steps, 2 the search left the trust region, 3 no usable value, gradient or
                              direction (a zero or non-finite direction: height 0, evals 0)
       "evals"    i32 [...]   evaluations of (d, g) the point used, 0 .. steps + 1
    count: a device int32 tensor of one element -- only the first min(count, N) points are read, and only their rows of the
    outputs are written; out: a dict of preallocated flat outputs ("height" and the extras) to write into, for the rows that
    must stay untouched.  A point's result depends on that point alone."""
    want = _want_extras("project_along", want)
    _project_args(steps, max_dist, res_tol, target)
    if points.shape[-1] != 3 or tuple(points.shape) != tuple(directions.shape):
        raise SculptError("project_along: points %s and directions %s must both be [..., 3]" % (tuple(points.shape), tuple(directions.shape)))
    if not isinstance(planes, ChannelLastPlanes):
        planes = ChannelLastPlanes(planes)
    shape = tuple(points.shape[:-1])
    pts = _req(points.reshape(-1, 3).contiguous(), torch.float32, "points")
    dirs = _req(directions.reshape(-1, 3).contiguous(), torch.float32, "directions")
    N = pts.shape[0]
    if count is not None:
        count = _req(count, torch.int32, "count")
        if count.numel() != 1:
            raise SculptError("project_along: count must hold one int32")
    ex = {}
    for k, dt in (("height", torch.float32),) + _PROJECT_EXTRAS:
        if k != "height" and k not in want:
            ex[k] = None
        elif out is not None and k in out:
            ex[k] = _req(out[k], dt, k)
            if ex[k].numel() != N:
                raise SculptError("project_along: out[%r] must hold %d elements" % (k, N))
        else:
            ex[k] = torch.empty((N,), dtype=dt, device=pts.device)
    _project_along_launch(planes, mlp, pts, dirs, N, count, radius, align_corners, target, steps, max_dist, res_tol, None, N,
                          ex["height"], ex)
    return ex["height"].view(*shape), {k: ex[k].view(*shape) for k in want}


def bake_texel_list(v_pos, faces, rast, normals=None):
    """The covered texels of a rasterised atlas as a list on the device, with NO host wait (sculpt_bake_texel_list: per-block
    counts and scans, no atomics): v_pos f32 [Nv,3], faces i32 / i64 [Nf,3], rast f32 [res,res,4] from bake_rasterize, normals
    f32 [Nv,3] or None.  "Covered" is the index guard of the scene bakes (tri >= 0 and in range, its vertex rows in range).
    -> dict(list i32 [res*res]: rows 0 .. count-1 are the flat indices of the covered texels in row-major order, the rest is not
    written; count i32 [1] on the device; p0 f32 [res*res,3]: per listed texel the position bake_interpolate gives; directions
    f32 [res*res,3] (with normals): per listed texel the per-vertex normals interpolated un-normalised, (N0 u + N1 v) + N2 w;
    mask bool [res,res])."""
    if not (isinstance(rast, torch.Tensor) and rast.is_contiguous()):
        raise SculptError("bake_texel_list: rast must be a contiguous tensor")
    v, f = _mesh_args("bake_texel_list", v_pos, faces)
    r = _req(rast, torch.float32, "rast")
    if r.ndim != 3 or r.shape[0] != r.shape[1] or r.shape[2] != 4:
        raise SculptError("bake_texel_list: rast %s must be [res, res, 4]" % (tuple(r.shape),))
    nrm = None
    if normals is not None:
        nrm = _req(normals.contiguous(), torch.float32, "normals")
        if tuple(nrm.shape) != tuple(v.shape):
            raise SculptError("bake_texel_list: normals %s must be per vertex %s" % (tuple(nrm.shape), tuple(v.shape)))
    return _texel_list(v, f, r, nrm, None)


def _texel_list(v, f, r, nrm, images):
    res, dev = r.shape[0], r.device
    n = res * res
    got = {"list": torch.empty((n,), dtype=torch.int32, device=dev), "count": torch.empty((1,), dtype=torch.int32, device=dev),
           "p0": torch.empty((n, 3), dtype=torch.float32, device=dev),
           "directions": torch.empty((n, 3), dtype=torch.float32, device=dev) if nrm is not None else None,
           "mask": torch.empty((res, res), dtype=torch.uint8, device=dev)}
    ws = torch.empty((max(1, int(lib.sculpt_bake_texel_list_workspace_bytes(res))),), dtype=torch.uint8, device=dev)
    im = images or {}
    check(lib.sculpt_bake_texel_list(_ptr(v), v.shape[0], _ptr(f), int(f.dtype == torch.int64), f.shape[0], _ptr(nrm), _ptr(r), res,
                                     _ptr(ws), _ptr(got["list"]), _ptr(got["count"]), _ptr(got["p0"]), _ptr(got["directions"]),
                                     _ptr(got["mask"]), _ptr(im.get("height")), _ptr(im.get("residual")), _ptr(im.get("status")),
                                     _ptr(im.get("evals")), _stream()))
    got["mask"] = got["mask"].view(torch.bool)
    return {k: t for k, t in got.items() if t is not None}


def _bake_displacement_args(who, planes, v_pos, faces, normals, rast, target, max_dist, steps, res_tol, want):
    want = _want_extras(who, want)
    _project_args(steps, max_dist, res_tol, target)
    if isinstance(rast, torch.Tensor) and not rast.is_contiguous():
        raise SculptError("%s: rast must be contiguous" % who)
    planes, v, f, r, res = _bake_scene_args(who, planes, v_pos, faces, rast)
    nrm = _req(normals.contiguous() if isinstance(normals, torch.Tensor) else normals, torch.float32, "normals")
    if tuple(nrm.shape) != tuple(v.shape):
        raise SculptError("%s: normals %s must be per vertex %s" % (who, tuple(nrm.shape), tuple(v.shape)))
    return planes, v, f, nrm, r, res, want


def bake_displacement(planes, mlp, v_pos, faces, normals, rast, target, max_dist, steps=DISPLACEMENT_STEPS, res_tol=PROJECT_RES_TOL,
                      radius=0.87, want=()):
    """The displacement bake without a host wait: per covered texel of a rasterised atlas the signed height along the low-poly
    normal at which the scene code's raw density reaches `target` -- project_along's rule from the texel's point p0
    (bake_interpolate's bits) along the per-vertex `normals` f32 [Nv,3] interpolated at the texel.  Two calls:
    sculpt_bake_texel_list (the covered texels as a list on the device, their p0 and directions, the images' values outside the
    charts) and sculpt_triplane_project_along over that list, which reads the list's length on the device and scatters into
    the images.  planes, v_pos, faces, rast, radius: as for bake_scene_normal; target, max_dist, steps, res_tol: as for
    project_along.
    -> (height f32 [res,res], mask bool [res,res], extras) with extras[k] for k in want: "residual" f32, "status" i32 (0 .. 3
    as project_along; -1 where not covered), "evals" i32, each [res,res].  Where a texel is not covered height and residual are
    exactly 0 and evals is 0.  A texel's outputs depend on that texel alone."""
    planes, v, f, nrm, r, res, want = _bake_displacement_args("bake_displacement", planes, v_pos, faces, normals, rast, target, max_dist,
                                                              steps, res_tol, want)
    dev = r.device
    im = {k: torch.empty((res, res), dtype=dt, device=dev) if k == "height" or k in want else None
          for k, dt in (("height", torch.float32),) + _PROJECT_EXTRAS}
    if res == 0:
        return im["height"], torch.empty((0, 0), dtype=torch.bool, device=dev), {k: im[k] for k in want}
    got = _texel_list(v, f, r, nrm, im)
    _project_along_launch(planes, mlp, got["p0"], got["directions"], res * res, got["count"], radius, False, target, steps, max_dist,
                          res_tol, got["list"], res * res, im["height"], im)
    return im["height"], got["mask"], {k: im[k] for k in want}


def bake_displacement_composed(planes, mlp, v_pos, faces, normals, rast, target, max_dist, steps=DISPLACEMENT_STEPS,
                               res_tol=PROJECT_RES_TOL, radius=0.87, want=()):
    """bake_displacement from ops that stand on their own, the restatement it is held to bit for bit and the route it is timed
    against (SCULPT_DISTANCE_FORM=composeddisplacement selects it in TSR.bake_displacement_map): the coverage in torch (bake_scene_surface_composed's) -> bake_interpolate of the positions and of the normals ->
    the covered texels (nonzero: this waits for the device) -> project_along -> scatter into images that are 0 (status -1)
    elsewhere.  Same arguments, same result."""
    planes, v, f, nrm, r, res, want = _bake_displacement_args("bake_displacement_composed", planes, v_pos, faces, normals, rast, target,
                                                              max_dist, steps, res_tol, want)
    dev = r.device
    im = {"height": torch.zeros((res, res), dtype=torch.float32, device=dev),
          "residual": torch.zeros((res, res), dtype=torch.float32, device=dev),
          "status": torch.full((res, res), -1, dtype=torch.int32, device=dev),
          "evals": torch.zeros((res, res), dtype=torch.int32, device=dev)}
    covered, r = _covered_texels(r, v, f)
    idx = covered.reshape(-1).nonzero()[:, 0]
    if idx.numel() > 0:
        pos = bake_interpolate(v, r, f).reshape(-1, 3)[idx].contiguous()
        dirs = bake_interpolate(nrm, r, f).reshape(-1, 3)[idx].contiguous()
        h, got = project_along(planes, mlp, pos, dirs, target, max_dist, steps=steps, res_tol=res_tol, radius=radius,
                               want=("residual", "status", "evals"))
        im["height"].view(-1)[idx] = h
        for k in got:
            im[k].view(-1)[idx] = got[k]
    return im["height"], covered, {k: im[k] for k in want}


def bake_displacement_route():
    """What TSR.bake_displacement_map calls: bake_displacement, the route without a host wait, unless SCULPT_DISTANCE_FORM holds
    the token `composeddisplacement` (then bake_displacement_composed).  The two give the same bits; the no-wait route is the
    default because it is the faster one on the flagship atlases, in both orders (DESIGN.md 3.1h has the figures)."""
    return bake_displacement_composed if _lib.form_has("SCULPT_DISTANCE_FORM", "composeddisplacement") else bake_displacement


def resize_aa_bilinear(img_hwc, size):
    """F.interpolate(bilinear, align_corners=False, antialias=True) to (size, size) on an HWC fp32 device image
    (ImagePreprocessor.convert_and_resize, tsr/utils.py:82-88)."""
    img = _req(img_hwc.contiguous(), torch.float32, "image")
    H, W, C = img.shape
    tmp = torch.empty((H, size, C), dtype=torch.float32, device=img.device)
    out = torch.empty((size, size, C), dtype=torch.float32, device=img.device)
    check(lib.sculpt_resize_aa_bilinear(_ptr(img), H, W, C, _ptr(tmp), _ptr(out), size, size, _stream()))
    return out


# ----------------------------------------------------------------------------------------------
# StableFast geometry tail
# ----------------------------------------------------------------------------------------------
def dilate_fill(img, mask, iterations=10):
    """dilate_fill (sf3d/models/utils.py:96-133): img [1,3,H,W] f32, mask [1,1,H,W] (bool or float) -> [1,3,H,W]."""
    img = _req(img.contiguous(), torch.float32, "img")
    H, W = img.shape[-2:]
    m = _req(mask.to(torch.float32).contiguous(), torch.float32, "mask")
    scratch = torch.empty(8 * H * W, dtype=torch.float32, device=img.device)
    out = torch.empty_like(img)
    check(lib.sculpt_dilate_fill(_ptr(img), _ptr(m), H, W, int(iterations), _ptr(scratch), _ptr(out), _stream()))
    return out


def vertex_normals(v_pos, faces):
    """Mesh._compute_vertex_normal (sf3d/models/mesh.py:66-92)."""
    v = _req(v_pos.contiguous(), torch.float32, "v_pos")
    f = faces.contiguous()
    ws = torch.empty(max(1, int(lib.sculpt_vertex_accumulate_workspace_bytes(v.shape[0]))), dtype=torch.uint8, device=v.device)
    out = torch.empty_like(v)
    check(lib.sculpt_vertex_normals(_ptr(v), v.shape[0], _ptr(f), int(f.dtype == torch.int64), f.shape[0], _ptr(ws), _ptr(out), _stream()))
    return out


def vertex_tangents(v_pos, v_tex, v_nrm, faces):
    """Mesh._compute_vertex_tangent (sf3d/models/mesh.py:94-139)."""
    v = _req(v_pos.contiguous(), torch.float32, "v_pos")
    t = _req(v_tex.contiguous(), torch.float32, "v_tex")
    n = _req(v_nrm.contiguous(), torch.float32, "v_nrm")
    f = faces.contiguous()
    ws = torch.empty(max(1, int(lib.sculpt_vertex_accumulate_workspace_bytes(v.shape[0]))), dtype=torch.uint8, device=v.device)
    out = torch.empty_like(v)
    check(lib.sculpt_vertex_tangents(_ptr(v), _ptr(t), _ptr(n), v.shape[0], _ptr(f), int(f.dtype == torch.int64), f.shape[0],
                                     _ptr(ws), _ptr(out), _stream()))
    return out


# ----------------------------------------------------------------------------------------------
# StableFast-3D networks: 3x3 conv as im2col + GEMM, pixel shuffle, marching tetrahedra
# ----------------------------------------------------------------------------------------------
def im2col3x3(act, n_planes, S, out):
    """act [n_planes*S*S][C] channel-last (bf16 or f32) -> out [n_planes*S*S][9*C], k = (ky*3+kx)*C + c."""
    C = act.shape[1]
    assert act.is_contiguous() and out.is_contiguous() and out.shape == (n_planes * S * S, 9 * C) and out.dtype == act.dtype
    check(lib.sculpt_im2col3x3(_ptr(act), n_planes, S, C, act.element_size(), _ptr(out), _stream()))


def conv3x3_planes(act, n_planes, S, W2, bias, out_f32=None, out_bf16=None, relu=False):
    """3x3 / pad 1 convolution of n_planes S x S channel-last images act [n_planes*S*S][C] (C % 64 == 0), implicit GEMM."""
    C = act.shape[1]
    assert act.is_contiguous() and W2.shape[1] == 9 * C
    o = out_f32 if out_f32 is not None else out_bf16
    check(lib.sculpt_conv3x3_bf16(_ptr(act), act.stride(0), n_planes, S, S, C, 1, _ptr(W2), _ptr(bias), _ptr(out_f32), _ptr(out_bf16),
                                  o.stride(0), 0, W2.shape[0], _lib.EPI_RELU if relu else _lib.EPI_NONE, _stream()))


def resize_bilinear_hwc(image_hwc, size, mul_hw=None, out=None):
    """F.interpolate(bilinear, align_corners=False, no antialias) of an fp32 [H][W][C] image to size x size; every source
    pixel is first multiplied by mul_hw [H][W] when given (sculpt_resize_bilinear_hwc)."""
    H, W, C = image_hwc.shape
    assert image_hwc.dtype == torch.float32 and image_hwc.is_contiguous()
    if mul_hw is not None:
        mul_hw = mul_hw.reshape(H, W)
        assert mul_hw.dtype == torch.float32 and mul_hw.is_contiguous()
    if out is None:
        out = torch.empty((size, size, C), dtype=torch.float32, device=image_hwc.device)
    check(lib.sculpt_resize_bilinear_hwc(_ptr(image_hwc), _ptr(mul_hw), H, W, C, _ptr(out), size, size, _stream()))
    return out


def im2col3x3_strided(act, n_groups, S, stride, out):
    """act [n_groups*S*S][C] channel-last groups (bf16 or f32) -> out [So*So][9*n_groups*C] of the 3x3 / padding 0 /
    stride convolution over the channel-concatenated image, k = (ky*3+kx)*n_groups*C + g*C + c."""
    C = act.shape[1]
    So = (S - 3) // stride + 1
    assert act.is_contiguous() and act.shape[0] == n_groups * S * S and out.is_contiguous() and out.dtype == act.dtype
    assert out.shape == (So * So, 9 * n_groups * C)
    check(lib.sculpt_im2col3x3_strided(_ptr(act), n_groups, S, C, act.element_size(), stride, _ptr(out), _stream()))
    return So


def col_reduce(x, rows, out, mean=False):
    """out[c] = max (or mean) over the first `rows` rows of fp32 x [*, cols] (sculpt_col_reduce_f32)."""
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and x.stride(1) == 1
    assert out.is_contiguous() and out.numel() >= x.shape[1], "col_reduce: out holds fewer than x.shape[1] columns"
    check(lib.sculpt_col_reduce_f32(_ptr(x), x.stride(0), rows, x.shape[1], 1 if mean else 0, _ptr(out), _stream()))
    return out


def pixel_shuffle(g, planes, n_planes, S, Co, r):
    """nn.PixelShuffle(r) of g f32 [n_planes*S*S][>= Co*r*r] into planes f32 [n_planes][Co][S*r][S*r]."""
    g = _req(g, torch.float32, "g")
    check(lib.sculpt_pixel_shuffle(_ptr(g), g.stride(0), _ptr(planes), n_planes, S, Co, r, _stream()))


def normalize_rows3(x, eps=1e-7, out=None):
    """F.normalize(x, dim=-1, eps=eps) for [N,3] fp32; out may be x itself (in place)."""
    x = _req(x.contiguous(), torch.float32, "x")
    y = torch.empty_like(x) if out is None else _req(out, torch.float32, "out")
    assert y.shape == x.shape
    check(lib.sculpt_normalize_rows3(_ptr(x), x.shape[0], float(eps), _ptr(y), _stream()))
    return y


def bake_material(rast, color, perturb_normal=None, nrm=None, tng=None):
    """system.py:375-440 per texel -> (albedo [res,res,3], bump [res,res,3] or None)."""
    res = rast.shape[0]
    rast = _req(rast.contiguous(), torch.float32, "rast")
    albedo = torch.empty((res, res, 3), dtype=torch.float32, device=rast.device)
    bump = torch.empty_like(albedo) if perturb_normal is not None else None
    args = [None if t is None else _req(t.reshape(-1, 3).contiguous(), torch.float32, "texel image")
            for t in (color, perturb_normal, nrm, tng)]
    check(lib.sculpt_bake_material(_ptr(rast), res, _ptr(args[0]), _ptr(args[1]), _ptr(args[2]), _ptr(args[3]),
                                   _ptr(albedo), _ptr(bump), _stream()))
    return albedo, bump


def uv_cell_atlas(v_pos, faces, padding=0.05):
    """One grid cell per triangle (stand-in unwrapper) -> (uv f32 [3*Nf, 2], indices i64 [Nf, 3] = arange)."""
    v = _req(v_pos.contiguous(), torch.float32, "v_pos")
    f = faces.contiguous()
    nf = f.shape[0]
    cols = max(1, int(np.ceil(np.sqrt(nf))))
    rows = max(1, -(-nf // cols))
    uv = torch.empty((3 * nf, 2), dtype=torch.float32, device=v.device)
    check(lib.sculpt_uv_cell_atlas(_ptr(v), _ptr(f), int(f.dtype == torch.int64), nf, cols, rows, float(padding), _ptr(uv),
                                   _stream()))
    return uv, torch.arange(3 * nf, device=v.device, dtype=torch.int64).reshape(-1, 3)


class TetGrid:
    """Static tetrahedral grid tables resident in HBM (see sculptmate_amd/sf3d/tets.py)."""

    def __init__(self, vertices, indices, device, edges=None, tet_edges=None):
        from .sf3d.tets import edge_tables

        v = np.ascontiguousarray(vertices, np.float32)
        t = np.ascontiguousarray(indices, np.int64)
        if edges is None or tet_edges is None:
            edges, tet_edges = edge_tables(t, v.shape[0])
        self.n_vertices, self.n_tets, self.n_edges = v.shape[0], t.shape[0], edges.shape[0]
        self.vertices = torch.from_numpy(v).to(device)
        self.tets = torch.from_numpy(t.astype(np.int32)).to(device)
        self.edges = torch.from_numpy(np.ascontiguousarray(edges, np.int32)).to(device)
        self.tet_edges = torch.from_numpy(np.ascontiguousarray(tet_edges, np.int32)).to(device)
        self.ws = torch.empty(lib.sculpt_mtet_workspace_bytes(self.n_edges, self.n_tets), dtype=torch.uint8, device=device)


def mtet_deform(grid: TetGrid, offsets, resolution):
    """grid_vertices + (1/resolution) * tanh(offsets)  (isosurface.py:108-115)."""
    off = _req(offsets.reshape(-1, 3).contiguous(), torch.float32, "offsets")
    out = torch.empty_like(grid.vertices)
    check(lib.sculpt_mtet_deform(_ptr(grid.vertices), _ptr(off), grid.n_vertices, float((1 - 0) / resolution), _ptr(out),
                                 _stream()))
    return out


def marching_tets(grid: TetGrid, pos, sdf, vert_mul=1.0, vert_add=0.0):
    """MarchingTetrahedraHelper._forward (isosurface.py:142-209) -> (verts f32 [Nv,3] * vert_mul + vert_add, faces i64)."""
    pos = _req(pos.contiguous(), torch.float32, "pos")
    sdf = _req(sdf.reshape(-1).contiguous(), torch.float32, "sdf")
    assert pos.shape == (grid.n_vertices, 3) and sdf.shape[0] == grid.n_vertices
    nv, nf = ctypes.c_int64(), ctypes.c_int64()
    check(lib.sculpt_mtet_count(_ptr(sdf), _ptr(grid.tets), grid.n_tets, _ptr(grid.edges), grid.n_edges, _ptr(grid.ws),
                                ctypes.byref(nv), ctypes.byref(nf), _stream()))
    verts = torch.empty((nv.value, 3), dtype=torch.float32, device=pos.device)
    faces = torch.empty((nf.value, 3), dtype=torch.int64, device=pos.device)
    if nv.value and nf.value:
        check(lib.sculpt_mtet_emit(_ptr(pos), _ptr(sdf), _ptr(grid.tets), grid.n_tets, _ptr(grid.edges), grid.n_edges,
                                   _ptr(grid.tet_edges), _ptr(grid.ws), float(vert_mul), float(vert_add), _ptr(verts),
                                   _ptr(faces), _stream()))
    return verts, faces


# ----------------------------------------------------------------------------------------------
# fp32 parity mode primitives
# ----------------------------------------------------------------------------------------------
def gemm_f32(A, W, bias=None, residual=None, out=None, out_t=None, M=None, N=None, epilogue=0, n_split=0, w_rows=0,
             alpha=1.0, l3=False, batch=1, a_bs=0, w_bs=0, o_bs=0):
    """out[m][n] = epi(alpha * A[m][:] . W[n][:] + bias[n]) (+ residual); fp32 in and out (sculpt_gemm_f32_ex).
    l3=False: the exact-fp32 matrix instruction.  l3=True: fp32 arithmetic on the bf16 matrix pipe through the exact
    three-limb split of both operands (K % 32 == 0).  batch > 1: grid z, entry z at A + z*a_bs, W + z*w_bs, out + z*o_bs."""
    K = A.shape[1]
    if N is None:
        N = W.shape[0] // 2 if epilogue == _lib.EPI_GEGLU else W.shape[0]
    M = A.shape[0] if M is None else M
    check(lib.sculpt_gemm_f32_ex(_ptr(A), A.stride(0), _ptr(W), W.stride(0), _ptr(bias), _ptr(residual),
                                 residual.stride(0) if residual is not None else 0, _ptr(out),
                                 out.stride(0) if out is not None else 0, _ptr(out_t),
                                 out_t.stride(0) if out_t is not None else 0, int(n_split), int(w_rows), M, N, K,
                                 float(alpha), epilogue, _lib.F32_BF16L3 if l3 else _lib.F32_EXACT, int(batch), int(a_bs), int(w_bs),
                                 int(o_bs), _stream()))


LIMB_FORMATS = {"bf16x3": _lib.LIMBS_BF16X3, "f16x2": _lib.LIMBS_F16X2}


class Limbs:
    """An fp32 matrix [rows][cols] held as 16-bit limbs in the limb-tiled layout of csrc/limbs.h: the operand form of `gemm_l3p`
    (weights split once at load time, activations written this way by the kernel that produces them).
    fmt "bf16x3": three bf16 limbs, exact; "f16x2": two fp16 limbs (22 bits, |x| < 65504) -- a weight is then stored times the
    power of two `scale` that puts its largest magnitude in [2^14, 2^15) and the GEMM multiplies by alpha = 1 / scale."""
    __slots__ = ("data", "rows", "cols", "fmt", "scale")

    def __init__(self, rows, cols, device=None, data=None, zero=False, fmt="bf16x3", scale=1.0):
        self.rows, self.cols, self.fmt, self.scale = int(rows), int(cols), fmt, float(scale)
        self.data = data if data is not None else limbs_empty(rows, cols, device, zero=zero, fmt=fmt)

    @staticmethod
    def of(x, fmt="bf16x3", weight=False):
        """weight=True (f16x2 only): stored pre-scaled into the fp16 range (see the class)."""
        scale = 1.0
        if weight and fmt == "f16x2":
            mx = float(x.abs().max())
            if mx > 0.0 and np.isfinite(mx):
                scale = 2.0 ** (14 - int(np.floor(np.log2(mx))))
        return Limbs(x.shape[0], x.shape[1], data=limbs_split(x, fmt=fmt, scale=scale), fmt=fmt, scale=scale)

    @property
    def code(self):
        return LIMB_FORMATS[self.fmt]

    def float(self):
        return limbs_join(self.data, self.rows, self.cols, self.fmt) / self.scale


def limbs_bytes(rows, K, fmt="bf16x3"):
    return int(lib.sculpt_limbs_bytes(int(rows), int(K), LIMB_FORMATS[fmt]))


def limbs_empty(rows, K, device, zero=False, fmt="bf16x3"):
    """An uninitialised limb-tiled [rows][K] matrix (sculpt_limbs_split's layout; a flat uint8 tensor)."""
    return (torch.zeros if zero else torch.empty)(limbs_bytes(rows, K, fmt), dtype=torch.uint8, device=device)


def limbs_split(x, out=None, fmt="bf16x3", scale=1.0):
    """scale * fp32 [rows][K] -> the limb-tiled form the `gemm_l3p` operands take (bf16x3: exact; f16x2: 22 bits)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    rows, K = x.shape
    if out is None:
        out = limbs_empty(rows, K, x.device, fmt=fmt)
    check(lib.sculpt_limbs_split(_ptr(x), x.stride(0), rows, K, float(scale), LIMB_FORMATS[fmt], _ptr(out), _stream()))
    return out


def limbs_join(lt, rows, K, fmt="bf16x3"):
    """The fp32 matrix a limb-tiled array stands for (tests): the sum of the limbs per element."""
    nl = 2 if fmt == "f16x2" else 3
    v = lt.view(torch.float16 if fmt == "f16x2" else torch.bfloat16).view(-1, K // 8, nl, 32, 8).to(torch.float32)   # [block][chunk][limb][row][k]
    x = v[:, :, 0] + v[:, :, 1]
    if nl == 3:
        x = x + v[:, :, 2]                                                         # exact: the limbs do not overlap
    return x.permute(0, 2, 1, 3).reshape(-1, K)[:rows].contiguous()


def geglu_row_blocks(W):
    """A GEGLU weight [2N][K] (value rows, then gate rows) with its 32-row blocks in gemm_l3p's tile order."""
    N = W.shape[0] // 2
    assert N % 64 == 0
    idx = torch.arange(N, device=W.device).view(N // 64, 2, 32)                    # [tile][half][row]
    order = torch.stack([idx[:, 0], idx[:, 0] + N, idx[:, 1], idx[:, 1] + N], 1).reshape(-1)
    return W.index_select(0, order)


def gemm_l3p(A_lt, W_lt, M, N, K, bias=None, residual=None, out=None, out_t=None, n_split=0, out_lt=None, epilogue=0, fmt=None,
             alpha=None):
    """sculpt_gemm_l3p: the limb GEMM on operands split once (A_lt [M][K], W_lt [N or 2N][K] limb-tiled; Limbs or raw tensors
    with fmt / alpha given).  A Limbs weight brings its format and alpha = 1 / scale."""
    if fmt is None:
        fmt = W_lt.fmt if isinstance(W_lt, Limbs) else "bf16x3"
    if alpha is None:
        alpha = 1.0 / (W_lt.scale * (A_lt.scale if isinstance(A_lt, Limbs) else 1.0)) if isinstance(W_lt, Limbs) else 1.0
    out_fmt = out_lt.fmt if isinstance(out_lt, Limbs) else fmt
    rows_w = 2 * N if epilogue == _lib.EPI_GEGLU else N
    for t, r, c, what, f in ((A_lt, M, K, "A", fmt), (W_lt, rows_w, K, "W", fmt), (out_lt, M, N, "out", out_fmt)):
        if isinstance(t, Limbs):
            assert t.cols == c and t.rows >= r and t.fmt == f, "gemm_l3p: %s is a limb-tiled %s [%d][%d], the call needs %s [>= %d][%d]" % (
                what, t.fmt, t.rows, t.cols, f, r, c)
        elif t is not None:
            assert t.numel() * t.element_size() >= limbs_bytes(r, c, f), "gemm_l3p: %s holds fewer bytes than a limb-tiled [%d][%d]" % (what, r, c)
    A_lt, W_lt = getattr(A_lt, "data", A_lt), getattr(W_lt, "data", W_lt)
    out_lt = getattr(out_lt, "data", out_lt)
    check(lib.sculpt_gemm_l3p(_ptr(A_lt), _ptr(W_lt), LIMB_FORMATS[fmt], float(alpha), _ptr(bias), _ptr(residual),
                              residual.stride(0) if residual is not None else 0, _ptr(out), out.stride(0) if out is not None else 0,
                              _ptr(out_t), out_t.stride(0) if out_t is not None else 0, int(n_split), _ptr(out_lt),
                              LIMB_FORMATS[out_fmt], int(M), int(N), int(K), int(epilogue), _stream()))


def softmax_rows_f32(x, rows, cols, pad_cols):
    check(lib.sculpt_softmax_rows_f32(_ptr(x), x.stride(0), rows, cols, pad_cols, _stream()))


def attention_f32_l3_batched(Q, K, Vt, O, Tq, Tk, heads, scale, batch, q_bs, k_bs, vt_bs, o_bs, two_fp16_limbs=False):
    """`batch` fused three-limb attentions in one launch (sculpt_attention_f32_l3_batched); O an fp32 tensor (o_bs in elements) or a
    Limbs (o_bs in elements of its logical [rows][cols] matrix: entry b starts at row b * o_bs / cols)."""
    lt = isinstance(O, Limbs)
    if lt:
        assert o_bs % O.cols == 0
    check(lib.sculpt_attention_f32_l3_batched(_ptr(Q), Q.stride(0), int(q_bs), _ptr(K), K.stride(0), int(k_bs), _ptr(Vt), Vt.stride(0),
                                              int(vt_bs), None if lt else _ptr(O), 0 if lt else O.stride(0), 0 if lt else int(o_bs),
                                              _ptr(O.data) if lt else None, O.code if lt else 0, 0, int(o_bs // O.cols) if lt else 0,
                                              O.cols if lt else 0,
                                              Tq, Tk, heads, int(batch), float(scale), 1 if two_fp16_limbs else 0, _stream()))


def attention_f32(Q, K, Vt, O, Tq, Tk, heads, scale, scores, l3=False, o_row0=0, two_fp16_limbs=False):
    """softmax(Q K^T scale) V per head in fp32: two GEMMs and a row softmax per head.
    Q [Tq][*], K [Tk][*] with head h at columns 64h..; Vt [heads*64][>= round_up(Tk,32)] (zero padded).
    scores: fp32 scratch.  [Tq][>= round_up(Tk,32)]: the heads run one after the other (three launches each);
    [heads][Tq][>= round_up(Tk,32)]: all heads at once, three launches per attention (grid z = head).
    l3: the two products on the three-limb bf16 matrix pipe (gemm_f32 l3=True) instead of the exact-fp32 instruction;
    with scores=None (l3 only) the whole attention is ONE fused launch (sculpt_attention_f32_l3): what TSR(precision="bf16l3") runs."""
    Tkp = ((Tk + 31) // 32) * 32 if l3 else ((Tk + 15) // 16) * 16
    N4 = ((Tk + 3) // 4) * 4
    if scores is None:   # the fused kernel of the three-limb mode: no score matrix in HBM
        assert l3, "the exact-fp32 attention is a composition: it needs the scores scratch"
        if isinstance(O, Limbs):   # the output as limbs: row o_row0 + q of the limb-tiled matrix O
            check(lib.sculpt_attention_f32_l3_limbs(_ptr(Q), Q.stride(0), _ptr(K), K.stride(0), _ptr(Vt), Vt.stride(0), _ptr(O.data),
                                                    O.code, int(o_row0), O.cols, Tq, Tk, heads, float(scale), 1 if two_fp16_limbs else 0,
                                                    _stream()))
            return
        if two_fp16_limbs:   # fp32 output through the batched entry (one entry)
            return attention_f32_l3_batched(Q, K, Vt, O, Tq, Tk, heads, scale, 1, 0, 0, 0, 0, two_fp16_limbs=True)
        check(lib.sculpt_attention_f32_l3(_ptr(Q), Q.stride(0), _ptr(K), K.stride(0), _ptr(Vt), Vt.stride(0), _ptr(O), O.stride(0),
                                          Tq, Tk, heads, float(scale), _stream()))
        return
    if scores.dim() == 3:
        assert scores.shape[0] >= heads and scores.shape[1] == Tq and scores.is_contiguous()
        ld = scores.shape[2]
        flat = scores.view(-1, ld)
        gemm_f32(Q[:, :64], K[:, :64], out=flat, M=Tq, N=N4, w_rows=Tk, alpha=scale, l3=l3, batch=heads, a_bs=64, w_bs=64, o_bs=Tq * ld)
        softmax_rows_f32(flat, heads * Tq, Tk, Tkp)
        gemm_f32(flat[:, :Tkp], Vt[:64, :Tkp], out=O[:, :64], M=Tq, N=64, l3=l3, batch=heads, a_bs=Tq * ld, w_bs=64 * Vt.stride(0), o_bs=64)
        return
    for h in range(heads):
        q, k = Q[:, 64 * h:64 * h + 64], K[:, 64 * h:64 * h + 64]
        gemm_f32(q, k, out=scores, M=Tq, N=N4, w_rows=Tk, alpha=scale, l3=l3)
        softmax_rows_f32(scores, Tq, Tk, Tkp)
        gemm_f32(scores[:, :Tkp], Vt[64 * h:64 * h + 64, :Tkp], out=O[:, 64 * h:64 * h + 64], M=Tq, N=64, l3=l3)


# ----------------------------------------------------------------------------------------------
# channel-last bf16 conv-net blocks (U^2-Net)
# ----------------------------------------------------------------------------------------------
class Act:
    """A slice [H*W][C] of a channel-last bf16 activation buffer (buf: [H*W, ld] bf16, channels off..off+C)."""

    def __init__(self, buf, off, C, H, W):
        assert buf.dtype == BF16 and buf.is_contiguous() and buf.shape[0] == H * W and off % 8 == 0 and C % 8 == 0
        assert off + C <= buf.shape[1]
        self.buf, self.off, self.C, self.H, self.W = buf, off, C, H, W

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 2 * self.off)

    @property
    def ld(self):
        return self.buf.stride(0)


def conv3x3_bf16(x: Act, W2, bias, out, n_store, dilation, relu, col=None, implicit=None):
    """Conv2d(3x3, padding=dilation, dilation) of the slice x with packed weights W2 [Npad][9*C_pad] (+bias [Npad]).
    out: an Act (bf16 slice, n_store columns written) or an fp32 tensor [H*W, Npad].
    implicit (default: whenever the slice has C_pad readable channels per pixel): no im2col rows, the GEMM fetches the
    shifted pixels itself (sculpt_conv3x3_bf16); otherwise im2col into `col` (bf16 scratch >= H*W*9*C_pad) + GEMM."""
    K = W2.shape[1]
    C_pad = K // 9
    M = x.H * x.W
    assert W2.dtype == BF16
    epi = _lib.EPI_RELU if relu else _lib.EPI_NONE
    can = x.off + C_pad <= x.buf.shape[1] and C_pad % 64 == 0
    if implicit is None:
        implicit = can
    if implicit:
        assert can, "implicit conv needs C_pad readable channels in the slice's rows"
        if isinstance(out, Act):
            check(lib.sculpt_conv3x3_bf16(x.ptr, x.ld, 1, x.H, x.W, C_pad, int(dilation), _ptr(W2), _ptr(bias), None, out.ptr,
                                          out.ld, int(n_store), W2.shape[0], epi, _stream()))
        else:
            check(lib.sculpt_conv3x3_bf16(x.ptr, x.ld, 1, x.H, x.W, C_pad, int(dilation), _ptr(W2), _ptr(bias), _ptr(out), None,
                                          out.stride(0), 0, W2.shape[0], epi, _stream()))
        return
    assert col is not None and col.numel() >= M * K
    check(lib.sculpt_im2col3x3_dilated(x.ptr, x.ld, x.H, x.W, x.C, C_pad, int(dilation), _ptr(col), _stream()))
    if isinstance(out, Act):
        check(lib.sculpt_gemm_bf16_ex(_ptr(col), K, _ptr(W2), K, _ptr(bias), None, 0, None, out.ptr, out.ld, None, 0, 0,
                                      int(n_store), M, W2.shape[0], K, epi, _stream()))
    else:
        check(lib.sculpt_gemm_bf16_ex(_ptr(col), K, _ptr(W2), K, _ptr(bias), None, 0, _ptr(out), None, out.stride(0), None, 0,
                                      0, 0, M, W2.shape[0], K, epi, _stream()))


def maxpool2x2_ceil(x: Act, out: Act):
    assert out.H == (x.H + 1) // 2 and out.W == (x.W + 1) // 2 and out.C == x.C
    check(lib.sculpt_maxpool2x2_ceil(x.ptr, x.ld, x.H, x.W, x.C, out.ptr, out.ld, _stream()))


def upsample_bilinear(x: Act, out: Act):
    assert out.C == x.C
    check(lib.sculpt_upsample_bilinear_bf16(x.ptr, x.ld, x.H, x.W, x.C, out.ptr, out.ld, out.H, out.W, _stream()))


def upsample_bilinear_f32(x, ld, h, w, out, H, W):
    check(lib.sculpt_upsample_bilinear_f32(_ptr(x), int(ld), h, w, _ptr(out), H, W, _stream()))


def add_bf16(a: Act, b: Act, out: Act):
    assert a.C == b.C == out.C and a.H * a.W == out.H * out.W
    check(lib.sculpt_add_bf16(a.ptr, a.ld, b.ptr, b.ld, out.ptr, out.ld, a.H * a.W, a.C, _stream()))


def fuse_sigmoid(maps, w, bias, out):
    check(lib.sculpt_fuse_sigmoid(_ptr(maps), maps.shape[0], maps.shape[1], _ptr(w), float(bias), _ptr(out), _stream()))


# ----------------------------------------------------------------------------------------------
# image front end: uint8 HWC images resident in HBM (csrc/image_front.hip; bit for bit the host library's results)
# ----------------------------------------------------------------------------------------------
def lanczos_tables_host(in_size, out_size):
    """Pillow's 8-bit LANCZOS tables of one axis (sculpt_resample_lanczos_*; host only, no GPU) ->
    (ksize, bounds int32 [out_size, 2] = (first input index, taps used), kk int32 [out_size, ksize])."""
    ksize = lib.sculpt_resample_lanczos_ksize(int(in_size), int(out_size))
    if ksize <= 0:
        raise SculptError("lanczos tables: sizes %r -> %r are out of range" % (in_size, out_size))
    bounds = np.empty((out_size, 2), np.int32)
    kk = np.empty((out_size, ksize), np.int32)
    check(lib.sculpt_resample_lanczos_coeffs(int(in_size), int(out_size), ksize, bounds.ctypes.data, kk.ctypes.data))
    return ksize, bounds, kk


_LANCZOS_TABLES = {}   # (device, in_size, out_size) -> (ksize, bounds, kk) on the device; the oldest entry leaves past 64


def _lanczos_tables(in_size, out_size, device):
    key = (str(device), int(in_size), int(out_size))
    hit = _LANCZOS_TABLES.get(key)
    if hit is None:
        ksize, bounds, kk = lanczos_tables_host(in_size, out_size)
        hit = (ksize, torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device))
        if len(_LANCZOS_TABLES) >= 64:
            _LANCZOS_TABLES.pop(next(iter(_LANCZOS_TABLES)))
        _LANCZOS_TABLES[key] = hit
    return hit


def resample_lanczos_u8(img, out_h, out_w):
    """Image.resize((out_w, out_h), LANCZOS) of an 8-bit image: uint8 [H, W, C] (C in 1, 3, 4; every channel alike) or [H, W]."""
    img = _req(img, torch.uint8, "image")
    flat = img.dim() == 2
    H, W = img.shape[:2]
    C = 1 if flat else img.shape[2]
    out_h, out_w = int(out_h), int(out_w)
    kx, bx, cx = _lanczos_tables(W, out_w, img.device) if W != out_w else (0, None, None)
    ky, by, cy = _lanczos_tables(H, out_h, img.device) if H != out_h else (0, None, None)
    tmp = torch.empty((H, out_w, C), dtype=torch.uint8, device=img.device) if (kx and ky) else None
    out = torch.empty((out_h, out_w) if flat else (out_h, out_w, C), dtype=torch.uint8, device=img.device)
    check(lib.sculpt_resample_u8(_ptr(img), H, W, C, _ptr(bx), _ptr(cx), kx, _ptr(by), _ptr(cy), ky, _ptr(tmp), _ptr(out), out_h, out_w,
                                 _stream()))
    return out


def u2net_input(img, mean, std):
    """rembg's normalize() after its resize: uint8 [H, W, 3 or 4] -> fp32 [3, H, W] = ((v / max - mean) / std in float64).astype(float32)."""
    img = _req(img, torch.uint8, "image")
    H, W, C = img.shape
    ws = torch.empty(4, dtype=torch.int32, device=img.device)
    out = torch.empty((3, H, W), dtype=torch.float32, device=img.device)
    m, s = (ctypes.c_double * 3)(*mean), (ctypes.c_double * 3)(*std)
    check(lib.sculpt_u2net_input(_ptr(img), H, W, C, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), _ptr(ws), _ptr(out),
                                 _stream()))
    return out


def u2net_mask(d0):
    """rembg's min-max stretch of the network output to 8 bits: fp32 [...] -> uint8 [...] (a constant d0 gives 0)."""
    d0 = _req(d0, torch.float32, "d0")
    ws = torch.empty(4, dtype=torch.int32, device=d0.device)
    out = torch.empty(d0.shape, dtype=torch.uint8, device=d0.device)
    check(lib.sculpt_u2net_mask(_ptr(d0), d0.numel(), _ptr(ws), _ptr(out), _stream()))
    return out


def cutout_bbox(img, mask):
    """(ymin, ymax, xmin, xmax), both ends inclusive, of the non-zero alpha of Image.composite(img, transparent, mask); None when
    the cut-out is empty.  img uint8 [H, W, 3 or 4], mask uint8 [H, W].  Four integers come back to the host: the call waits for
    them (an event behind the copy), not for the stream."""
    img, mask = _req(img, torch.uint8, "image"), _req(mask, torch.uint8, "mask")
    H, W, C = img.shape
    if tuple(mask.shape) != (H, W):
        raise SculptError("cutout_bbox: mask %s for a %d x %d image" % (tuple(mask.shape), H, W))
    ws = torch.empty(4, dtype=torch.int32, device=img.device)
    box = (ctypes.c_int32 * 4)()
    check(lib.sculpt_cutout_bbox(_ptr(img), _ptr(mask), H, W, C, _ptr(ws), ctypes.cast(box, ctypes.c_void_p), _stream()))
    return None if box[1] < 0 else (box[0], box[1], box[2], box[3])


def cutout_frame(img, mask, y0, x0, h, w, top, left, side, grey):
    """The cut-out's box [y0, y0 + h) x [x0, x0 + w) placed at (top, left) of a transparent side x side frame: uint8 [side, side, 4],
    or with grey=True composited on 0.5 grey as preprocess_image does: uint8 [side, side, 3]."""
    img, mask = _req(img, torch.uint8, "image"), _req(mask, torch.uint8, "mask")
    H, W, C = img.shape
    if tuple(mask.shape) != (H, W):
        raise SculptError("cutout_frame: mask %s for a %d x %d image" % (tuple(mask.shape), H, W))
    out = torch.empty((side, side, 3 if grey else 4), dtype=torch.uint8, device=img.device)
    if side > 0:
        check(lib.sculpt_cutout_frame(_ptr(img), _ptr(mask), H, W, C, int(y0), int(x0), int(h), int(w), int(top), int(left), int(side),
                                      1 if grey else 0, _ptr(out), _stream()))
    return out


def u8_to_unit_f32(x):
    """uint8 -> fp32 v / 255 (ImagePreprocessor's conversion of an 8-bit image)."""
    x = _req(x, torch.uint8, "image")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if x.numel():
        check(lib.sculpt_u8_to_unit_f32(_ptr(x), x.numel(), _ptr(out), _stream()))
    return out
