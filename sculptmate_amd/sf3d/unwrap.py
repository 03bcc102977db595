"""Box-projection UV unwrapping on the MI355X: the reference's `Unwrapper` (StableFast/sf3d/uv_unwrapper/unwrap.py:12-697)
as a callable with the hook signature Mesh.unwrap_uv expects,

    unwrapper(v_pos [Nv,3], v_nrm [Nv,3], faces [Nf,3], island_padding) -> (uv [3*Nf, 2], indices [Nf, 3]).

Stages (each one HIP entry point, csrc/uv_unwrap.hip; the reference lines are cited there and in include/sculpt_hip.h):
principal-axis alignment -> projection onto the six cube faces -> per-chart rotation into a consistent tangent frame ->
atlas assignment (front layer / overlap slice / remaining) -> placement in the 3x2 (+ half-size 6x... ) atlas.

Differences from the reference, stated once:
  * the principal axes are the exact eigenvectors of the vertex covariance (3x3 eigen-decomposition on the host from
    nine device-side sums); the reference's randomised rank-2 torch.pca_lowrank lands within ~15 degrees of them.  Signs:
    each axis points to its larger-magnitude side (deterministic);
  * the atlas assignment is the library's own z-buffer algorithm (the reference's lives in uv_unwrapper.dll);
  * (uv, indices) are returned per corner -- indices = arange(3*Nf) -- instead of torch.unique's sorted unique rows plus
    inverse (:529-544): Mesh.unwrap_uv only ever forms uv[indices], which is identical, and the sort is skipped.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _lib
from ..ops import _ptr, _stream, check, lib


def principal_axes(sums9, n):
    """Nine sums (x, y, z, xx, xy, xz, yy, yz, zz) -> (main, secondary) unit eigenvectors of the covariance, float64."""
    s = np.asarray(sums9, np.float64)
    mu = s[:3] / n
    m2 = np.array([[s[3], s[4], s[5]], [s[4], s[6], s[7]], [s[5], s[7], s[8]]]) / n
    cov = m2 - np.outer(mu, mu)
    w, vec = np.linalg.eigh(cov)
    axes = []
    for k in (2, 1):
        a = vec[:, k]
        if a[np.abs(a).argmax()] < 0:
            a = -a
        axes.append(a)
    return axes[0], axes[1]


def axis_rotation(main_axis, secondary_axis):
    """unwrap.py:566-617: orthonormalise (main, secondary, main x secondary) in float32 and sort the three onto the
    canonical axes they point along (a clash is resolved in favour of the stronger axes) -> row-major 3x3 float32."""
    f = np.float32

    def unit(v):
        return (v / max(f(np.sqrt((v * v).sum(dtype=f))), f(1e-6))).astype(f)

    a = unit(np.asarray(main_axis, f))
    b = np.asarray(secondary_axis, f)
    b = unit(b - (b * a).sum(dtype=f) * a)
    c = unit(np.cross(a, b).astype(f))
    where = [int(np.abs(v).argmax()) for v in (a, b, c)]
    for fix in (2, 1):                      # move the third axis first, then the second (it contributed less to the shape)
        if len(set(where)) == 3:
            break
        where[fix] = ({0, 1, 2} - set(where)).pop()
    if len(set(where)) != 3:
        raise ValueError("Could not find 3 unique axis")
    rows = [None] * 3
    for v, k in zip((a, b, c), where):
        rows[k] = v
    return np.stack(rows, 0).astype(f)


class BoxProjectionUnwrapper:
    """Callable UV unwrapper; keeps its scratch buffers between calls.  `raster_resolution`: pixels per chart side of the
    overlap test's z-buffer."""

    def __init__(self, raster_resolution: int = 1024):
        self.raster_resolution = int(raster_resolution)
        self._buf = {}
        self.last = {}     # per-stage tensors of the last call (chart, assigned, rotation, angles): read by tests / tools

    def _b(self, name, shape, dtype, dev):
        key = (name, tuple(shape), dtype, str(dev))
        t = self._buf.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
            self._buf = {k: v for k, v in self._buf.items() if k[0] != name}
            self._buf[key] = t
        return t

    # ---- stages -------------------------------------------------------------------------------------------------
    def rotation(self, v_pos):
        sums = self._b("sums9", (9,), torch.float64, v_pos.device)
        ws = self._b("moments_ws", (int(lib.sculpt_uv_moments_workspace_bytes()),), torch.uint8, v_pos.device)
        check(lib.sculpt_uv_moments(_ptr(v_pos), v_pos.shape[0], _ptr(sums), _ptr(ws), _stream()))
        main, second = principal_axes(sums.cpu().numpy(), v_pos.shape[0])
        return axis_rotation(main, second)

    def box_project(self, v_pos, v_nrm, faces, rot):
        dev, nv, nf = v_pos.device, v_pos.shape[0], faces.shape[0]
        st = self._b("stats", (int(lib.sculpt_uv_stats_words()),), torch.int32, dev)
        rp = self._b("rot_pos", (nv, 3), torch.float32, dev)
        rn = self._b("rot_nrm", (nv, 3), torch.float32, dev)
        uv = self._b("face_uv", (nf, 3, 2), torch.float32, dev)
        chart = self._b("chart", (nf,), torch.int32, dev)
        r9 = (ctypes.c_float * 9)(*[float(x) for x in np.asarray(rot, np.float32).reshape(-1)])
        check(lib.sculpt_uv_box_project(_ptr(v_pos), _ptr(v_nrm), nv, _ptr(faces), int(faces.dtype == torch.int64), nf,
                                        ctypes.cast(r9, ctypes.c_void_p), _ptr(rp), _ptr(rn), _ptr(uv), _ptr(chart), _ptr(st), _stream()))
        return rp, rn, uv, chart, st

    def chart_angles(self, rp, rn, faces, uv, chart):
        dev, nv, nf = rp.device, rp.shape[0], faces.shape[0]
        vt = self._b("vtan", (nv, 4), torch.float32, dev)
        sums = self._b("sums42", (6, 7), torch.float64, dev)
        ws = self._b("tangent_ws", (int(lib.sculpt_uv_chart_tangents_workspace_bytes(nv)),), torch.uint8, dev)
        check(lib.sculpt_uv_chart_tangents(_ptr(rp), _ptr(rn), nv, _ptr(faces), int(faces.dtype == torch.int64), nf, _ptr(uv), _ptr(chart),
                                           _ptr(vt), _ptr(sums), _ptr(ws), _stream()))
        s = sums.cpu().numpy()
        angles = np.zeros(6, np.float32)
        for c in range(6):
            if s[c, 6] == 0:
                continue
            a = (s[c, 0:3] / s[c, 6]).astype(np.float32)
            e = (s[c, 3:6] / s[c, 6]).astype(np.float32)
            # :350-355: atan2(cross_z, dot) of the two mean tangents (3-D dot, 2-D cross)
            angles[c] = np.float32(math.atan2(float(a[0] * e[1] - a[1] * e[0]), float((a * e).sum(dtype=np.float32))))
        return angles, vt

    def rotate_charts(self, uv, chart, angles, st):
        co = (ctypes.c_float * 6)(*[float(np.float32(math.cos(float(a)))) for a in angles])
        si = (ctypes.c_float * 6)(*[float(np.float32(math.sin(float(a)))) for a in angles])
        check(lib.sculpt_uv_rotate_charts(_ptr(uv), _ptr(chart), uv.shape[0], ctypes.cast(co, ctypes.c_void_p),
                                          ctypes.cast(si, ctypes.c_void_p), _ptr(st), _stream()))
        return uv

    def assign_atlas(self, rp, faces, uv, chart):
        dev, nf, res = rp.device, faces.shape[0], self.raster_resolution
        zbuf = self._b("zbuf", (6 * res * res,), torch.int64, dev)
        assigned = self._b("assigned", (nf,), torch.int32, dev)
        check(lib.sculpt_uv_assign_atlas(_ptr(rp), _ptr(faces), int(faces.dtype == torch.int64), nf, _ptr(uv), _ptr(chart), res,
                                         _ptr(zbuf), _ptr(assigned), _stream()))
        return assigned

    def place(self, uv, assigned, island_padding, st, out=None):
        dev, nf = uv.device, uv.shape[0]
        scratch = self._b("blocks", ((nf + 255) // 256,), torch.int32, dev)
        if out is None:
            out = torch.empty((nf * 3, 2), dtype=torch.float32, device=dev)
        check(lib.sculpt_uv_place(_ptr(uv), _ptr(assigned), nf, float(island_padding), _ptr(st), _ptr(scratch), _ptr(out), _stream()))
        return out

    # ---- Unwrapper.forward ---------------------------------------------------------------------------------------
    def __call__(self, vertex_positions, vertex_normals, triangle_idxs, island_padding, rot=None, assigned=None):
        """`rot` (3x3) / `assigned` ([Nf] int32 on the device) override the two stages that are not pinned to the reference
        (used by the parity tests to feed both sides the same values)."""
        v = vertex_positions
        if v.device.type != "cuda":
            raise _lib.SculptError("BoxProjectionUnwrapper runs on an MI355X only (device %s; there is no CPU fallback)" % v.device)
        v = v.to(torch.float32).contiguous()
        n = vertex_normals.to(torch.float32).contiguous()
        f = triangle_idxs.contiguous()
        if f.dtype not in (torch.int32, torch.int64):
            raise _lib.SculptError("BoxProjectionUnwrapper: faces must be int32 or int64")
        if f.shape[0] == 0:
            return torch.zeros((0, 2), dtype=torch.float32, device=v.device), f.reshape(0, 3)
        rot = self.rotation(v) if rot is None else np.asarray(rot, np.float32)
        rp, rn, uv, chart, st = self.box_project(v, n, f, rot)
        angles, _ = self.chart_angles(rp, rn, f, uv, chart)
        self.rotate_charts(uv, chart, angles, st)
        if assigned is None:
            assigned = self.assign_atlas(rp, f, uv, chart)
        placed = self.place(uv, assigned, island_padding, st)
        self.last = dict(rot=rot, angles=angles, chart=chart, assigned=assigned, face_uv=uv, rot_pos=rp, rot_nrm=rn)
        indices = torch.arange(3 * f.shape[0], device=v.device, dtype=f.dtype).reshape(-1, 3)
        return placed, indices


class ChartUnwrapper:
    """Callable UV unwrapper whose charts are CONNECTED pieces of surface, however many layers the object has (csrc/uv_charts.hip;
    the rule is stated in include/sculpt_hip.h under "UV CHART ATLAS" and restated in tests/_chartref.py).  The hook signature of
    BoxProjectionUnwrapper: unwrapper(v_pos, v_nrm, faces, island_padding) -> (uv f32 [3*Nf, 2], indices [Nf, 3] = arange); the
    normals are not used.  Per round: faces of one axis direction and one layer that share a manifold, consistently wound edge
    form a chart (union-find) -> per-chart rectangles -> shelf pack, gutter island_padding / GUTTER_DIVISOR -> place -> the
    placed UVs rasterised twice at `raster_resolution` (lowest / highest face wins); a face strictly overlapping a lower one
    moves up a layer, from `max_layers` on it is a chart of its own.  At most MAX_ROUNDS rounds.  The host reads eight integers
    per round; no rectangle or UV crosses to it.  Two calls give the same bits.
    `last` (tests, tools): direction, layer, chart int32 [Nf]; rect f32 [n_charts, 4] (pmin, pmax, qmin, qmax); extent f64
    [n_charts, 2]; cell int64 [n_charts, 2]; scale (float); n_charts, rows, rounds (int); evicted (list, per round); conflicts."""

    GUTTER_DIVISOR = 8.0   # gutter = island_padding / 8 in UV units: 5 texels at 2048^2 for the default 0.02
    MAX_ROUNDS = 8

    def __init__(self, raster_resolution: int = 1024, max_layers: int = 4):
        self.raster_resolution = int(raster_resolution)
        self.max_layers = int(max_layers)
        if self.raster_resolution < 1 or self.max_layers < 0:
            raise ValueError("ChartUnwrapper: raster_resolution must be positive and max_layers >= 0")
        self.last = {}
        self.stage_ms = None   # tools set a dict: every stage then ends with a synchronise and adds its wall time (ms) here

    def _mark(self, name):
        if self.stage_ms is not None:
            import time

            torch.cuda.synchronize()
            now = time.perf_counter()
            if name is not None:
                self.stage_ms[name] = self.stage_ms.get(name, 0.0) + (now - self._t0) * 1e3
            self._t0 = now

    def _round(self, a, mode):
        """Steps 2 .. 6 once -> the header's eight words (one read-back)."""
        from .. import ops

        nf, s, dev = a["nf"], _stream(), a["F"].device
        check(lib.sculpt_uv_chart_label(_ptr(a["skeys"]), _ptr(a["sperm"]), _ptr(a["F"]), nf, _ptr(a["direction"]), _ptr(a["layer"]),
                                        self.max_layers, _ptr(a["label"]), _ptr(a["ws"]), s))
        check(lib.sculpt_uv_chart_rects(_ptr(a["pq"]), _ptr(a["label"]), nf, _ptr(a["chart"]), _ptr(a["rect"]), _ptr(a["extent"]),
                                        _ptr(a["sort_key"]), _ptr(a["ws"]), s))
        self._mark("charts_and_rectangles")
        order = torch.sort(a["sort_key"], stable=True).indices
        self._mark("sort")
        check(lib.sculpt_uv_chart_pack(_ptr(order), _ptr(a["extent"]), nf, a["gutter"], _ptr(a["cell"]), _ptr(a["ws"]), s))
        self._mark("pack")
        check(lib.sculpt_uv_chart_place(_ptr(a["pq"]), _ptr(a["chart"]), _ptr(a["rect"]), _ptr(a["cell"]), nf, a["gutter"], _ptr(a["ws"]),
                                        _ptr(a["uv"]), s))
        self._mark("place")
        low = ops.bake_rasterize(a["uv"], a["corners"], self.raster_resolution)
        high = ops.bake_rasterize(a["uv"], a["corners_reversed"], self.raster_resolution)
        self._mark("rasterise_twice")
        check(lib.sculpt_uv_chart_conflicts(_ptr(low), _ptr(high), self.raster_resolution, _ptr(a["uv"]), _ptr(a["chart"]), nf,
                                            _ptr(a["evicted"]), _ptr(a["chart_conflict"]), _ptr(a["ws"]), s))
        check(lib.sculpt_uv_chart_evict(_ptr(a["evicted"]), _ptr(a["chart_conflict"]), _ptr(a["chart"]), nf, self.max_layers, mode,
                                        _ptr(a["layer"]), _ptr(a["ws"]), s))
        words = a["ws"][:64].view(torch.int64).cpu()
        self._mark("conflicts_and_read_back")
        hdr = dict(n_charts=int(words[0]), evicted=int(words[1]), error=int(words[2]), rows=int(words[3]), evaluations=int(words[4]),
                   scale=float(words[5:6].view(torch.float64)[0]), conflict_texels=int(words[6]))
        if hdr["error"] & 1:
            raise _lib.SculptError("ChartUnwrapper: a union-find walk ran out of its step budget: a defect, the result is not valid")
        if hdr["error"] & 2:
            raise _lib.SculptError("ChartUnwrapper: no scale packs %d charts with a gutter of %g: lower island_padding"
                                   % (hdr["n_charts"], a["gutter"]))
        return hdr

    def __call__(self, vertex_positions, vertex_normals, triangle_idxs, island_padding):
        from .. import ops

        v, f = vertex_positions, triangle_idxs
        if not (isinstance(v, torch.Tensor) and v.is_cuda):
            raise _lib.SculptError("ChartUnwrapper runs on an MI355X only (device %s; there is no CPU fallback)"
                                   % (v.device if isinstance(v, torch.Tensor) else type(v).__name__))
        if not isinstance(f, torch.Tensor) or f.dtype not in (torch.int32, torch.int64):
            raise _lib.SculptError("ChartUnwrapper: faces must be int32 or int64")
        gutter = float(island_padding) / self.GUTTER_DIVISOR
        if not (0.0 <= gutter < 0.5):
            raise ValueError("ChartUnwrapper: island_padding %r (0 <= island_padding < %g)" % (island_padding, 0.5 * self.GUTTER_DIVISOR))
        dev = v.device
        if f.shape[0] == 0:
            self.last = {}
            return torch.zeros((0, 2), dtype=torch.float32, device=dev), f.reshape(0, 3)
        self._mark(None)
        P, F = ops._surface(v, f, "ChartUnwrapper")   # index out of range, non-finite position: SculptError
        self._mark("input_check")
        nv, nf = P.shape[0], F.shape[0]
        size = int(lib.sculpt_uv_chart_workspace_bytes(nf))
        if size == 0:
            raise _lib.SculptError("ChartUnwrapper: %d faces (fewer than 2^24: the rasteriser carries face ids in fp32)" % nf)
        s = _stream()
        i32 = dict(dtype=torch.int32, device=dev)
        a = dict(nf=nf, F=F, gutter=gutter, ws=torch.empty(size, dtype=torch.uint8, device=dev),
                 direction=torch.empty(nf, **i32), layer=torch.zeros(nf, **i32), label=torch.empty(nf, **i32),
                 chart=torch.empty(nf, **i32), evicted=torch.empty(nf, **i32), chart_conflict=torch.empty(nf, **i32),
                 pq=torch.empty((nf, 3, 2), dtype=torch.float32, device=dev), rect=torch.empty((nf, 4), dtype=torch.float32, device=dev),
                 extent=torch.empty((nf, 2), dtype=torch.float64, device=dev), sort_key=torch.empty(nf, dtype=torch.int64, device=dev),
                 cell=torch.zeros((nf, 2), dtype=torch.int64, device=dev), uv=torch.empty((3 * nf, 2), dtype=torch.float32, device=dev))
        a["corners"] = torch.arange(3 * nf, **i32).view(-1, 3)
        a["corners_reversed"] = a["corners"].flip(0).contiguous()
        check(lib.sculpt_uv_chart_directions(_ptr(P), nv, _ptr(F), nf, _ptr(a["direction"]), _ptr(a["pq"]), s))
        keys = torch.empty(3 * nf, dtype=torch.int64, device=dev)   # the half-edge table of the remesh passes
        check(lib.sculpt_rmd_halfedge_keys(_ptr(F), nf, _ptr(keys), s))
        a["skeys"], a["sperm"] = torch.sort(keys, stable=True)
        self._mark("directions_and_half_edges")
        evicted, conflicts = [], 0
        for r in range(self.MAX_ROUNDS):
            hdr = self._round(a, 1 if r == self.MAX_ROUNDS - 1 else 0)
            evicted.append(hdr["evicted"])
            if hdr["evicted"] == 0:
                break
        else:   # the cap: the conflicting charts went to pieces; one last pack and test
            hdr = self._round(a, 2)
            conflicts = hdr["evicted"]
        n = hdr["n_charts"]
        self.last = dict(direction=a["direction"], layer=a["layer"], chart=a["chart"], rect=a["rect"][:n], extent=a["extent"][:n],
                         cell=a["cell"][:n], scale=hdr["scale"], n_charts=n, rows=hdr["rows"], rounds=len(evicted), evicted=evicted,
                         conflicts=conflicts, evaluations=hdr["evaluations"])
        return a["uv"], torch.arange(3 * nf, device=dev, dtype=f.dtype).reshape(-1, 3)
