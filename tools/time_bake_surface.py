"""Time the bake at the surface on the 256^3 mesh of the seeded model after simplify=0.1, at 1024^2 and 2048^2, project=True:
the fused kernel (ops.bake_scene_surface) against the composed route (ops.bake_scene_surface_composed), both in one process and
the pair once more in the opposite order; against the plain ops.bake_scene_normal on the same atlas (what projecting costs); the
colour query over the projected points; and the whole TSR.bake_surface_maps against TSR.bake_texture + TSR.bake_normal_map.

    python tools/time_bake_surface.py [--runs 21] [--warmup 3] [--out profiles/time_bake_surface.json]

Every figure is wall clock around the stage including a final torch.cuda.synchronize(), after warm-up calls, as the median over
the runs with the quartiles beside it.  Both routes read the same rasterised atlas, the same frames and the same channel-last
planes (made once, outside the timed region), and their outputs are compared bit for bit before anything is timed.  Beside the
times: evaluations per texel, the status histogram, |d - t| before and after, the displacement in lattice cells, and the angle
between the normal baked at the texel's own point and the one baked at the projected point -- how much the feature changes the
map.  `fused_is_default_by_the_rule`: the fused median below the composed first quartile in both orders (DESIGN.md 3.1e's rule).
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

RESOLUTIONS = [1024, 2048]
MC_RES, THRESHOLD, SIMPLIFY, PROJECT = 256, 25.0, 0.1, True
WANT = ("residual", "status", "evals")


def _same(a, b):
    return bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--island-padding", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_bake_surface.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d.unwrap import BoxProjectionUnwrapper

    dev = torch.device("cuda:0")
    model, code, full = seeded_mesh(dev, MC_RES, THRESHOLD)
    mesh = full.simplify(SIMPLIFY)
    v, f = mesh.vertices, mesh.faces
    cfg = model.renderer.cfg
    radius = cfg.radius
    steps, cells = ops.project_rule(PROJECT)
    target = float(np.float32(math.log(THRESHOLD) - float(cfg.density_bias)))
    cell = 2.0 * float(radius) / (MC_RES - 1)
    max_dist = cells * cell
    planes = ops.ChannelLastPlanes(code)
    unwrap = BoxProjectionUnwrapper()
    corner = torch.arange(3 * f.shape[0], device=dev, dtype=torch.int32).view(-1, 3)
    uv, idx = unwrap(v, ops.vertex_normals(v, f), f, a.island_padding)
    uv = uv.to(torch.float32)[idx.reshape(-1).long()].contiguous()
    cn = (model.WINDING_OUTWARD * ops.vertex_normals(v, f))[f.reshape(-1).long()].contiguous()
    ct = ops.corner_tangents(v, f, uv, cn)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "project": [steps, cells],
              "faces_before_simplify": int(full.faces.shape[0]), "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
              "island_padding": a.island_padding, "target": target, "max_dist": max_dist, "res_tol": ops.PROJECT_RES_TOL,
              "decoder_hidden_layers": int(model.decoder.n_hidden), "resolutions": {}}
    for res in RESOLUTIONS:
        rast = ops.bake_rasterize(uv, corner, res)
        covered = rast[..., 3] >= 0
        kw = dict(steps=steps, radius=radius, frame=(cn, ct), want=WANT)   # every output, in both routes: the same work is timed

        def fused(**over):
            return ops.bake_scene_surface(planes, model.decoder, v, f, rast, target, max_dist, **dict(kw, **over))

        def composed(**over):
            return ops.bake_scene_surface_composed(planes, model.decoder, v, f, rast, target, max_dist, **dict(kw, **over))

        def plain():
            return ops.bake_scene_normal(planes, model.decoder, v, f, rast, radius=radius, frame=(cn, ct))

        # what is compared and described, before anything is timed
        same = {}
        for space, frame in (("tangent", (cn, ct)), ("object", None)):
            x, y = fused(frame=frame), composed(frame=frame)
            same[space] = all([_same(x[0], y[0]), _same(x[1], y[1]), _same(x[2], y[2])] + [_same(x[3][k], y[3][k]) for k in WANT])
        point, world, mask, ex = x                                   # object space, steps as timed
        p0, world0, _, ex0 = fused(frame=None, steps=0)
        status = ex["status"][mask]
        r, r0 = ex["residual"][mask].abs(), ex0["residual"][mask].abs()
        moved = (point[mask] - p0[mask]).double().norm(dim=1) / cell
        a64, b64 = world[mask].double(), world0[mask].double()
        both = (a64.norm(dim=1) > 0) & (b64.norm(dim=1) > 0)
        angle = 2.0 * torch.atan2((a64 - b64).norm(dim=1), (a64 + b64).norm(dim=1))[both]
        pts = point[mask].contiguous()

        def colour():
            return ops.triplane_query(planes, model.decoder, pts, radius=radius, density_bias=cfg.density_bias, want=("color",))["color"]

        def maps_at_the_surface():
            return model.bake_surface_maps(mesh, code, threshold=THRESHOLD, project=PROJECT, resolution=MC_RES, atlas_resolution=res,
                                           island_padding=a.island_padding)

        def maps_on_the_face():
            return model.bake_normal_map(model.bake_texture(mesh, code, res, a.island_padding), code, island_padding=a.island_padding)

        entry = {"covered_share": round(float(covered.float().mean()), 4), "covered_texels": int(covered.sum()), "texels": res * res,
                 "fused_equals_composed_bit_for_bit": same,
                 "mean_evals_per_covered_texel": round(float(ex["evals"][mask].float().mean()), 4),
                 "status_histogram": np.bincount(status.cpu().numpy(), minlength=4).tolist(),
                 "abs_residual_median_before": float(r0.median()), "abs_residual_median_after": float(r.median()),
                 "displacement_cells_median": float(moved.median()), "displacement_cells_max": float(moved.max()),
                 "normal_angle_rad_median": float(angle.median()), "normal_angle_rad_p95": float(np.percentile(angle.cpu().numpy(), 95)),
                 "fused": timed(fused, a.runs, a.warmup)[1],
                 "composed": timed(composed, a.runs, a.warmup)[1]}
        # the pair once more in the opposite order: the second of two routes must not owe its time to the first one's caches
        entry["composed_again"] = timed(composed, a.runs, a.warmup)[1]
        entry["fused_again"] = timed(fused, a.runs, a.warmup)[1]
        entry["fused_is_default_by_the_rule"] = bool(entry["fused"]["median_ms"] < entry["composed"]["q1_ms"]
                                                     and entry["fused_again"]["median_ms"] < entry["composed_again"]["q1_ms"])
        entry["fused_steps_0"] = timed(lambda: fused(steps=0), a.runs, a.warmup)[1]
        entry["plain_bake_scene_normal"] = timed(plain, a.runs, a.warmup)[1]
        entry["colour_query_at_projected_points"] = timed(colour, a.runs, a.warmup)[1]
        entry["bake_surface_maps_whole_call"] = timed(maps_at_the_surface, a.runs, a.warmup)[1]
        entry["bake_texture_plus_bake_normal_map"] = timed(maps_on_the_face, a.runs, a.warmup)[1]
        result["resolutions"][str(res)] = entry
        print("%d^2: covered %.1f %%; fused %.3f ms (again %.3f), composed %.3f ms q1 %.3f (again %.3f q1 %.3f) -> default by the rule: "
              "%s; plain normal bake %.3f ms, fused with 0 steps %.3f ms; colour query %.3f ms; bake_surface_maps %.3f ms, bake_texture + "
              "bake_normal_map %.3f ms; evals %.2f, status %s; |d - t| median %.3e -> %.3e; moved median %.3f max %.3f cells; "
              "normal turned median %.4f p95 %.4f rad; equal bits %s" % (
                  res, 100 * entry["covered_share"], entry["fused"]["median_ms"], entry["fused_again"]["median_ms"],
                  entry["composed"]["median_ms"], entry["composed"]["q1_ms"], entry["composed_again"]["median_ms"],
                  entry["composed_again"]["q1_ms"], entry["fused_is_default_by_the_rule"], entry["plain_bake_scene_normal"]["median_ms"],
                  entry["fused_steps_0"]["median_ms"], entry["colour_query_at_projected_points"]["median_ms"],
                  entry["bake_surface_maps_whole_call"]["median_ms"], entry["bake_texture_plus_bake_normal_map"]["median_ms"],
                  entry["mean_evals_per_covered_texel"], entry["status_histogram"], entry["abs_residual_median_before"],
                  entry["abs_residual_median_after"], entry["displacement_cells_median"], entry["displacement_cells_max"],
                  entry["normal_angle_rad_median"], entry["normal_angle_rad_p95"], same), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
