"""Time the displacement bake on the 256^3 mesh of the seeded model after simplify=0.1, at 1024^2 and 2048^2, displacement=True:
the route without a host wait (ops.bake_displacement: texel list on the device + line search over it) against the composed route
(ops.bake_displacement_composed), both in one process and the pair once more in the opposite order; ops.project_along against
the rule restated with one torch call per operation (tests/_dispref.py composed_device) on the same covered texels; the list
kernel alone; the whole TSR.bake_displacement_map; and beside them ops.bake_scene_surface_composed and the plain
ops.bake_scene_normal on the same atlas.

    python tools/time_bake_displacement.py [--runs 21] [--warmup 3] [--out profiles/time_bake_displacement.json]

Every figure is wall clock around the stage including a final torch.cuda.synchronize(), after warm-up calls, as the median over
the runs with the quartiles beside it.  Both routes read the same rasterised atlas, normals and channel-last planes (made once,
outside the timed region), and their outputs are compared bit for bit before anything is timed.  Beside the times: the status
histogram, evaluations per texel and the median |d - t| before and after.  `list_route_is_default_by_the_rule`: the no-wait
route's median below the composed first quartile in both orders (DESIGN.md 3.1e's rule).
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

RESOLUTIONS = [1024, 2048]
MC_RES, THRESHOLD, SIMPLIFY, DISPLACEMENT = 256, 25.0, 0.1, True
WANT = ("residual", "status", "evals")


def _same(a, b):
    return bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--island-padding", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_bake_displacement.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    import _dispref

    from sculptmate_amd import ops
    from sculptmate_amd.sf3d.unwrap import BoxProjectionUnwrapper

    dev = torch.device("cuda:0")
    model, code, full = seeded_mesh(dev, MC_RES, THRESHOLD)
    mesh = full.simplify(SIMPLIFY)
    v, f = mesh.vertices, mesh.faces
    cfg = model.renderer.cfg
    radius = cfg.radius
    steps, cells = ops.displacement_rule(DISPLACEMENT)
    target = float(np.float32(math.log(THRESHOLD) - float(cfg.density_bias)))
    cell = 2.0 * float(radius) / (MC_RES - 1)
    max_dist = cells * cell
    planes = ops.ChannelLastPlanes(code)
    corner = torch.arange(3 * f.shape[0], device=dev, dtype=torch.int32).view(-1, 3)
    uv, idx = BoxProjectionUnwrapper()(v, ops.vertex_normals(v, f), f, a.island_padding)
    uv = uv.to(torch.float32)[idx.reshape(-1).long()].contiguous()
    normals = (model.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
    baked = mesh._derive(mesh.vertices, mesh.faces, uvs=uv)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "displacement": [steps, cells],
              "faces_before_simplify": int(full.faces.shape[0]), "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
              "island_padding": a.island_padding, "target": target, "max_dist": max_dist, "res_tol": ops.PROJECT_RES_TOL,
              "decoder_hidden_layers": int(model.decoder.n_hidden), "resolutions": {}}
    for res in RESOLUTIONS:
        rast = ops.bake_rasterize(uv, corner, res)
        kw = dict(steps=steps, radius=radius, want=WANT)   # every output, in both routes: the same work is timed

        def listed(**over):
            return ops.bake_displacement(planes, model.decoder, v, f, normals, rast, target, max_dist, **dict(kw, **over))

        def composed(**over):
            return ops.bake_displacement_composed(planes, model.decoder, v, f, normals, rast, target, max_dist, **dict(kw, **over))

        x, y = listed(), composed()
        same = all([_same(x[0], y[0]), _same(x[1], y[1])] + [_same(x[2][k], y[2][k]) for k in WANT])
        height, mask, ex = x
        r0 = listed(steps=0)[2]["residual"][mask].abs()
        r = ex["residual"][mask].abs()
        status = ex["status"][mask]
        got = ops.bake_texel_list(v, f, rast, normals=normals)
        n = int(got["count"].item())
        pts, dirs = got["p0"][:n].contiguous(), got["directions"][:n].contiguous()

        def along():
            return ops.project_along(planes, model.decoder, pts, dirs, target, max_dist, steps=steps, radius=radius, want=WANT)

        def along_composed():
            return _dispref.composed_device(ops, planes, model.decoder, pts, dirs, target, steps, max_dist, ops.PROJECT_RES_TOL, radius=radius)

        h1, e1 = along()
        h2 = along_composed()
        same_rule = all(_same(p, q) for p, q in zip((h1, e1["residual"], e1["status"], e1["evals"]), h2))
        cn = normals[f.reshape(-1).long()].contiguous()
        ct = ops.corner_tangents(v, f, uv, cn)

        entry = {"covered_share": round(float(mask.float().mean()), 4), "covered_texels": int(mask.sum()), "texels": res * res,
                 "list_route_equals_composed_bit_for_bit": same, "project_along_equals_the_composed_rule_bit_for_bit": same_rule,
                 "mean_evals_per_covered_texel": round(float(ex["evals"][mask].float().mean()), 4),
                 "status_histogram": np.bincount(status.cpu().numpy(), minlength=4).tolist(),
                 "abs_residual_median_before": float(r0[torch.isfinite(r0)].median()), "abs_residual_median_after": float(r[torch.isfinite(r)].median()),
                 "abs_height_cells_median": float(height[mask].abs().median()) / cell,
                 "list_route": timed(listed, a.runs, a.warmup)[1],
                 "composed": timed(composed, a.runs, a.warmup)[1]}
        # the pair once more in the opposite order: the second of two routes must not owe its time to the first one's caches
        entry["composed_again"] = timed(composed, a.runs, a.warmup)[1]
        entry["list_route_again"] = timed(listed, a.runs, a.warmup)[1]
        entry["list_route_is_default_by_the_rule"] = bool(entry["list_route"]["median_ms"] < entry["composed"]["q1_ms"]
                                                          and entry["list_route_again"]["median_ms"] < entry["composed_again"]["q1_ms"])
        entry["project_along"] = timed(along, a.runs, a.warmup)[1]
        entry["composed_device_rule"] = timed(along_composed, a.runs, a.warmup)[1]
        entry["texel_list_alone"] = timed(lambda: ops.bake_texel_list(v, f, rast, normals=normals), a.runs, a.warmup)[1]
        entry["bake_displacement_map_whole_call"] = timed(
            lambda: model.bake_displacement_map(baked, code, threshold=THRESHOLD, displacement=DISPLACEMENT, resolution=MC_RES,
                                                atlas_resolution=res), a.runs, a.warmup)[1]
        entry["bake_scene_surface_composed"] = timed(
            lambda: ops.bake_scene_surface_composed(planes, model.decoder, v, f, rast, target, cell, steps=8, radius=radius, frame=(cn, ct),
                                                    want=WANT), a.runs, a.warmup)[1]
        entry["plain_bake_scene_normal"] = timed(
            lambda: ops.bake_scene_normal(planes, model.decoder, v, f, rast, radius=radius, frame=(cn, ct)), a.runs, a.warmup)[1]
        result["resolutions"][str(res)] = entry
        print("%d^2: covered %.1f %%; list route %.3f ms (again %.3f), composed %.3f ms q1 %.3f (again %.3f q1 %.3f) -> default by the "
              "rule: %s; project_along %.3f ms, composed_device %.3f ms; texel list alone %.3f ms; bake_displacement_map %.3f ms; "
              "bake_scene_surface_composed %.3f ms, plain normal bake %.3f ms; evals %.2f, status %s; |d - t| median %.3e -> %.3e; "
              "equal bits %s / %s" % (
                  res, 100 * entry["covered_share"], entry["list_route"]["median_ms"], entry["list_route_again"]["median_ms"],
                  entry["composed"]["median_ms"], entry["composed"]["q1_ms"], entry["composed_again"]["median_ms"],
                  entry["composed_again"]["q1_ms"], entry["list_route_is_default_by_the_rule"], entry["project_along"]["median_ms"],
                  entry["composed_device_rule"]["median_ms"], entry["texel_list_alone"]["median_ms"],
                  entry["bake_displacement_map_whole_call"]["median_ms"], entry["bake_scene_surface_composed"]["median_ms"],
                  entry["plain_bake_scene_normal"]["median_ms"], entry["mean_evals_per_covered_texel"], entry["status_histogram"],
                  entry["abs_residual_median_before"], entry["abs_residual_median_after"], same, same_rule), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
