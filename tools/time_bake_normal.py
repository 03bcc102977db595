"""Time TSR.bake_normal_map stage by stage on the 256^3 mesh of the seeded model after simplify=0.1, at 2048^2 and 1024^2, and the
normal stage twice: the fused kernel (ops.bake_scene_normal) against the composed route (ops.bake_interpolate, ops.field_normals
over ALL texels on channel-last planes, and for the tangent space the frame transform in torch), on the same box and in the same
process.

    python tools/time_bake_normal.py [--runs 21] [--warmup 3] [--out profiles/time_bake_normal.json]

Every figure is wall clock around the stage including a final torch.cuda.synchronize(), after warm-up calls, as the median over
the runs with the quartiles beside it.  Both routes read the same rasterised atlas, the same frames and the same channel-last
planes (made once, outside the timed region); the world normals of the two are compared bit for bit on the covered texels, and
the largest difference to the torch frame transform (whose roundings are torch's, not the kernel's) is reported, before anything
is timed.  The covered share
of the atlas is reported next to the times: the fused kernel skips what the composed route evaluates and throws away.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

RESOLUTIONS = [2048, 1024]
MC_RES, THRESHOLD, SIMPLIFY = 256, 25.0, 0.1


def frame_transform_torch(n, rast, cn, ct):
    """The composed route's last step: world normals [R,R,3] -> tangent-space vectors, whole image, in torch."""
    t = rast[..., 3].clamp(min=0).long()
    b = rast[..., :3]
    N = (cn.view(-1, 3, 3)[t] * b[..., None]).sum(-2)
    T = (ct.view(-1, 3, 4)[t][..., :3] * b[..., None]).sum(-2)
    B = ct.view(-1, 3, 4)[t][..., 0, 3:4] * torch.cross(N, T, dim=-1)
    gtt, gnn, gtn = (T * T).sum(-1), (N * N).sum(-1), (T * N).sum(-1)
    nT, nN, nB = (n * T).sum(-1), (n * N).sum(-1), (n * B).sum(-1)
    s = torch.stack([nT * gnn - nN * gtn, nB, nN * gtt - nT * gtn], -1)
    return torch.nn.functional.normalize(s, dim=-1) * (rast[..., 3:4] >= 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--island-padding", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_bake_normal.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d.unwrap import BoxProjectionUnwrapper

    dev = torch.device("cuda:0")
    model, code, full = seeded_mesh(dev, MC_RES, THRESHOLD)
    mesh = full.simplify(SIMPLIFY)
    v, f = mesh.vertices, mesh.faces
    radius = model.renderer.cfg.radius
    planes = ops.ChannelLastPlanes(code)
    unwrap = BoxProjectionUnwrapper()
    corner = torch.arange(3 * f.shape[0], device=dev, dtype=torch.int32).view(-1, 3)
    f32 = f.to(torch.int32)   # bake_interpolate takes int32 indices: converted once, outside the timed region
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "faces_before_simplify": int(full.faces.shape[0]),
              "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "island_padding": a.island_padding,
              "decoder_hidden_layers": int(model.decoder.n_hidden), "resolutions": {}}
    nrm = ops.vertex_normals(v, f)
    uv, idx = unwrap(v, nrm, f, a.island_padding)
    uv = uv.to(torch.float32)[idx.reshape(-1).long()].contiguous()

    def corner_normals():
        return (model.WINDING_OUTWARD * ops.vertex_normals(v, f))[f.reshape(-1).long()].contiguous()

    cn = corner_normals()
    ct = ops.corner_tangents(v, f, uv, cn)
    result["mesh_stages"] = {"unwrap": timed(lambda: unwrap(v, nrm, f, a.island_padding), a.runs, a.warmup)[1],
                             "corner_normals": timed(corner_normals, a.runs, a.warmup)[1],
                             "corner_tangents": timed(lambda: ops.corner_tangents(v, f, uv, cn), a.runs, a.warmup)[1]}
    result["mirrored_corner_share"] = round(float((ct[:, 3] < 0).float().mean()), 4)
    print("mesh: %d faces of %d; unwrap %.3f ms, corner normals %.3f ms, corner tangents %.3f ms" % (
        f.shape[0], full.faces.shape[0], *[result["mesh_stages"][k]["median_ms"] for k in ("unwrap", "corner_normals", "corner_tangents")]),
        flush=True)
    for res in RESOLUTIONS:
        rast = ops.bake_rasterize(uv, corner, res)
        covered = rast[..., 3] >= 0
        share = float(covered.float().mean())

        def fused(frame=(cn, ct)):
            return ops.bake_scene_normal(planes, model.decoder, v, f, rast, radius=radius, frame=frame)

        def composed_world():
            pos = ops.bake_interpolate(v, rast, f32)
            return ops.field_normals(planes, model.decoder, pos, radius=radius)["normal"]

        def composed():
            return frame_transform_torch(composed_world(), rast, cn, ct)

        world, mask = fused(None)
        tangent, _ = fused()
        same_world = bool(torch.equal(world[covered], composed_world()[covered])) and bool(torch.equal(mask, covered)) and not bool(world[~covered].any())
        diff = float((tangent[covered] - composed()[covered]).abs().max())
        it = res // 150
        planar = (0.5 + 0.5 * tangent).permute(2, 0, 1)[None].contiguous()
        entry = {"covered_share": round(share, 4), "covered_texels": int(covered.sum()), "texels": res * res,
                 "world_normals_equal_composed_on_covered_texels": same_world, "tangent_max_abs_diff_to_torch_transform": diff,
                 "rasterise": timed(lambda: ops.bake_rasterize(uv, corner, res), a.runs, a.warmup)[1],
                 "normal_fused_tangent": timed(fused, a.runs, a.warmup)[1],
                 "normal_fused_object": timed(lambda: fused(None), a.runs, a.warmup)[1],
                 "normal_composed_tangent": timed(composed, a.runs, a.warmup)[1],
                 "normal_composed_object": timed(composed_world, a.runs, a.warmup)[1],
                 "padding": timed(lambda: ops.dilate_fill(planar, mask[None, None], iterations=it), a.runs, a.warmup)[1],
                 "padding_iterations": it,
                 "bake_normal_map_whole_call": timed(lambda: model.bake_normal_map(mesh, code, res, "tangent", a.island_padding), a.runs, a.warmup)[1]}
        # the normal stage once more in the other order: the second of two routes must not owe its time to the first one's caches
        entry["normal_composed_tangent_again"] = timed(composed, a.runs, a.warmup)[1]
        entry["normal_fused_tangent_again"] = timed(fused, a.runs, a.warmup)[1]
        result["resolutions"][str(res)] = entry
        print("%d^2: covered %.1f %%; rasterise %.3f ms; tangent: fused %.3f ms (again %.3f), composed %.3f ms (again %.3f); object: fused "
              "%.3f ms, composed %.3f ms; padding %.3f ms, whole call %.3f ms; world normals identical %s, torch transform within %.2g" % (
                  res, 100 * share, entry["rasterise"]["median_ms"], entry["normal_fused_tangent"]["median_ms"],
                  entry["normal_fused_tangent_again"]["median_ms"], entry["normal_composed_tangent"]["median_ms"],
                  entry["normal_composed_tangent_again"]["median_ms"], entry["normal_fused_object"]["median_ms"],
                  entry["normal_composed_object"]["median_ms"], entry["padding"]["median_ms"],
                  entry["bake_normal_map_whole_call"]["median_ms"], same_world, diff), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
