"""Time TSR.bake_texture stage by stage on a 256^3 mesh of a synthetic model, at 2048^2 and 1024^2, and the colour stage twice:
the fused kernel (ops.bake_scene_color) against the composed route of the parent commit (ops.bake_interpolate followed by
ops.triplane_query over ALL texels on channel-last planes: what sf3d/bake.py does), on the same box and in the same process.

    python tools/time_bake_texture.py [--runs 21] [--warmup 3] [--out profiles/time_bake_texture.json]

The model is the full-size TSR with seeded weights (its density bias shifted so that the default threshold gives a surface, as
bench.py does); the mesh is extract_meshes at 256^3 of one synthetic picture.  Every figure is wall clock around the stage
including a final torch.cuda.synchronize(), after warm-up calls, as the median over the runs with the quartiles beside it.  Both
colour routes read the same rasterised atlas and the same channel-last planes (converted once, outside the timed region), and
their results are compared on the covered texels before anything is timed.  The covered share of the atlas is reported next to
the times: the fused kernel skips what the composed route evaluates and throws away.
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
MC_RES, THRESHOLD = 256, 25.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--island-padding", type=float, default=0.02)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_bake_texture.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d.unwrap import BoxProjectionUnwrapper

    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    v, f = mesh.vertices, mesh.faces
    radius = model.renderer.cfg.radius
    planes = ops.ChannelLastPlanes(code)
    unwrap = BoxProjectionUnwrapper()
    corner = torch.arange(3 * f.shape[0], device=dev, dtype=torch.int32).view(-1, 3)
    f32 = f.to(torch.int32)   # bake_interpolate takes int32 indices: converted once, outside the timed region
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
              "island_padding": a.island_padding, "decoder_hidden_layers": int(model.decoder.n_hidden), "resolutions": {}}
    nrm = ops.vertex_normals(v, f)
    uv, _ = unwrap(v, nrm, f, a.island_padding)
    shared = {"normals": timed(lambda: ops.vertex_normals(v, f), a.runs, a.warmup)[1],
              "unwrap": timed(lambda: unwrap(v, nrm, f, a.island_padding), a.runs, a.warmup)[1]}
    result["mesh_stages"] = shared
    print("mesh: %d vertices, %d faces; normals %.3f ms, unwrap %.3f ms" % (v.shape[0], f.shape[0], shared["normals"]["median_ms"],
                                                                           shared["unwrap"]["median_ms"]), flush=True)
    for res in RESOLUTIONS:
        rast = ops.bake_rasterize(uv, corner, res)
        covered = rast[..., 3] >= 0
        share = float(covered.float().mean())

        def fused():
            return ops.bake_scene_color(planes, model.decoder, v, f, rast, radius=radius)

        def composed():
            pos = ops.bake_interpolate(v, rast, f32)
            return ops.triplane_query(planes, model.decoder, pos.reshape(-1, 3), radius=radius, want=("color",))["color"]

        color, mask = fused()
        ref = composed().view(res, res, 3)
        same = bool(torch.equal(color[covered], ref[covered])) and bool(torch.equal(mask, covered)) and not bool(color[~covered].any())
        it = res // 150
        planar = color.permute(2, 0, 1)[None].contiguous()
        entry = {"covered_share": round(share, 4), "covered_texels": int(covered.sum()), "texels": res * res,
                 "fused_equals_composed_on_covered_texels": same,
                 "rasterise": timed(lambda: ops.bake_rasterize(uv, corner, res), a.runs, a.warmup)[1],
                 "colour_fused": timed(fused, a.runs, a.warmup)[1],
                 "colour_composed": timed(composed, a.runs, a.warmup)[1],
                 "padding": timed(lambda: ops.dilate_fill(planar, mask[None, None], iterations=it), a.runs, a.warmup)[1],
                 "padding_iterations": it,
                 "bake_texture_whole_call": timed(lambda: model.bake_texture(mesh, code, res, a.island_padding), a.runs, a.warmup)[1]}
        # the colour stage once more in the other order: the second of two routes must not owe its time to the first one's caches
        entry["colour_composed_again"] = timed(composed, a.runs, a.warmup)[1]
        entry["colour_fused_again"] = timed(fused, a.runs, a.warmup)[1]
        result["resolutions"][str(res)] = entry
        print("%d^2: covered %.1f %%; rasterise %.3f ms, colour fused %.3f ms (again %.3f), composed %.3f ms (again %.3f), padding %.3f ms, "
              "whole call %.3f ms, identical %s" % (res, 100 * share, entry["rasterise"]["median_ms"], entry["colour_fused"]["median_ms"],
                                                    entry["colour_fused_again"]["median_ms"], entry["colour_composed"]["median_ms"],
                                                    entry["colour_composed_again"]["median_ms"], entry["padding"]["median_ms"],
                                                    entry["bake_texture_whole_call"]["median_ms"], same), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
