"""Time the occlusion bake over an atlas (csrc/mesh_ray.hip sculpt_bake_occlusion, ops.bake_occlusion) on the meshes it is meant
for: the 256^3 mesh of the full-size TSR with seeded weights (the HIGH mesh), simplify=0.1 of it (the LOW mesh) and the low
mesh's atlas at 2048^2, 64 directions.

    python tools/time_occlusion_map.py [--runs 7] [--warmup 2] [--res 2048] [--k 64] [--out profiles/time_occlusion_map.json]

Two cases, each the fused kernel against the composed route (ops.bake_occlusion_composed's stages) on the same inputs and the
same prebuilt index, whose bits it must equal:
    self     the low mesh against itself (no snap)
    source   the low mesh against the high mesh with the default cage (2^-6 of the longest side of the high mesh's bounds)
Reported beside the times: the covered texels, the share of them that snapped onto the source and the share that fell back,
the index build of each surface, and the peak device memory each route allocates on top of its inputs.

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; median and quartiles over
the runs (the quartiles are the run-to-run spread).  No threshold is set here."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

MC_RES, THRESHOLD, SIMPLIFY = 256, 25.0, 0.1


def _bits(t):
    return t.view(torch.int32)


def peak_extra(fn):
    """Peak bytes fn allocates on top of what is live when it starts (the caching allocator's own count)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_occlusion_map.json"))
    a = ap.parse_args()
    import numpy as np

    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.system import Mesh

    dev = torch.device("cuda:0")
    model, code, high = seeded_mesh(dev, MC_RES, THRESHOLD)
    lv, lf = ops.mesh_simplify(high.vertices, high.faces, SIMPLIFY)[:2]
    with torch.no_grad():
        (v, f, uv, rast), atlas = timed(lambda: model._atlas(Mesh(lv, lf), a.res, 0.02, None), 1, 0)
    nrm = (TSR.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
    dirs = torch.from_numpy(ops.occlusion_directions(a.k, 0)).to(dev)
    covered = int((rast[..., 3] >= 0).sum())
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "resolution": a.res,
              "directions": a.k, "high": {"vertices": int(high.vertices.shape[0]), "faces": int(high.faces.shape[0])},
              "low": {"vertices": int(v.shape[0]), "faces": int(f.shape[0])}, "covered_texels": covered,
              "unwrap_and_rasterise": atlas}
    # how the fused kernel's 32 x 32 tiles fill their waves: the covered texels of a tile are compacted, 64 to a wave
    tiles = -(-a.res // 32)
    grid = torch.zeros((tiles * 32, tiles * 32), dtype=torch.int64, device=dev)
    grid[:a.res, :a.res] = (rast[..., 3] >= 0).long()
    per_tile = grid.view(tiles, 32, tiles, 32).sum((1, 3)).reshape(-1)
    waves = int(((per_tile + 63) // 64).sum())
    result["tiles"] = {"all": tiles * tiles, "with_texels": int((per_tile > 0).sum()), "full": int((per_tile == 1024).sum()),
                       "waves": waves, "wave_fill": covered / (64.0 * max(waves, 1)), "waves_of_a_global_list": -(-covered // 64)}
    print("high %d faces, low %d faces, atlas %d^2, %d covered texels (%.1f%%), %d rays at most; %d of %d tiles hold texels, %d waves "
          "at %.1f%% fill (a global list: %d)" % (
              high.faces.shape[0], f.shape[0], a.res, covered, 100.0 * covered / (a.res * a.res), covered * a.k,
              result["tiles"]["with_texels"], tiles * tiles, waves, 100.0 * result["tiles"]["wave_fill"], -(-covered // 64)), flush=True)

    ok = True
    for case, surface in (("self", (v, f)), ("source", (high.vertices, high.faces))):
        P, F = ops._surface(surface[0], surface[1], "time_occlusion_map")
        index, build = timed(lambda: ops._SurfaceIndex(P, F), a.runs, a.warmup)
        index.records()
        longest = index.longest_side()
        offset = float(np.float32(ops.OCCLUSION_OFFSET * longest))
        cage = 0.0 if case == "self" else float(np.float32(ops.OCCLUSION_CAGE * longest))
        args = (index, v, f, nrm, rast, dirs, offset, math.inf, cage)
        fused, t_fused = timed(lambda: ops._bake_occlusion_fused(*args), a.runs, a.warmup)
        comp, t_comp = timed(lambda: ops._bake_occlusion_composed(*args), max(1, min(a.runs, 5)), 1)
        same = torch.equal(_bits(fused[0]), _bits(comp[0])) and torch.equal(fused[1], comp[1])
        ok = ok and same
        entry = {"index_build": build, "fused": t_fused, "composed": t_comp, "same_bits": same,
                 "composed_over_fused": t_comp["median_ms"] / t_fused["median_ms"], "cage": cage, "offset": offset,
                 "mean_ao": float(fused[0][fused[1]].nanmean()), "nan_texels": int(torch.isnan(fused[0]).sum()),
                 "peak_extra_bytes": {"fused": peak_extra(lambda: ops._bake_occlusion_fused(*args)),
                                      "composed": peak_extra(lambda: ops._bake_occlusion_composed(*args))}}
        if cage > 0.0:
            at = torch.nonzero(fused[1].reshape(-1))[:, 0]
            pts = ops.bake_interpolate(v, rast, f).reshape(-1, 3)[at].contiguous()
            nr = ops.bake_interpolate(nrm, rast, f).reshape(-1, 3)[at].contiguous()
            hit = ops._snap_composed(index, pts, nr, cage, want_stats=True)[2]
            entry["snapped_share"] = float(hit.float().mean())
            entry["fell_back_share"] = 1.0 - entry["snapped_share"]
        result[case] = entry
        print("%s: fused %.3f ms (%.3f .. %.3f), composed %.3f ms (%.3f .. %.3f), ratio %.2f, same bits: %s; index build %.3f ms; "
              "peak extra memory fused %.1f MB, composed %.1f MB; mean ao %.4f%s" % (
                  case, t_fused["median_ms"], t_fused["q1_ms"], t_fused["q3_ms"], t_comp["median_ms"], t_comp["q1_ms"], t_comp["q3_ms"],
                  entry["composed_over_fused"], same, build["median_ms"], entry["peak_extra_bytes"]["fused"] / 1e6,
                  entry["peak_extra_bytes"]["composed"] / 1e6, entry["mean_ao"],
                  "; snapped %.2f%%, fell back %.2f%% (cage %.5f)" % (100 * entry["snapped_share"], 100 * entry["fell_back_share"], cage)
                  if cage > 0.0 else ""), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))
    assert ok, "the fused and the composed route differ"


if __name__ == "__main__":
    main()
