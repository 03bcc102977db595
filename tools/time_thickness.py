"""Time the wall-thickness queries (csrc/mesh_ray.hip sculpt_surface_thickness, ops.mesh_thickness / bake_thickness) on the meshes
they are meant for -- extract_meshes at 256^3 of the full-size TSR with seeded weights (the HIGH mesh), simplify=0.1 of it (the
LOW mesh) and the low mesh's atlas at 2048^2.

    python tools/time_thickness.py [--runs 5] [--warmup 1] [--k 32] [--res 2048] [--out profiles/time_thickness.json]

Timed, each on a prebuilt index (the grid build is reported beside it):
    high     the fused kernel (one launch) at k rays over the high mesh's own vertices against the composed route on the same
             inputs and the same grid (one closest-hit query per direction with its own sort, the back-face gather and the
             reductions in torch: the loop of ops.mesh_thickness_composed), whose bits it must equal
    low      the same on the low mesh
    bake     ops.bake_thickness of the low mesh against itself over its atlas at `res`^2 (coverage, two interpolations, the point
             kernel over the global cell-sorted list of texels, the scatter)
What the numbers say about the mesh: the share of vertices with no valid ray, the mean valid rays per vertex, the median of
`thinnest` and the share of vertices whose thinnest ray is shorter than one lattice cell of the extraction.

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; median and quartiles over
the runs.  No threshold is set here."""
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
FORM = "SCULPT_DISTANCE_FORM"


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--composed-runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_thickness.json"))
    a = ap.parse_args()
    import numpy as np

    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.system import Mesh

    os.environ.pop(FORM, None)
    dev = torch.device("cuda:0")
    model, code, high = seeded_mesh(dev, MC_RES, THRESHOLD)
    lv, lf = ops.mesh_simplify(high.vertices, high.faces, SIMPLIFY)[:2]
    cell = 2.0 * float(model.renderer.cfg.radius) / (MC_RES - 1)
    dirs = torch.from_numpy(ops.thickness_directions(a.k, ops.THICKNESS_CONE, 0)).to(dev)
    outward = float(TSR.WINDING_OUTWARD)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "rays": a.k,
              "cone": ops.THICKNESS_CONE, "lattice_cell": cell}
    ok = True
    for case, (v, f) in (("high", (high.vertices, high.faces)), ("low", (lv, lf))):
        P, F = ops._surface(v, f, "time_thickness")
        index, build = timed(lambda: ops._SurfaceIndex(P, F), a.runs, a.warmup)
        index.records()
        nrm = (outward * ops.vertex_normals(P, F)).contiguous()
        offset = float(np.float32(ops.OCCLUSION_OFFSET * index.longest_side()))
        args = (index, P, nrm, dirs, offset, math.inf, outward)
        fused, t_fused = timed(lambda: index.thickness(*args[1:]), a.runs, a.warmup)
        comp, t_comp = timed(lambda: ops._thickness_composed(*args), max(1, a.composed_runs), 1)
        same = _same(fused, comp)
        ok = ok and same
        thick, thin, valid = fused
        finite = thin[torch.isfinite(thin)]
        entry = {"vertices": int(P.shape[0]), "faces": int(F.shape[0]), "index_build": build, "fused": t_fused, "composed": t_comp,
                 "same_bits": same, "composed_over_fused": t_comp["median_ms"] / t_fused["median_ms"],
                 "no_valid_ray_share": float((valid == 0).float().mean()), "valid_rays_per_vertex": float(valid.float().mean()),
                 "thinnest_median": float(finite.median()) if finite.numel() else float("nan"),
                 "thinnest_under_one_cell_share": float((thin < cell).float().mean())}
        result[case] = entry
        print("%s (%d vertices, %d faces) k=%d: fused %.3f ms (%.3f .. %.3f), composed %.3f ms (%.3f .. %.3f), ratio %.2f, same bits: "
              "%s; index build %.3f ms; %.2f valid rays per vertex, %.2f%% with none, median thinnest %.5f, %.2f%% thinner than one "
              "lattice cell (%.5f)" % (case, P.shape[0], F.shape[0], a.k, t_fused["median_ms"], t_fused["q1_ms"], t_fused["q3_ms"],
                                       t_comp["median_ms"], t_comp["q1_ms"], t_comp["q3_ms"], entry["composed_over_fused"], same,
                                       build["median_ms"], entry["valid_rays_per_vertex"], 100 * entry["no_valid_ray_share"],
                                       entry["thinnest_median"], 100 * entry["thinnest_under_one_cell_share"], cell), flush=True)

    with torch.no_grad():
        (v, f, uv, rast), atlas = timed(lambda: model._atlas(Mesh(lv, lf), a.res, 0.02, None), 1, 0)
    nrm = (outward * ops.vertex_normals(v, f)).contiguous()
    covered = int((rast[..., 3] >= 0).sum())
    bake = lambda: ops.bake_thickness(v, f, nrm, rast, thickness=a.k, outward=outward)   # noqa: E731
    fused, t_fused = timed(bake, max(1, min(a.runs, 3)), 1)
    os.environ[FORM] = "composedthickness"
    try:
        comp, t_comp = timed(bake, 1, 0)
    finally:
        os.environ.pop(FORM, None)
    same = _same(fused[:3], comp[:3]) and torch.equal(fused[3], comp[3])
    ok = ok and same
    result["bake"] = {"resolution": a.res, "covered_texels": covered, "unwrap_and_rasterise": atlas, "fused_point_kernel": t_fused,
                      "composed_point_route": t_comp, "same_bits": same,
                      "no_valid_ray_share": float((fused[2][fused[3]] == 0).float().mean()) if covered else 0.0}
    print("bake %d^2 (%d covered texels, %.1f%%) k=%d, grid build included: %.3f ms (%.3f .. %.3f) with the fused point kernel, %.3f ms "
          "with the composed point route, same bits: %s" % (a.res, covered, 100.0 * covered / (a.res * a.res), a.k, t_fused["median_ms"],
                                                            t_fused["q1_ms"], t_fused["q3_ms"], t_comp["median_ms"], same), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))
    assert ok, "the fused and the composed route differ"


if __name__ == "__main__":
    main()
