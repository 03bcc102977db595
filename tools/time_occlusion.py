"""Time the ray queries (csrc/mesh_ray.hip, ops.mesh_ray_cast / mesh_occlusion) on the mesh they are meant for -- extract_meshes
at 256^3 of the full-size TSR with seeded weights.

    python tools/time_occlusion.py [--runs 7] [--warmup 2] [--rays 1000000] [--k 64] [--out profiles/time_occlusion.json]

Timed: the grid build; the fused occlusion (one launch, sculpt_surface_occlusion) at k directions over the mesh's own vertices
against the composed route on the same inputs and the same grid (one closest-hit query per direction plus torch reductions:
the loop of ops.mesh_occlusion_composed, without its grid build), whose bits it must equal; and `rays` closest-hit rays in the
plain and the default form (the two alternate inside one run): origins on a sphere around the mesh, aimed at area-uniform
points of it.

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; median and quartiles over
the runs.  No threshold is set here."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import seeded_mesh, stats, timed  # noqa: E402

MC_RES, THRESHOLD = 256, 25.0
FORM = "SCULPT_DISTANCE_FORM"


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def both_forms(index, origins, directions, runs, warmup):
    """The closest-hit query in the two forms, alternating run by run -> ({form: stats}, the results agree bit for bit)."""
    ms, out = {"default": [], "plain": []}, {}
    for i in range(warmup + runs):
        for form in ("default", "plain"):
            if form == "plain":
                os.environ[FORM] = "plain"
            else:
                os.environ.pop(FORM, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[form] = index.ray_cast(origins, directions)
            torch.cuda.synchronize()
            if i >= warmup:
                ms[form].append((time.perf_counter() - t0) * 1e3)
    os.environ.pop(FORM, None)
    same = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out["default"], out["plain"]))
    return {form: stats(t) for form, t in ms.items()}, same, out["default"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_occlusion.json"))
    a = ap.parse_args()
    import numpy as np

    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR

    os.environ.pop(FORM, None)
    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    v, f = mesh.vertices, mesh.faces
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
              "rays": a.rays, "directions": a.k}
    print("mesh: %d vertices, %d faces" % (v.shape[0], f.shape[0]), flush=True)

    P, F = ops._surface(v, f, "time_occlusion")
    index, result["grid_build"] = timed(lambda: ops._SurfaceIndex(P, F), a.runs, a.warmup)
    index.records()
    result["grid_cells"] = [int(index.grid.params[4 + k]) for k in range(3)]
    result["grid_entries"] = int(index.grid.items.shape[0])

    nrm = (TSR.WINDING_OUTWARD * ops.vertex_normals(P, F)).contiguous()
    dirs = torch.from_numpy(ops.occlusion_directions(a.k, 0)).to(dev)
    offset = float(np.float32(ops.OCCLUSION_OFFSET * index.longest_side()))
    fused, result["occlusion_fused"] = timed(lambda: index.occlusion(P, nrm, dirs, offset, math.inf), a.runs, a.warmup)
    comp, result["occlusion_composed"] = timed(lambda: ops._occlusion_composed(index, P, nrm, dirs, offset, math.inf), max(1, min(a.runs, 3)), 1)
    same_ao = torch.equal(_bits(fused), _bits(comp))
    ratio = result["occlusion_composed"]["median_ms"] / result["occlusion_fused"]["median_ms"]
    result["occlusion"] = {"same_bits": same_ao, "composed_over_fused": ratio, "mean_ao": float(fused.mean()),
                           "open_vertices": int((fused == 1).sum()), "points": int(P.shape[0])}
    print("occlusion k=%d over %d vertices: fused %.3f ms (%.3f .. %.3f), composed %.3f ms (%.3f .. %.3f), ratio %.2f, same bits: %s, "
          "mean ao %.4f" % (a.k, P.shape[0], result["occlusion_fused"]["median_ms"], result["occlusion_fused"]["q1_ms"],
                            result["occlusion_fused"]["q3_ms"], result["occlusion_composed"]["median_ms"],
                            result["occlusion_composed"]["q1_ms"], result["occlusion_composed"]["q3_ms"], ratio, same_ao,
                            result["occlusion"]["mean_ao"]), flush=True)

    targets = ops._sample(P, F, a.rays, 0)[0]
    lo, hi = P.min(0).values, P.max(0).values
    centre, radius = 0.5 * (lo + hi), float((hi - lo).norm())
    g = torch.Generator(device="cpu").manual_seed(0)
    u = torch.randn((a.rays, 3), generator=g).to(dev)
    origins = (centre + radius * u / u.norm(dim=1, keepdim=True)).contiguous()
    directions = (targets - origins).contiguous()
    forms, same, out = both_forms(index, origins, directions, a.runs, a.warmup)
    result["ray_cast"] = dict(forms, same_bits=same, rays=a.rays, hits=int((out[1] >= 0).sum()))
    r = result["ray_cast"]
    print("ray_cast %d rays: default %.3f ms (%.3f .. %.3f), plain %.3f ms (%.3f .. %.3f), same bits: %s, %d hit" % (
        a.rays, r["default"]["median_ms"], r["default"]["q1_ms"], r["default"]["q3_ms"], r["plain"]["median_ms"], r["plain"]["q1_ms"],
        r["plain"]["q3_ms"], same, r["hits"]), flush=True)
    t = result["grid_build"]
    print("grid_build: %.3f ms (quartiles %.3f .. %.3f)" % (t["median_ms"], t["q1_ms"], t["q3_ms"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))
    assert same and same_ao, "the forms / routes of the ray queries differ"


if __name__ == "__main__":
    main()
