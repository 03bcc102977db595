"""Time the smooth normals of a 256^3 mesh: ops.field_normals (the density-gradient kernel, csrc/field_normal.hip) at the
mesh's vertices, beside ops.triplane_query (density only) at the same points and ops.vertex_normals (the averaged facet
normals) of the same mesh, on the same box and in the same process.

    python tools/time_field_normals.py [--runs 21] [--warmup 3] [--out profiles/time_field_normals.json]

The model is the full-size TSR with seeded weights (its density bias shifted so that the default threshold gives a surface, as
bench.py does); the mesh is extract_meshes at 256^3 of one synthetic picture.  Every figure is wall clock around the call
including a final torch.cuda.synchronize(), after warm-up calls, as the median over the runs with the quartiles beside it.  All
routes read the same channel-last planes (converted once, outside the timed region).  The gradient kernel evaluates four MFMA
columns per point where the point query evaluates one; the expectation from the column count is about 4x the point query plus
the quad broadcasts.  Each route is timed a second time in the other order: the second of two must not owe its time to the
first one's caches.
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

MC_RES, THRESHOLD = 256, 25.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_field_normals.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    from sculptmate_amd import ops

    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    v, f = mesh.vertices, mesh.faces
    radius = model.renderer.cfg.radius
    planes = ops.ChannelLastPlanes(code)

    def field():
        return ops.field_normals(planes, model.decoder, v, radius=radius)["normal"]

    def field_all():
        return ops.field_normals(planes, model.decoder, v, radius=radius, want=("normal", "grad", "density"))

    def query():
        return ops.triplane_query(planes, model.decoder, v, radius=radius, want=("density",))["density"]

    def facets():
        return ops.vertex_normals(v, f)

    every = field_all()
    same = bool(torch.equal(every["density"], query())) and bool(torch.equal(every["normal"], field()))
    nf, nv = field(), facets()
    unit = float((torch.linalg.norm(nf.double(), dim=1) - 1).abs().max())
    cos = (nf * nv).sum(1)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
              "decoder_hidden_layers": int(model.decoder.n_hidden), "density_equals_point_query": same,
              "largest_deviation_from_unit_length": unit, "mean_cosine_field_vs_facet_normals": float(cos.mean()),
              "share_cosine_above_0.9": float((cos > 0.9).float().mean()),
              "field_normals": timed(field, a.runs, a.warmup)[1],
              "triplane_query_density": timed(query, a.runs, a.warmup)[1],
              "vertex_normals": timed(facets, a.runs, a.warmup)[1],
              "field_normals_all_outputs": timed(field_all, a.runs, a.warmup)[1]}
    result["vertex_normals_again"] = timed(facets, a.runs, a.warmup)[1]
    result["triplane_query_density_again"] = timed(query, a.runs, a.warmup)[1]
    result["field_normals_again"] = timed(field, a.runs, a.warmup)[1]
    result["ratio_field_normals_to_point_query"] = round(
        result["field_normals"]["median_ms"] / result["triplane_query_density"]["median_ms"], 3)
    print("%d vertices: field_normals %.3f ms (again %.3f), triplane_query density %.3f ms (again %.3f), vertex_normals %.3f ms "
          "(again %.3f); ratio %.2f; density identical %s" % (
              v.shape[0], result["field_normals"]["median_ms"], result["field_normals_again"]["median_ms"],
              result["triplane_query_density"]["median_ms"], result["triplane_query_density_again"]["median_ms"],
              result["vertex_normals"]["median_ms"], result["vertex_normals_again"]["median_ms"],
              result["ratio_field_normals_to_point_query"], same), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
