"""Time the surface distance queries (csrc/mesh_distance.hip, ops.mesh_closest_points / mesh_sample_surface / mesh_distance) on
the mesh they are meant for -- extract_meshes at 256^3 of the full-size TSR with seeded weights -- and measure with them what
the mesh options do to that surface: mesh_distance(plain, X, samples=None) for X = smooth=10, simplify=0.1, project=True, the
simplified mesh refined by subdivide=1 (with and without project) and simplify=0.4, in lattice cells.

    python tools/time_mesh_distance.py [--runs 7] [--warmup 2] [--samples 1000000] [--out profiles/time_mesh_distance.json]

Timed: the grid build, the sample kernel's call, and the closest-point query in the plain and the default form (the two
alternate inside one run, on the same grid): `samples` area-uniform points of the mesh against the mesh itself, and the mesh's
vertices against simplify=0.1 of it.  The two forms' results are compared bit for bit on both cases.

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; median and quartiles over
the runs.  No threshold is set here."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import seeded_mesh, stats  # noqa: E402

MC_RES, THRESHOLD = 256, 25.0
FORM = "SCULPT_DISTANCE_FORM"


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def both_forms(index, points, runs, warmup):
    """The query in the two forms, alternating run by run -> ({form: stats}, the results agree bit for bit)."""
    import time

    ms, out = {"default": [], "plain": []}, {}
    for i in range(warmup + runs):
        for form in ("default", "plain"):
            if form == "plain":
                os.environ[FORM] = "plain"
            else:
                os.environ.pop(FORM, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[form] = index.closest(points)
            torch.cuda.synchronize()
            if i >= warmup:
                ms[form].append((time.perf_counter() - t0) * 1e3)
    os.environ.pop(FORM, None)
    same = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out["default"], out["plain"]))
    return {form: stats(t) for form, t in ms.items()}, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_mesh_distance.json"))
    a = ap.parse_args()
    from _timing import timed
    from sculptmate_amd import ops

    os.environ.pop(FORM, None)
    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    v, f = mesh.vertices, mesh.faces
    cell = 2.0 * float(model.renderer.cfg.radius) / (MC_RES - 1)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
              "samples": a.samples, "lattice_cell": cell}
    print("mesh: %d vertices, %d faces; lattice cell %.6f" % (v.shape[0], f.shape[0], cell), flush=True)

    P, F = ops._surface(v, f, "time_mesh_distance")
    index, result["grid_build"] = timed(lambda: ops._SurfaceIndex(P, F), a.runs, a.warmup)
    _, result["records_pack"] = timed(lambda: _pack(index), a.runs, a.warmup)
    (pts, _, _), result["sample"] = timed(lambda: ops._sample(P, F, a.samples, 0), a.runs, a.warmup)
    result["grid_cells"] = [int(index.grid.params[4 + k]) for k in range(3)]
    result["grid_entries"] = int(index.grid.items.shape[0])

    forms, same = both_forms(index, pts, a.runs, a.warmup)
    result["closest_samples_vs_self"] = dict(forms, same_bits=same, queries=int(pts.shape[0]), faces=int(F.shape[0]))
    with torch.no_grad():
        variants = {"smooth=10": model.extract_meshes([code], False, MC_RES, THRESHOLD, smooth=10)[0],
                    "simplify=0.1": model.extract_meshes([code], False, MC_RES, THRESHOLD, simplify=0.1)[0],
                    "project=True": model.extract_meshes([code], False, MC_RES, THRESHOLD, project=True)[0],
                    # what subdivision gives back to the simplified cage, against a simplification to about as many faces
                    "simplify=0.1, subdivide=1": model.extract_meshes([code], False, MC_RES, THRESHOLD, simplify=0.1, subdivide=1)[0],
                    "simplify=0.1, subdivide=1, project=True": model.extract_meshes([code], False, MC_RES, THRESHOLD, simplify=0.1,
                                                                                    subdivide=1, project=True)[0],
                    "simplify=0.4": model.extract_meshes([code], False, MC_RES, THRESHOLD, simplify=0.4)[0]}
    simp = variants["simplify=0.1"]
    Ps, Fs = ops._surface(simp.vertices, simp.faces, "time_mesh_distance")
    forms, same2 = both_forms(ops._SurfaceIndex(Ps, Fs), P, a.runs, a.warmup)
    result["closest_vertices_vs_simplified"] = dict(forms, same_bits=same2, queries=int(P.shape[0]), faces=int(Fs.shape[0]))
    for name in ("closest_samples_vs_self", "closest_vertices_vs_simplified"):
        r = result[name]
        print("%s: default %.3f ms (%.3f .. %.3f), plain %.3f ms (%.3f .. %.3f), same bits: %s" % (
            name, r["default"]["median_ms"], r["default"]["q1_ms"], r["default"]["q3_ms"], r["plain"]["median_ms"],
            r["plain"]["q1_ms"], r["plain"]["q3_ms"], r["same_bits"]), flush=True)
    for name in ("grid_build", "records_pack", "sample"):
        t = result[name]
        print("%s: %.3f ms (quartiles %.3f .. %.3f)" % (name, t["median_ms"], t["q1_ms"], t["q3_ms"]), flush=True)

    result["quality"] = {}
    for name, other in variants.items():
        d, t = timed(lambda: mesh.distance_to(other, samples=None), max(1, min(a.runs, 3)), 1)
        cells = {way: {k: x / cell for k, x in d[way].items()} for way in ("a_to_b", "b_to_a")}
        result["quality"][name] = {"vertices": int(other.vertices.shape[0]), "faces": int(other.faces.shape[0]), "distance": d,
                                   "in_cells": dict(cells, chamfer=d["chamfer"] / cell, hausdorff=d["hausdorff"] / cell),
                                   "mesh_distance": t}
        print("plain -> %s: mean %.4f, max %.4f cells; back: mean %.4f, max %.4f cells (%.1f ms)" % (
            name, cells["a_to_b"]["mean"], cells["a_to_b"]["max"], cells["b_to_a"]["mean"], cells["b_to_a"]["max"], t["median_ms"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))
    assert same and same2, "the two forms of the query differ"


def _pack(index):
    index._records = None
    return index.records()


if __name__ == "__main__":
    main()
