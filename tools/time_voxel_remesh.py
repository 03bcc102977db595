"""Time the voxel remesh (csrc/mesh_winding.hip, ops.mesh_voxel_remesh) on the mesh it is meant for -- extract_meshes at 256^3 of
the full-size TSR with seeded weights -- at R = 128 and 256 cells along the longest side.

    python tools/time_voxel_remesh.py [--runs 5] [--warmup 1] [--resolutions 128 256] [--whole-lattice-max 128]
                                      [--out profiles/time_voxel_remesh.json]

Timed per R, stage by stage on one surface index: the sign lattice (sculpt_surface_winding_lattice), the active-corner list
(one readback), the closest-point query over the listed corners (the band route), the fill, marching cubes, and the whole
ops.mesh_voxel_remesh call (which also builds the index).  In the same run:
  - the lattice kernel against ops.mesh_winding's kernel on the MATERIALISED lattice points, in both forms (sorted by cell, and
    plain in input order), alternating, with the integers compared;
  - the band route against a closest-point query over the WHOLE lattice (only up to --whole-lattice-max: the whole lattice at
    256 is 17.8 M queries, most of them far from any face).
Reported for the output: faces, border and non-manifold edges, components, and Mesh.distance_to the input in lattice cells.

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

from _timing import seeded_mesh, timed  # noqa: E402

MC_RES, THRESHOLD = 256, 25.0
FORM = "SCULPT_DISTANCE_FORM"


def edge_report(faces):
    """Border (one face) and non-manifold (more than two faces) edges of a triangle mesh."""
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = torch.sort(e, 1).values
    counts = torch.unique(e[:, 0] * (int(faces.max()) + 1) + e[:, 1], return_counts=True)[1]
    return {"edges": int(counts.shape[0]), "border_edges": int((counts == 1).sum()), "non_manifold_edges": int((counts > 2).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--whole-lattice-max", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_voxel_remesh.json"))
    a = ap.parse_args()
    from sculptmate_amd import ops
    from sculptmate_amd.tsr.mesh import Mesh

    os.environ.pop(FORM, None)
    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    v, f = mesh.vertices, mesh.faces
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
              "input_edges": edge_report(f), "input_components": int(ops.mesh_components(f, v.shape[0])["roots"].shape[0]), "R": {}}
    print("input: %d vertices, %d faces, %s, %d components" % (v.shape[0], f.shape[0], result["input_edges"], result["input_components"]),
          flush=True)
    P, F = ops._surface(v, f, "time_voxel_remesh")
    index, result["index_build"] = timed(lambda: _index(ops, P, F), a.runs, a.warmup)
    same_all = True

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")

    for R in a.resolutions:
        r = result["R"][str(R)] = {}
        lo, h, n = ops._voxel_lattice(index, R, "time_voxel_remesh")
        band = ops.VOXEL_BAND_CELLS * h
        r.update(h=h, lattice=n, points=n[0] * n[1] * n[2])
        (planes, _), r["sign_lattice"] = timed(lambda: index.winding_lattice(lo, h, n), a.runs, a.warmup)
        listed, r["active_list"] = timed(lambda: ops.lattice_active_corners(planes, n), a.runs, a.warmup)
        pts, r["list_points"] = timed(lambda: ops._lattice_points(listed, lo, h, n), a.runs, a.warmup)
        (d2, _, _), r["band_distance"] = timed(lambda: index.closest(pts), a.runs, a.warmup)
        vol, r["fill"] = timed(lambda: ops._sdf_fill(planes, listed, d2, n, band), a.runs, a.warmup)
        (ov, of), r["marching_cubes"] = timed(lambda: ops.marching_cubes(vol, 0.0, reference_order=True, sign_planes=planes), a.runs, a.warmup)
        (ov, of), r["total"] = timed(lambda: ops.mesh_voxel_remesh(v, f, R), a.runs, a.warmup)
        r["listed"] = int(listed.shape[0])
        print("R=%d: lattice %s, %d listed; sign lattice %.2f ms, list %.2f, points %.2f, band distance %.2f, fill %.2f, MC %.2f, total %.2f" % (
            R, n, r["listed"], *(r[k]["median_ms"] for k in ("sign_lattice", "active_list", "list_points", "band_distance", "fill",
                                                               "marching_cubes", "total"))), flush=True)

        # the lattice kernel against the point kernel on materialised points, both forms
        all_idx = torch.arange(r["points"], dtype=torch.int32, device=dev)
        every = ops._lattice_points(all_idx, lo, h, n)
        del all_idx
        counts, r["lattice_kernel_with_counts"] = timed(lambda: index.winding_lattice(lo, h, n, True)[1], a.runs, a.warmup)
        counts = counts.reshape(-1, 3)
        for form in ("default", "plain"):
            if form == "plain":
                os.environ[FORM] = "plain"
            w, r["point_kernel_" + form] = timed(lambda: index.winding(every), a.runs, a.warmup)
            os.environ.pop(FORM, None)
            same = bool(torch.equal(w, counts))
            same_all = same_all and same
            r["point_kernel_" + form]["same_integers"] = same
            del w
        print("R=%d: lattice kernel %.2f ms (with counts %.2f); point kernel on %d materialised points: sorted %.2f ms, plain %.2f ms" % (
            R, r["sign_lattice"]["median_ms"], r["lattice_kernel_with_counts"]["median_ms"], r["points"],
            r["point_kernel_default"]["median_ms"], r["point_kernel_plain"]["median_ms"]), flush=True)
        del counts
        out = Mesh(ov, of)
        d = mesh.distance_to(out, samples=None)
        r["output"] = dict(edge_report(of), vertices=int(ov.shape[0]), faces=int(of.shape[0]),
                           components=int(ops.mesh_components(of, ov.shape[0])["roots"].shape[0]),
                           distance_in_cells={way: {k: x / h for k, x in d[way].items()} for way in ("a_to_b", "b_to_a")})
        print("R=%d output: %s" % (R, json.dumps(r["output"], sort_keys=True)), flush=True)
        r["whole_lattice_distance"] = "not measured"
        save()
        if R <= a.whole_lattice_max:   # far lattice points walk many empty cells: two calls, no warm-up
            (d2_all, _, _), r["whole_lattice_distance"] = timed(lambda: index.closest(every), 2, 0)
            r["whole_lattice_distance"]["same_bits_at_listed"] = bool(torch.equal(d2_all[listed.long()].view(torch.int64), d2.view(torch.int64)))
            print("R=%d: distance over the whole lattice %.2f ms against %.2f ms over the band's %d points" % (
                R, r["whole_lattice_distance"]["median_ms"], r["band_distance"]["median_ms"], r["listed"]), flush=True)
            del d2_all
        else:
            r["whole_lattice_distance"] = "not measured (above --whole-lattice-max)"
        del every
        save()
    print(json.dumps({"out": a.out}))
    assert same_all, "the lattice kernel and the point kernel differ"


def _index(ops, P, F):
    index = ops._SurfaceIndex(P, F)
    index.records()
    return index


if __name__ == "__main__":
    main()
