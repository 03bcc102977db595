"""Time the curvature queries (csrc/mesh_curvature.hip, ops.mesh_curvature / bake_curvature) on the meshes they are meant for --
extract_meshes at 256^3 of the full-size TSR with seeded weights (the HIGH mesh), simplify=0.1 of it (the LOW mesh) and the low
mesh's atlas at 2048^2.

    python tools/time_curvature.py [--runs 5] [--warmup 1] [--rings 4] [--res 2048] [--out profiles/time_curvature.json]

Timed:
    high, low   ops.mesh_curvature at rings 0 and `rings` (the whole call: input check, one topology, the neighbour table when
                rings > 0, the kernels), and its parts on prebuilt inputs: the input check, the topology, the neighbour table,
                the terms kernel (with its pack), the `rings` rounds (with pack and unpack), the finish
    host        on the low mesh only, once: the same result by way of the host -- device -> host copies, tests/_curvref.py
                (NumPy, a Python loop over the corners), host -> device; mean must equal the device's bits at rings 0
    bake        ops.bake_curvature of the low mesh over its atlas at `res`^2, of itself and against the high mesh as source
What the numbers say about the mesh: the share of valid vertices, and the spread of the mean curvature at rings 0 and `rings`
in units of 1 / lattice cell.

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; median and quartiles over
the runs.  No threshold is set here."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

MC_RES, THRESHOLD, SIMPLIFY = 256, 25.0, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rings", type=int, default=4)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_curvature.json"))
    a = ap.parse_args()
    import numpy as np

    from sculptmate_amd import ops
    from sculptmate_amd.sf3d import remesh_device as rmd
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.system import Mesh

    dev = torch.device("cuda:0")
    model, code, high = seeded_mesh(dev, MC_RES, THRESHOLD)
    lv, lf = ops.mesh_simplify(high.vertices, high.faces, SIMPLIFY)[:2]
    cell = 2.0 * float(model.renderer.cfg.radius) / (MC_RES - 1)
    outward = float(TSR.WINDING_OUTWARD)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "rings": a.rings, "lattice_cell": cell}
    for case, (v, f) in (("high", (high.vertices, high.faces)), ("low", (lv, lf))):
        entry = {"vertices": int(v.shape[0]), "faces": int(f.shape[0])}
        for r in (0, a.rings):
            (mean, gauss, valid), t = timed(lambda: ops.mesh_curvature(v, f, r, outward), a.runs, a.warmup)
            h = mean[valid].double() * cell
            entry["call_rings_%d" % r] = t
            entry["mean_cells_rings_%d" % r] = {"p5": float(h.quantile(0.05)) if h.numel() < 1 << 24 else None, "median": float(h.median()),
                                                "std": float(h.std())}
            entry["valid_share"] = float(valid.float().mean())
        ctx = rmd._Ctx()
        (P, F), t_check = timed(lambda: rmd._inputs(v, f, "time_curvature"), a.runs, a.warmup)
        T, t_topo = timed(lambda: rmd._plain_topo(ctx, F, P.shape[0]), a.runs, a.warmup)
        (start, nb, _), t_table = timed(lambda: rmd._smooth_table(ctx, F, P.shape[0], topo=T), a.runs, a.warmup)
        terms, t_terms = timed(lambda: rmd._curvature_terms(ctx, T, P, outward), a.runs, a.warmup)
        ringed, t_ring = timed(lambda: rmd._curvature_ring(ctx, terms, start, nb, a.rings), a.runs, a.warmup)
        _, t_finish = timed(lambda: rmd._curvature_finish(ctx, ringed), a.runs, a.warmup)
        entry.update(input_check=t_check, topology=t_topo, neighbour_table=t_table, terms=t_terms, rings=t_ring, finish=t_finish)
        result[case] = entry
        print("%s (%d vertices, %d faces, %.1f%% valid): call %.3f ms at rings 0, %.3f ms at rings %d; input check %.3f, topology %.3f, "
              "neighbour table %.3f, terms %.3f, %d rounds %.3f, finish %.3f ms; std of H in 1/cell %.3f -> %.3f"
              % (case, v.shape[0], f.shape[0], 100 * entry["valid_share"], entry["call_rings_0"]["median_ms"],
                 entry["call_rings_%d" % a.rings]["median_ms"], a.rings, t_check["median_ms"], t_topo["median_ms"], t_table["median_ms"],
                 t_terms["median_ms"], a.rings, t_ring["median_ms"], t_finish["median_ms"], entry["mean_cells_rings_0"]["std"],
                 entry["mean_cells_rings_%d" % a.rings]["std"]), flush=True)

    if not a.no_host:
        import _curvref as C

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        V, F = lv.cpu().numpy(), lf.cpu().numpy()
        t1 = time.perf_counter()
        mean_h, gauss_h, valid_h = C.curvature(V, F, 0, outward)
        t2 = time.perf_counter()
        back = torch.from_numpy(mean_h).to(dev), torch.from_numpy(gauss_h).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        mean_d = ops.mesh_curvature(lv, lf, 0, outward)[0]
        same = bool(torch.equal(torch.nan_to_num(mean_d, nan=0.0).view(torch.int32), torch.nan_to_num(back[0], nan=0.0).view(torch.int32)))
        result["host"] = {"download_ms": 1e3 * (t1 - t0), "numpy_ms": 1e3 * (t2 - t1), "upload_ms": 1e3 * (t3 - t2), "mean_same_bits": same}
        print("low mesh by way of the host at rings 0: download %.1f ms, NumPy restatement %.1f ms, upload %.1f ms; mean bit for bit: %s"
              % (result["host"]["download_ms"], result["host"]["numpy_ms"], result["host"]["upload_ms"], same), flush=True)

    with torch.no_grad():
        (v, f, uv, rast), atlas = timed(lambda: model._atlas(Mesh(lv, lf), a.res, 0.02, None), 1, 0)
    nrm = (outward * ops.vertex_normals(v, f)).contiguous()
    covered = int((rast[..., 3] >= 0).sum())
    source = (high.vertices, high.faces)
    runs = max(1, min(a.runs, 3))
    own, t_own = timed(lambda: ops.bake_curvature(v, f, nrm, rast, curvature=a.rings, outward=outward), runs, 1)
    src, t_src = timed(lambda: ops.bake_curvature(v, f, nrm, rast, curvature=a.rings, outward=outward, source=source), runs, 1)
    moved = own[2] & (own[0] != src[0]) & ~(torch.isnan(own[0]) & torch.isnan(src[0]))
    result["bake"] = {"resolution": a.res, "covered_texels": covered, "unwrap_and_rasterise": atlas, "own": t_own, "source": t_src,
                      "texels_read_from_the_source_share": float(moved.sum()) / max(covered, 1)}
    print("bake %d^2 (%d covered texels, %.1f%%) rings %d: %.3f ms (%.3f .. %.3f) of the mesh itself, %.3f ms (%.3f .. %.3f) against the "
          "high mesh (topology, grid build and snap included); %.1f%% of the covered texels differ from the own value"
          % (a.res, covered, 100.0 * covered / (a.res * a.res), a.rings, t_own["median_ms"], t_own["q1_ms"], t_own["q3_ms"],
             t_src["median_ms"], t_src["q1_ms"], t_src["q3_ms"], 100 * result["bake"]["texels_read_from_the_source_share"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))
    assert a.no_host or result["host"]["mean_same_bits"], "the device and the restatement differ"


if __name__ == "__main__":
    main()
