"""Time the projection of a 256^3 mesh onto the field's iso-surface: (a) ops.project_to_isosurface, the fused Newton kernel
(csrc/mesh_project.hip), (b) the same rule composed from ops.field_normals and one torch call per operation
(tests/_projref.py composed_device: every step over all vertices, no compaction, no early exit, no host wait), and (c)
ops.mesh_unfold, the fold guard, on the projected mesh -- on the same box and in the same process.

    python tools/time_project.py [--runs 21] [--warmup 3] [--out profiles/time_project.json]

The model is the full-size TSR with seeded weights (its density bias shifted so that the default threshold gives a surface, as
bench.py does); the mesh is extract_meshes at 256^3 of one synthetic picture; steps = 8, trust radius one lattice cell,
res_tol = 1e-3.  Every figure is wall clock around the call including a final torch.cuda.synchronize(), after warm-up calls, as
the median over the runs with the quartiles beside it.  All routes read the same channel-last planes (converted once, outside
the timed region).  Each route is timed a second time in the opposite order: the second of two must not owe its time to the
first one's caches.  Acceptance: the median of (a) is below the first quartile of (b), in both orders.  Also recorded: that
(a) and (b) give the same bits, the mean evaluations per vertex, the status histogram and the guard's statistics.
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

MC_RES, THRESHOLD, STEPS, CELLS, RES_TOL, ROUNDS = 256, 25.0, 8, 1.0, 1e-3, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_project.json"))
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    import _projref as ref
    from sculptmate_amd import ops

    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    v, f = mesh.vertices.contiguous(), mesh.faces
    cfg = model.renderer.cfg
    radius = float(cfg.radius)
    planes = ops.ChannelLastPlanes(code)
    target = float(np.float32(math.log(THRESHOLD) - float(cfg.density_bias)))
    max_dist = CELLS * 2.0 * radius / (MC_RES - 1)

    def fused():
        return ops.project_to_isosurface(planes, model.decoder, v, target, max_dist, steps=STEPS, res_tol=RES_TOL, radius=radius)[0]

    def fused_all():
        return ops.project_to_isosurface(planes, model.decoder, v, target, max_dist, steps=STEPS, res_tol=RES_TOL, radius=radius,
                                         want=("residual", "status", "evals"))

    def composed():
        return ref.composed_device(ops, planes, model.decoder, v, target, STEPS, max_dist, RES_TOL, radius)

    def one_evaluation():
        return ops.field_normals(planes, model.decoder, v, radius=radius, want=("grad", "density"))

    p, ex = fused_all()
    cp, cr, cs, ce = composed()
    same = (bool(torch.equal(p.view(torch.int32), cp.view(torch.int32))) and bool(torch.equal(ex["residual"].view(torch.int32), cr.view(torch.int32)))
            and bool(torch.equal(ex["status"], cs)) and bool(torch.equal(ex["evals"], ce)))
    d0 = one_evaluation()["density"][:, 0]

    def guard():
        return ops.mesh_unfold(v, p, f, ROUNDS)

    unfolded, st = guard()
    moved = torch.linalg.norm((p - v).double(), dim=1) / max_dist
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
              "decoder_hidden_layers": int(model.decoder.n_hidden), "steps": STEPS, "cells": CELLS, "res_tol": RES_TOL,
              "unfold_rounds": ROUNDS, "fused_equals_composed_bit_for_bit": same,
              "mean_evals": float(ex["evals"].double().mean()),
              "status_histogram": torch.bincount(ex["status"].long(), minlength=4).tolist(),
              "median_abs_residual_before": float((d0 - target).abs().median()),
              "median_abs_residual_after": float(ex["residual"].abs().median()),
              "median_displacement_cells": float(moved.median()), "largest_displacement_cells": float(moved.max()),
              "faces_inverted_before_guard": ops.unfold_stats(ops.mesh_unfold(v, p, f, 0)[1])["inverted"],
              "unfold": ops.unfold_stats(st),
              "fused": timed(fused, a.runs, a.warmup)[1],
              "composed": timed(composed, a.runs, a.warmup)[1],
              "unfold_ms": timed(guard, a.runs, a.warmup)[1],
              "one_evaluation": timed(one_evaluation, a.runs, a.warmup)[1],
              "fused_all_outputs": timed(fused_all, a.runs, a.warmup)[1]}
    result["one_evaluation_again"] = timed(one_evaluation, a.runs, a.warmup)[1]
    result["unfold_ms_again"] = timed(guard, a.runs, a.warmup)[1]
    result["composed_again"] = timed(composed, a.runs, a.warmup)[1]
    result["fused_again"] = timed(fused, a.runs, a.warmup)[1]
    result["accepted_fused_median_below_composed_q1"] = bool(
        result["fused"]["median_ms"] < result["composed"]["q1_ms"] and result["fused_again"]["median_ms"] < result["composed_again"]["q1_ms"])
    print("%d vertices, %d faces: fused %.3f ms (again %.3f), composed %.3f ms (again %.3f, q1 %.3f / %.3f), unfold %.3f ms (again "
          "%.3f), one evaluation %.3f ms; mean evals %.2f, status %s, unfold %s; same bits %s; accepted %s" % (
              v.shape[0], f.shape[0], result["fused"]["median_ms"], result["fused_again"]["median_ms"], result["composed"]["median_ms"],
              result["composed_again"]["median_ms"], result["composed"]["q1_ms"], result["composed_again"]["q1_ms"],
              result["unfold_ms"]["median_ms"], result["unfold_ms_again"]["median_ms"], result["one_evaluation"]["median_ms"],
              result["mean_evals"], result["status_histogram"], result["unfold"], same,
              result["accepted_fused_median_below_composed_q1"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))
    if not (same and result["accepted_fused_median_below_composed_q1"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
