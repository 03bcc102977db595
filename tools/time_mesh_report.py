"""Time the mesh report (csrc/mesh_report.hip, ops.mesh_report / ops.mesh_self_intersections) on the meshes it is meant for --
extract_meshes at 256^3 of the full-size TSR with seeded weights, simplify=0.1 of it, and voxel_remesh=128 of it -- and record
what the report says about each: the self-intersection count before and after the voxel remesh is the measurement behind "the
overlapping blobs of a generated mesh fuse" (DESIGN.md 3.3m).

    python tools/time_mesh_report.py [--runs 5] [--warmup 1] [--out profiles/time_mesh_report.json]

Timed per mesh, each stage on its own, on inputs that are already checked and indexed: the edge census (the kernel alone, on a
built topology, and with the topology build), the per-face measures with their two sums, the self-intersection count (phase 1
with its scan and readback) and the count with the emitted, sorted pair list, in both kernel forms, and the whole
ops.mesh_report call with and without self-intersections.  Beside the census: the host route the earlier figures took (faces
device -> NumPy, the edge count there, the result back).

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; median and quartiles over
the runs.  No threshold is set here."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

MC_RES, THRESHOLD = 256, 25.0
FORM = "SCULPT_DISTANCE_FORM"


def host_census(faces):
    """The route the figures in README / DESIGN.md took so far: device -> host, the edge count in NumPy, three integers back."""
    f = faces.cpu().numpy().astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    counts = np.unique(e[:, 0] * (int(f.max()) + 1) + e[:, 1], return_counts=True)[1]
    return torch.tensor([len(counts), int((counts == 1).sum()), int((counts > 2).sum())], device=faces.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_mesh_report.json"))
    a = ap.parse_args()
    from sculptmate_amd import _lib, ops
    from sculptmate_amd.ops import _ptr, _stream
    from sculptmate_amd.sf3d import remesh_device as rmd

    os.environ.pop(FORM, None)
    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    meshes = {"extracted_256": mesh, "simplify_0.1": mesh.simplify(0.1), "voxel_remesh_128": mesh.voxel_remesh(128)}
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "meshes": {}}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")

    for name, m in meshes.items():
        r = result["meshes"][name] = {}
        v, f = m.vertices, m.faces
        P, F = ops._surface(v, f, "time_mesh_report")
        r["report"] = ops.mesh_report(v, f)
        print("%s: %s" % (name, json.dumps(r["report"], sort_keys=True)), flush=True)
        save()

        topo, r["topology_build"] = timed(lambda: rmd._Topo(rmd._Ctx(), F, P.shape[0]), a.runs, a.warmup)
        counts = torch.empty(8, dtype=torch.int64, device=dev)

        def census():
            _lib.check(_lib.lib.sculpt_mesh_edge_census(topo.ref(), _ptr(counts), _stream()))
            return counts.tolist()

        got, r["census_kernel_and_readback"] = timed(census, a.runs, a.warmup)
        host, r["census_host_route"] = timed(lambda: host_census(f).tolist(), a.runs, a.warmup)
        assert got[:3] == host, (got, host)

        def measures():
            area2, vol6 = ops._face_measures(P, F, counts[5:6])
            return torch.stack([area2.sum(), vol6.sum()]).tolist()

        _, r["measures_and_sums"] = timed(measures, a.runs, a.warmup)
        for form in ("default", "plain"):
            if form == "plain":
                os.environ[FORM] = "plain"
            (total, flagged, _, _), r["self_count_" + form] = timed(lambda: ops._self_intersections(P, F, False, 0), a.runs, a.warmup)
            (total2, _, _, pairs), r["self_count_and_emit_" + form] = timed(lambda: ops._self_intersections(P, F, True, ops.SELF_MAX_PAIRS),
                                                                              a.runs, a.warmup)
            os.environ.pop(FORM, None)
            assert total == total2 == r["report"]["self_intersections"] == pairs.shape[0]
        _, r["report_without_self_intersections"] = timed(lambda: ops.mesh_report(v, f, self_intersections=False), a.runs, a.warmup)
        _, r["report_full"] = timed(lambda: ops.mesh_report(v, f), a.runs, a.warmup)
        print("%s: topology %.2f ms, census %.2f ms (host route %.2f ms), measures %.2f ms, self count %.2f ms (plain %.2f), with the "
              "pair list %.2f ms (plain %.2f), report %.2f ms, full %.2f ms" % (
                  name, *(r[k]["median_ms"] for k in ("topology_build", "census_kernel_and_readback", "census_host_route",
                                                      "measures_and_sums", "self_count_default", "self_count_plain",
                                                      "self_count_and_emit_default", "self_count_and_emit_plain",
                                                      "report_without_self_intersections", "report_full"))), flush=True)
        save()
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
