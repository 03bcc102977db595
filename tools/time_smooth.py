"""Time the device smoother (csrc/mesh_smooth.hip, ops.mesh_smooth) on the mesh it is meant for: extract_meshes at 256^3 of the
full-size TSR with seeded weights (every component, the size a trained model's object has), 10 iterations of the default
lambda|mu pair.  Split out: the neighbour table (one topology construction, the key sort, the row offsets) and the 2 x
iterations half-steps with their pack / unpack.  Beside it the route a caller has without it: device -> host, the same
arithmetic as a scipy.sparse CSR mat-vec per half-step (float32: row sums, a division by the degree, p + k (c - p), fixed rows
masked), host -> device.

    python tools/time_smooth.py [--runs 7] [--warmup 2] [--iterations 10] [--no-host] [--out profiles/time_smooth.json]

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


def host_route(v, f, n, lam, mu):
    """device -> host -> scipy.sparse -> device; the table is built on the host as well (the caller has none)."""
    import scipy.sparse as sp

    P, F = v.cpu().numpy(), f.cpu().numpy().astype(np.int64)
    nv = len(P)
    he = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    he.sort(axis=1)
    E, count = np.unique(he[:, 0] << 32 | he[:, 1], return_counts=True)
    u, w = E >> 32, E & 0xFFFFFFFF
    A = sp.csr_matrix((np.ones(2 * len(E), np.float32), (np.concatenate([u, w]), np.concatenate([w, u]))), shape=(nv, nv))
    deg = np.diff(A.indptr).astype(np.float32)
    fixed = np.zeros(nv, bool)
    odd = count != 2
    fixed[u[odd]] = True
    fixed[w[odd]] = True
    move = (deg > 0) & ~fixed
    safe = np.where(deg > 0, deg, np.float32(1))[:, None]
    p = P.astype(np.float32)
    for _ in range(n):
        for k in ((lam,) if mu == 0 else (lam, mu)):
            c = (A @ p) / safe
            p = np.where(move[:, None], p + np.float32(k) * (c - p), p)
    return torch.from_numpy(p).to(v.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_smooth.json"))
    a = ap.parse_args()
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d import remesh_device as rd

    dev = torch.device("cuda:0")
    model, code, mesh = seeded_mesh(dev, MC_RES, THRESHOLD)
    v, f = mesh.vertices, mesh.faces
    n, lam, mu = ops.smooth_rule(a.iterations)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "iterations": n, "lambda": lam, "mu": mu,
              "vertices": int(v.shape[0]), "faces": int(f.shape[0])}
    print("mesh: %d vertices, %d faces; %d iterations" % (v.shape[0], f.shape[0], n), flush=True)

    out, result["mesh_smooth"] = timed(lambda: ops.mesh_smooth(v, f, a.iterations), a.runs, a.warmup)
    result["mesh_smooth"]["readbacks"] = rd.last_stats()["readbacks"]
    P, F = rd._inputs(v, f, "time_smooth")
    _, result["inputs_check"] = timed(lambda: rd._inputs(v, f, "time_smooth"), a.runs, a.warmup)
    table, result["table"] = timed(lambda: rd._smooth_table(rd._Ctx(), F, P.shape[0]), a.runs, a.warmup)
    steps, result["half_steps"] = timed(lambda: rd._smooth_steps(rd._Ctx(), P, table, n, lam, mu), a.runs, a.warmup)
    assert torch.equal(steps, out)
    result["half_steps"]["us_per_half_step"] = round(result["half_steps"]["median_ms"] * 1e3 / (2 * n), 2)
    result["neighbours"] = int(table[1].shape[0])
    result["fixed_vertices"] = int(table[2].sum())
    for name in ("mesh_smooth", "inputs_check", "table", "half_steps"):
        t = result[name]
        print("%s: %.3f ms (quartiles %.3f .. %.3f)" % (name, t["median_ms"], t["q1_ms"], t["q3_ms"]), flush=True)
    with torch.no_grad():
        result["extract_meshes_smooth"] = timed(lambda: model.extract_meshes([code], False, MC_RES, THRESHOLD, smooth=a.iterations),
                                                a.runs, a.warmup)[1]
        result["extract_meshes_plain"] = timed(lambda: model.extract_meshes([code], False, MC_RES, THRESHOLD), a.runs, a.warmup)[1]
    print("extract_meshes: %.3f ms plain, %.3f ms with smooth=%d" % (result["extract_meshes_plain"]["median_ms"],
                                                                    result["extract_meshes_smooth"]["median_ms"], n), flush=True)
    if not a.no_host:
        few = max(1, min(a.runs, 3))
        back, result["host_round_trip"] = timed(lambda: host_route(v, f, n, lam, mu), few, 1)
        diff = float((back - out).abs().max())
        result["host_round_trip"]["max_abs_difference_to_device"] = diff      # the mat-vec sums a row in another order
        print("host round trip: %.1f ms (max |difference| to the device %.2e)" % (result["host_round_trip"]["median_ms"], diff), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
