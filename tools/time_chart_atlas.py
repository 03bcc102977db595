"""Time and describe the two UV unwrappers -- sf3d.unwrap.BoxProjectionUnwrapper and sf3d.unwrap.ChartUnwrapper (csrc/uv_charts.hip)
-- on the meshes the bakes run over: the 256^3 mesh of the full-size TSR with seeded weights, simplify=0.1 of it and
keep_components="largest" of it; and on three nested icospheres, where box projection has to push a layer into "remaining".

    python tools/time_chart_atlas.py [--runs 5] [--warmup 1] [--res 2048] [--out profiles/time_chart_atlas.json]

Per mesh and unwrapper, both in the same run and timed in both orders (box, charts, charts again, box again): the time of the
unwrap; for the chart unwrapper its time per stage, rounds, evictions, charts and single-face charts; the seam edges (manifold
edges whose two faces hold different UV bits at a shared vertex) and the faces all of whose edges are seams; the coverage at
res^2 (share of texels ops.bake_rasterize covers).  On the simplified mesh also the fused and the composed route of the
occlusion bake (the mesh against itself) and of the surface bake, over each atlas.

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; medians and quartiles.
These are measurements; no threshold is set here and no default depends on them."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import seeded_mesh, timed  # noqa: E402

MC_RES, THRESHOLD, SIMPLIFY = 256, 25.0, 0.1


def icosphere(levels, radius):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in
         [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
          (-t, 0, -1), (-t, 0, 1)]]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int64)


def nested_icospheres(dev, levels=5):
    vs, fs, off = [], [], 0
    for r in (1.0, 0.7, 0.4):
        v, f = icosphere(levels, r)
        vs.append(v); fs.append(f + off); off += len(v)
    return torch.from_numpy(np.concatenate(vs)).to(dev), torch.from_numpy(np.concatenate(fs)).to(dev)


def seams(f, uv):
    """(manifold edges, seam edges among them, faces all of whose three edges are seams or not manifold)."""
    nf = f.shape[0]
    flat = f.reshape(-1).long()
    nxt = (torch.arange(3 * nf, device=f.device) // 3) * 3 + (torch.arange(3 * nf, device=f.device) % 3 + 1) % 3
    a, b = flat, flat[nxt]
    key = (torch.minimum(a, b) << 32) | torch.maximum(a, b)
    skey, order = torch.sort(key, stable=True)
    head = torch.ones_like(skey, dtype=torch.bool)
    head[1:] = skey[1:] != skey[:-1]
    start = torch.nonzero(head)[:, 0]
    count = torch.diff(torch.cat([start, torch.tensor([3 * nf], device=f.device)]))
    two = start[count == 2]
    h0, h1 = order[two], order[two + 1]
    lo = torch.minimum(a[h0], b[h0])
    bits = uv.view(torch.int32).reshape(-1, 2)

    def corner(h, want_lo):
        at_start = (a[h] == lo) == want_lo
        return torch.where(at_start, h, nxt[h])

    seam = torch.zeros(two.shape[0], dtype=torch.bool, device=f.device)
    for want_lo in (True, False):
        seam |= (bits[corner(h0, want_lo)] != bits[corner(h1, want_lo)]).any(1)
    joined = torch.zeros(3 * nf, dtype=torch.bool, device=f.device)   # half-edges across which the UVs continue
    joined[h0[~seam]] = True
    joined[h1[~seam]] = True
    alone = int((~joined.view(nf, 3).any(1)).sum())
    return int(two.shape[0]), int(seam.sum()), alone


def describe(f, uv, res):
    from sculptmate_amd import ops

    corners = torch.arange(3 * f.shape[0], device=f.device, dtype=torch.int32).view(-1, 3)
    rast = ops.bake_rasterize(uv, corners, res)
    manifold, seam, alone = seams(f, uv)
    return {"coverage": float((rast[..., 3] >= 0).float().mean()), "manifold_edges": manifold, "seam_edges": seam,
            "faces_without_a_continued_edge": alone}, rast


def bakes(model, code, v, f, uv, rast, runs, warmup):
    """The fused and the composed route of the occlusion bake (the mesh against itself) and of the surface bake over one atlas."""
    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR

    dev = v.device
    out = {}
    nrm = (TSR.WINDING_OUTWARD * ops.vertex_normals(v, f)).contiguous()
    dirs = torch.from_numpy(ops.occlusion_directions(64, 0)).to(dev)
    P, F = ops._surface(v, f, "time_chart_atlas")
    index = ops._SurfaceIndex(P, F)
    index.records()
    offset = float(np.float32(ops.OCCLUSION_OFFSET * index.longest_side()))
    args = (index, v, f, nrm, rast, dirs, offset, math.inf, 0.0)
    out["occlusion"] = {"fused": timed(lambda: ops._bake_occlusion_fused(*args), runs, warmup)[1],
                        "composed": timed(lambda: ops._bake_occlusion_composed(*args), runs, warmup)[1]}
    cfg = model.renderer.cfg
    steps, cells = ops.project_rule(True)
    target = float(np.float32(math.log(THRESHOLD) - float(cfg.density_bias)))
    max_dist = cells * 2.0 * float(cfg.radius) / (MC_RES - 1)
    planes = ops.ChannelLastPlanes(code)
    cn = (model.WINDING_OUTWARD * ops.vertex_normals(v, f))[f.reshape(-1).long()].contiguous()
    ct = ops.corner_tangents(v, f, uv, cn)
    kw = dict(steps=steps, radius=cfg.radius, frame=(cn, ct))
    out["surface"] = {
        "fused": timed(lambda: ops.bake_scene_surface(planes, model.decoder, v, f, rast, target, max_dist, **kw), runs, warmup)[1],
        "composed": timed(lambda: ops.bake_scene_surface_composed(planes, model.decoder, v, f, rast, target, max_dist, **kw), runs, warmup)[1]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_chart_atlas.json"))
    a = ap.parse_args()
    from sculptmate_amd import ops
    from sculptmate_amd._lib import SculptError
    from sculptmate_amd.sf3d.unwrap import BoxProjectionUnwrapper, ChartUnwrapper

    dev = torch.device("cuda:0")
    model, code, full = seeded_mesh(dev, MC_RES, THRESHOLD)
    low = ops.mesh_simplify(full.vertices, full.faces, SIMPLIFY)[:2]
    largest = ops.mesh_keep_components(full.vertices, full.faces, "largest")[:2]
    meshes = [("mc256", (full.vertices, full.faces)), ("simplify_0.1", low), ("largest_component", largest),
              ("nested_icospheres", nested_icospheres(dev))]
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "resolution": a.res,
              "island_padding": 0.02, "meshes": {}}
    box, charts = BoxProjectionUnwrapper(), ChartUnwrapper()
    for name, (v, f) in meshes:
        v, f = v.to(torch.float32).contiguous(), f.contiguous()
        nrm = ops.vertex_normals(v, f)
        entry = {"vertices": int(v.shape[0]), "faces": int(f.shape[0])}
        try:
            uv_b, t_box = timed(lambda: box(v, nrm, f, 0.02)[0], a.runs, a.warmup)
            uv_c, t_charts = timed(lambda: charts(v, nrm, f, 0.02)[0], a.runs, a.warmup)
            _, t_charts2 = timed(lambda: charts(v, nrm, f, 0.02)[0], a.runs, a.warmup)
            _, t_box2 = timed(lambda: box(v, nrm, f, 0.02)[0], a.runs, a.warmup)
        except SculptError as e:
            entry["error"] = str(e)
            result["meshes"][name] = entry
            print("%s: %s" % (name, e), flush=True)
            continue
        last = charts.last
        sizes = torch.bincount(last["chart"].long(), minlength=last["n_charts"])
        charts.stage_ms = {}
        charts(v, nrm, f, 0.02)
        stages, charts.stage_ms = {k: round(x, 4) for k, x in charts.stage_ms.items()}, None
        d_box, rast_b = describe(f, uv_b.contiguous(), a.res)
        d_charts, rast_c = describe(f, uv_c, a.res)
        entry.update(box=dict(d_box, unwrap=t_box, unwrap_again=t_box2),
                     charts=dict(d_charts, unwrap=t_charts, unwrap_again=t_charts2, stages_ms_one_call=stages, n_charts=last["n_charts"],
                                 single_face_charts=int((sizes == 1).sum()), largest_chart_faces=int(sizes.max()),
                                 rows=last["rows"], rounds=last["rounds"], evicted=last["evicted"], conflicts=last["conflicts"],
                                 scale=last["scale"], scale_evaluations_last_round=last["evaluations"],
                                 faces_per_layer=torch.bincount(last["layer"].long()).tolist()))
        if name == "simplify_0.1":
            entry["box"]["bakes"] = bakes(model, code, v, f, uv_b.contiguous(), rast_b, a.runs, a.warmup)
            entry["charts"]["bakes"] = bakes(model, code, v, f, uv_c, rast_c, a.runs, a.warmup)
        result["meshes"][name] = entry
        print("%s (%d faces): box %.2f ms (again %.2f), coverage %.1f %%, seams %d of %d, lone faces %d | charts %.2f ms (again %.2f), "
              "coverage %.1f %%, seams %d, lone faces %d, %d charts (%d single), rounds %d, evicted %s, stages %s" % (
                  name, f.shape[0], t_box["median_ms"], t_box2["median_ms"], 100 * d_box["coverage"], d_box["seam_edges"],
                  d_box["manifold_edges"], d_box["faces_without_a_continued_edge"], t_charts["median_ms"], t_charts2["median_ms"],
                  100 * d_charts["coverage"], d_charts["seam_edges"], d_charts["faces_without_a_continued_edge"], last["n_charts"],
                  entry["charts"]["single_face_charts"], last["rounds"], last["evicted"], stages), flush=True)
        for which in ("box", "charts"):
            if "bakes" in entry[which]:
                b = entry[which]["bakes"]
                print("  %s atlas: occlusion fused %.2f ms, composed %.2f ms; surface fused %.2f ms, composed %.2f ms" % (
                    which, b["occlusion"]["fused"]["median_ms"], b["occlusion"]["composed"]["median_ms"],
                    b["surface"]["fused"]["median_ms"], b["surface"]["composed"]["median_ms"]), flush=True)
        with open(a.out, "w") as fh:   # after every mesh: a later mesh that fails loses nothing
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
