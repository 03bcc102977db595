"""Time the mesh render (csrc/mesh_ray.hip sculpt_surface_render, ops.mesh_render) on the assets it is meant to show, and
measure those assets against the field they came from: the 256^3 mesh of the full-size TSR with seeded weights and vertex
colours (the HIGH mesh), and simplify=0.1 of it carrying the three baked maps -- texture, tangent-space normal map, occlusion map
against the high mesh -- at 2048^2 (the LOW mesh); 8 turntable views at 512^2, all passes.

    python tools/time_mesh_render.py [--runs 7] [--warmup 2] [--views 8] [--size 512] [--res 2048] [--out profiles/time_mesh_render.json]

Per mesh: the fused kernel against the composed route (ops.mesh_render_composed's stages) on the same rays and the same prebuilt
index, whose bits it must equal, and the index build on its own.  Per mesh and view, against TSR.render_passes of the same
cameras (pixel (i, j) of view k is the same ray in both renderers):
    psnr_color        of the mesh's "color" against the field's picture on white, over the whole picture (peak 1)
    opacity_agree     the share of pixels on which "opacity" and (the field's opacity > 0.5) agree
    depth_mean / p99  of |depth_mesh - depth_field| in lattice cells (2 radius / 255) where both are opaque
    normal_angle_deg  the mean angle between "normal" and the field's normal pass where both are opaque
    field_opaque      the share of pixels on which the field's opacity is > 0.5 (what the four above are to be read with)
A volume render integrates whatever density lies in front of the iso-surface, so those four say as much about the field as
about the mesh.  Beside them, per mesh over all views, the field read AT the point the mesh render reports (o + depth d):
    at_hit.color_psnr        "color" against the colour field at the hit points (the texture, or the vertex colours, decoded)
    at_hit.normal_angle_deg  mean and p99 of the angle between "normal" and TSR.field_normals at the hit points -- for the low
                             mesh the normal map decoded through the exported uvs and tangent frames, against what it was baked from
    at_hit.face_normal_angle_deg  the same for the faces' own normals (the mesh rendered without its maps): what the map is to beat
    at_hit.density_log_ratio mean |ln(density / threshold)| at the hit points: how far from the iso-surface the mesh lies

Device times: wall clock around the call with a final torch.cuda.synchronize(), after warm-up calls; median and quartiles over
the runs (the quartiles are the run-to-run spread).  No threshold is set here."""
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


def _same_bits(a, b):
    """Equal bit for bit, a NaN equal to any NaN."""
    if a.dtype.is_floating_point:
        return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())
    return torch.equal(a, b)


def _mean(xs):
    return sum(xs) / max(len(xs), 1)


def against_field(mesh_views, field_views, cell):
    """The four figures per view -> a list of dicts."""
    out = []
    for mv, fv in zip(mesh_views, field_views):
        mse = float(((mv["color"].double() - fv["color"].double()) ** 2).mean())
        solid_m, solid_f = mv["opacity"] > 0.5, fv["opacity"] > 0.5
        both = solid_m & solid_f
        entry = {"psnr_color": 10.0 * math.log10(1.0 / mse) if mse > 0 else math.inf,
                 "opacity_agree": float((solid_m == solid_f).float().mean()), "both_opaque": int(both.sum()),
                 "field_opaque": float(solid_f.float().mean())}
        if int(both.sum()):
            dd = ((mv["depth"] - fv["depth"]).abs()[both] / cell).double()
            entry["depth_mean_cells"] = float(dd.mean())
            entry["depth_p99_cells"] = float(torch.quantile(dd[:: max(1, dd.numel() // 1_000_000)], 0.99))
            cos = (mv["normal"] * fv["normal"]).sum(-1)[both].clamp(-1.0, 1.0)
            entry["normal_angle_deg"] = float(torch.rad2deg(torch.acos(cos)).mean())
        out.append(entry)
    return out


def at_hit(model, code, rays_o, rays_d, fused, threshold, face_normal):
    """The field at the points the mesh render reports -> the three figures over all hit pixels of all views."""
    hit = fused["face"] >= 0
    pts = (rays_o + fused["depth"][..., None] * rays_d)[hit].contiguous()
    with torch.no_grad():
        field = model.renderer.query_triplane(model.decoder, pts, code)
        normal = model.field_normals(pts, code)
    mse = float(((fused["color"][hit].double() - field["color"].double()) ** 2).mean())
    cos = (fused["normal"][hit] * normal).sum(-1).clamp(-1.0, 1.0)
    angle = torch.rad2deg(torch.acos(cos)).double()
    flat = torch.rad2deg(torch.acos((face_normal[hit] * normal).sum(-1).clamp(-1.0, 1.0))).double()
    ratio = (field["density_act"].reshape(-1).double().clamp_min(1e-30) / threshold).log().abs()
    return {"points": int(pts.shape[0]), "color_psnr": 10.0 * math.log10(1.0 / mse) if mse > 0 else math.inf,
            "normal_angle_deg": float(angle.mean()),
            "normal_angle_p99_deg": float(torch.quantile(angle[:: max(1, angle.numel() // 1_000_000)], 0.99)),
            "face_normal_angle_deg": float(flat.mean()), "density_log_ratio": float(ratio.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_mesh_render.json"))
    a = ap.parse_args()

    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.cameras import get_spherical_cameras

    dev = torch.device("cuda:0")
    model, code, _ = seeded_mesh(dev, MC_RES, THRESHOLD)
    with torch.no_grad():
        high = model.extract_meshes([code], True, MC_RES, THRESHOLD)[0]
        low = model.extract_meshes([code], True, MC_RES, THRESHOLD, bake_texture=a.res, simplify=SIMPLIFY)[0]
        low = model.bake_normal_map(low, code)
        low = model.bake_occlusion_map(low, source=high)
        field_views = model.render_passes([code], a.views, height=a.size, width=a.size, passes=("color", "opacity", "depth", "normal"))[0]
    torch.cuda.synchronize()
    rays_o, rays_d = get_spherical_cameras(a.views, 0.0, 1.9, 40.0, a.size, a.size)
    rays_o, rays_d = rays_o.to(dev), rays_d.to(dev)
    cell = 2.0 * float(model.renderer.cfg.radius) / (MC_RES - 1)
    passes = tuple(ops.MESH_RENDER_PASSES)
    result = {"device": torch.cuda.get_device_name(0), "mc_resolution": MC_RES, "simplify": SIMPLIFY, "map_resolution": a.res,
              "views": a.views, "size": a.size, "rays": a.views * a.size * a.size, "passes": list(passes), "lattice_cell": cell}
    ok = True
    for name, mesh in (("high", high), ("low", low)):
        material = ops._render_material(mesh.uvs, mesh.texture, mesh.normal_map, mesh.normal_map_space, mesh.corner_normals, mesh.corner_tangents,
                                 mesh.occlusion_map, mesh.vertex_colors, mesh.vertex_normals, mesh.vertex_occlusion)

        def job(which=passes):
            return ops._RenderJob("time_mesh_render", rays_o, rays_d, mesh.vertices, mesh.faces, which, material, 0.3, None,
                                  TSR.WINDING_OUTWARD)

        P, F = ops._surface(mesh.vertices, mesh.faces, "time_mesh_render")
        _, build = timed(lambda: ops._SurfaceIndex(P, F).records(), a.runs, a.warmup)
        entry = {"vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0]), "index_build": build,
                 "material": sorted(k for k, v in material.items() if v is not None)}
        for label, which in (("all_passes", passes), ("color_only", ("color",))):
            j = job(which)
            j.index.records()
            fused, t_fused = timed(lambda: ops._mesh_render_fused(j), a.runs, a.warmup)
            comp, t_comp = timed(lambda: ops._mesh_render_composed(j), max(1, min(a.runs, 5)), 1)
            same = all(_same_bits(fused[p], comp[p]) for p in which)
            ok = ok and same
            entry[label] = {"fused": t_fused, "composed": t_comp, "same_bits": same,
                            "composed_over_fused": t_comp["median_ms"] / t_fused["median_ms"]}
            print("%s, %s: fused %.3f ms (%.3f .. %.3f), composed %.3f ms (%.3f .. %.3f), ratio %.2f, same bits: %s" % (
                name, label, t_fused["median_ms"], t_fused["q1_ms"], t_fused["q3_ms"], t_comp["median_ms"], t_comp["q1_ms"],
                t_comp["q3_ms"], entry[label]["composed_over_fused"], same), flush=True)
            if label == "all_passes":
                views = [{p: fused[p][k] for p in which} for k in range(a.views)]
                bare = ops.mesh_render(rays_o, rays_d, mesh.vertices, mesh.faces, passes=("normal",), outward=TSR.WINDING_OUTWARD)
                entry["at_hit"] = at_hit(model, code, rays_o, rays_d, fused, THRESHOLD, bare["normal"])
        per_view = against_field(views, field_views, cell)
        entry["per_view"] = per_view
        entry["hit_share"] = float(_mean([float((v["face"] >= 0).float().mean()) for v in views]))
        entry["mean"] = {k: _mean([v[k] for v in per_view if k in v]) for k in ("psnr_color", "opacity_agree", "depth_mean_cells",
                                                                                 "depth_p99_cells", "normal_angle_deg", "field_opaque")}
        result[name] = entry
        print("%s: %d faces, index build %.3f ms, %.1f%% of the rays hit; against the field, mean over %d views: PSNR %.2f dB, opacity "
              "agrees on %.3f%% (the field is opaque on %.3f%%), depth off by %.3f cells (p99 %.3f), normals %.2f degrees apart; the field "
              "at the %d hit points: colour PSNR %.2f dB, normals %.2f degrees apart (p99 %.2f; the faces' own %.2f), |ln(density / threshold)| %.4f" % (
                  name, entry["faces"], build["median_ms"], 100 * entry["hit_share"], a.views, entry["mean"]["psnr_color"],
                  100 * entry["mean"]["opacity_agree"], 100 * entry["mean"]["field_opaque"], entry["mean"]["depth_mean_cells"],
                  entry["mean"]["depth_p99_cells"], entry["mean"]["normal_angle_deg"], entry["at_hit"]["points"],
                  entry["at_hit"]["color_psnr"], entry["at_hit"]["normal_angle_deg"], entry["at_hit"]["normal_angle_p99_deg"],
                  entry["at_hit"]["face_normal_angle_deg"], entry["at_hit"]["density_log_ratio"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": a.out}))
    assert ok, "the fused and the composed route differ"


if __name__ == "__main__":
    main()
