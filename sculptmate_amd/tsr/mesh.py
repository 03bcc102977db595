"""Mesh -- what TSR.run and TSR.extract_meshes return per image -- and its device -> pinned-host hand-off (PendingMesh)."""
import math
import weakref

import numpy as np
import torch

from .. import ops
from . import passes as render_pass_rules


# What a mesh can carry beyond vertices and faces, by what each field is bound to (Mesh's docstring says what each one is)
VERTEX_FIELDS = ("vertex_colors", "vertex_normals", "vertex_occlusion")    # the vertex numbering: one row per vertex
CORNER_FIELDS = ("uvs", "corner_normals", "corner_tangents")               # the face corners: three rows per face
ATLAS_FIELDS = ("texture", "normal_map", "occlusion_map")                  # the atlas of `uvs`
MAP_TAGS = {"normal_map": "normal_map_space", "occlusion_map": "occlusion_map_rule"}   # a tag travels with its map
FACE_FIELDS = ("quads",)                                                   # the extractor's faces
TENSOR_FIELDS = VERTEX_FIELDS + CORNER_FIELDS + ATLAS_FIELDS               # what TSR.render_mesh moves to the device
FIELDS = TENSOR_FIELDS + tuple(MAP_TAGS.values()) + FACE_FIELDS


class Mesh:
    """What run() returns per image: trimesh-constructible arrays.  Beyond vertices and faces it can carry
    the FIELDS below -- plain attributes, None until set, five of them constructor parameters -- each bound to:
    the vertex numbering (VERTEX_FIELDS): vertex_colors, vertex_normals, vertex_occlusion (__init__ says what they hold).
    the face corners, 3 rows per face (CORNER_FIELDS): uvs; and the frame a tangent-space normal map is decoded in, which
      TSR.bake_normal_map adds: corner_normals f32 [3*Nf, 3], corner_tangents f32 [3*Nf, 4] = (T, w).
    the atlas of `uvs` (ATLAS_FIELDS, a map with its tag: MAP_TAGS): texture; normal_map f32 [res, res, 3], the unit normal
      encoded 0.5 + 0.5 n, row 0 at the top, with normal_map_space "tangent" | "object" (TSR.bake_normal_map); occlusion_map
      f32 [res, res], ambient occlusion, row 0 at the top, 1 = open, 0 = occluded, with occlusion_map_rule = (k, max_distance),
      the rule it was baked under (TSR.bake_occlusion_map).
    the extractor's faces (FACE_FIELDS): quads int [Nq, 4], the all-quad mesh over the same vertices that
      extract_meshes(isosurface="surface_nets") adds, while `faces` are still the extractor's -- faces[2q], faces[2q + 1] are
      quad q split along its shorter diagonal.  smooth and project keep it (faces and vertex numbering stay); keep_components,
      fill_holes, voxel_remesh, simplify and the triangle schemes of subdivide (Loop, midpoint) make new faces and drop it; subdivide with
      (n, "catmull_clark") sets it anew, to the refined quads, on any mesh.
    A step that makes one mesh from another names what it carries over (_derive); what it does not name is None on its result."""

    quads = None   # (a mesh object made before the attribute existed has none either)

    def __init__(self, vertices, faces, vertex_colors=None, uvs=None, texture=None, vertex_normals=None, vertex_occlusion=None):
        """uvs / texture: what TSR.bake_texture adds -- uvs f32 [3*Nf, 2] per face corner (origin bottom-left, the convention of
        sf3d and meshio.write_glb), texture f32 [res, res, 3] in [0, 1] with row 0 at the top.
        vertex_normals: f32 [Nv, 3] unit normals per shared vertex (extract_meshes(normals=...)), also on a baked mesh.
        vertex_occlusion: f32 [Nv] ambient occlusion per shared vertex, 1 = open, 0 = occluded (extract_meshes(occlusion=...),
        Mesh.ambient_occlusion), also on a baked mesh."""
        self.vertices, self.faces = vertices, faces
        given = dict(vertex_colors=vertex_colors, uvs=uvs, texture=texture, vertex_normals=vertex_normals, vertex_occlusion=vertex_occlusion)
        for name in FIELDS:
            setattr(self, name, given.get(name))

    def _derive(self, vertices, faces, carry=(), vertex_index=None, face_index=None, **new) -> "Mesh":
        """The mesh a step makes from this one: `vertices` and `faces`, the fields named in `carry` taken over from this mesh,
        the fields in `new` set to the values given, every other field None.  With vertex_index, what is bound to the vertex
        numbering is carried as field[vertex_index]; with face_index, what is bound to the face corners as field[corner],
        corner = face_index * 3 + (0, 1, 2).  A map takes its tag along.  A name that is no field is refused."""
        unknown = [name for name in (*carry, *new) if name not in FIELDS]
        if unknown:
            raise ValueError("Mesh._derive: %s: not a field a mesh carries (%s)" % (", ".join(map(repr, unknown)), ", ".join(FIELDS)))
        out, corner = Mesh(vertices, faces), None
        for name in carry:
            value = getattr(self, name)
            if value is not None and vertex_index is not None and name in VERTEX_FIELDS:
                value = value[vertex_index]
            elif value is not None and face_index is not None and name in CORNER_FIELDS:
                if corner is None:
                    three = torch.arange(3, device=face_index.device) if isinstance(face_index, torch.Tensor) else np.arange(3)
                    corner = (face_index[:, None] * 3 + three).reshape(-1)
                value = value[corner]
            setattr(out, name, value)
            if name in MAP_TAGS:
                setattr(out, MAP_TAGS[name], getattr(self, MAP_TAGS[name]))
        vars(out).update(new)
        return out

    def keep_components(self, keep) -> "Mesh":
        """The mesh without its small connected components (the "floaters" a thresholded density field leaves around the
        object): keep = "largest", an int >= 1 (components of at least that many faces) or a float in (0, 1) (at least that
        fraction of the largest component's faces) -- ops.mesh_keep_components on this mesh's device tensors (a mesh of host
        arrays, as TSR.run returns them, is refused there like any CPU tensor).  Rows keep their order; vertex_colors,
        vertex_normals and vertex_occlusion follow their vertices (vertex_index), the per-corner uvs of a baked mesh their faces (face_index, three
        rows per face); the texture is untouched (the dropped charts stay in it, unused).  A baked normal map
        (TSR.bake_normal_map) is carried the same way: the map as it is, corner_normals and corner_tangents through face_index; a
        baked occlusion map (TSR.bake_occlusion_map) as it is, with its rule."""
        v, f, vi, fi = ops.mesh_keep_components(self.vertices, self.faces, keep)
        return self._derive(v, f, VERTEX_FIELDS + CORNER_FIELDS + ATLAS_FIELDS, vertex_index=vi, face_index=fi)

    def simplify(self, simplify) -> "Mesh":
        """The mesh reduced to a target face count by quadric-error edge collapses on the device (ops.mesh_simplify): simplify =
        an int >= 1 (target faces) or a float in (0, 1) (ratio of the faces).  vertex_colors and vertex_normals follow
        vertex_index -- the values of the input vertex each output vertex descends from.  That is an approximation: the vertex
        has moved to its collapses' target point; TSR.extract_meshes(simplify=...) evaluates colours and normals at the final
        vertices instead.  vertex_occlusion is dropped: it is stale once the vertices have moved.  A baked mesh (uvs / texture)
        is refused: its atlas belongs to the faces it was baked for, so simplify
        before baking."""
        ops.simplify_rule(simplify)
        if self.uvs is not None or self.texture is not None:
            raise ValueError("Mesh.simplify: this mesh has a baked texture; simplify before baking "
                             "(TSR.extract_meshes(simplify=..., bake_texture=...))")
        v, f, vi = ops.mesh_simplify(self.vertices, self.faces, simplify)
        return self._derive(v, f, ("vertex_colors", "vertex_normals"), vertex_index=vi)

    def smooth(self, smooth) -> "Mesh":
        """The mesh after Taubin's lambda|mu smoothing on the device (ops.mesh_smooth): smooth = an int n, 1 <= n <= 1000
        (n iterations with lam = 0.5, mu = -0.53) or a tuple (n, lam, mu) (ops.smooth_rule).  The faces are the same tensor and
        the vertices keep their indices, so vertex_colors, uvs and texture are carried over as they are: the topology is
        unchanged and a baked atlas stays valid.  vertex_normals and vertex_occlusion are dropped: the vertices have moved and
        they would be stale (TSR.field_normals / ops.vertex_normals at the new vertices give fresh ones).  TSR.extract_meshes(smooth=...)
        smooths before it simplifies; this method lets a caller choose another order."""
        v = ops.mesh_smooth(self.vertices, self.faces, smooth)
        # (quads: the faces are the same, so the quads they came from still cover them)
        return self._derive(v, self.faces, ("vertex_colors", "uvs", "texture", "quads"))

    def subdivide(self, subdivide) -> "Mesh":
        """The mesh refined 1 -> 4 faces per level on the device (ops.mesh_subdivide): subdivide = an int n, 1 <= n <= 6 (n
        levels of the Loop scheme: the surface the mesh spans as a control cage) or a tuple (n, "loop" | "midpoint")
        (ops.subdivide_rule).  vertex_colors go through the same masks as the positions (attributes=), so they stay in their
        range.  vertex_normals and vertex_occlusion are dropped: they are stale on the refined surface.  A baked mesh
        (uvs / texture) is refused: its atlas belongs to the faces it was baked for, so subdivide before baking.
        (n, "catmull_clark") is the all-quad scheme (ops.mesh_catmull_clark): it starts from `quads` when the mesh has them,
        else from `faces` (a triangle becomes three quads), and the result carries the refined quads in `quads` and their
        split along the shorter diagonal in `faces`.  The Loop and midpoint schemes refine triangles and drop `quads`."""
        levels, scheme = ops.subdivide_rule(subdivide)
        if self.uvs is not None or self.texture is not None:
            raise ValueError("Mesh.subdivide: this mesh has a baked texture; subdivide before baking "
                             "(TSR.extract_meshes(subdivide=..., bake_texture=...))")
        if scheme == "catmull_clark":
            cage = self.faces if self.quads is None else self.quads
            v, q, f, colors = ops.mesh_catmull_clark(self.vertices, cage, levels, attributes=self.vertex_colors)
            return self._derive(v, f, vertex_colors=colors, quads=q)
        v, f, colors = ops.mesh_subdivide(self.vertices, self.faces, subdivide, attributes=self.vertex_colors)
        return self._derive(v, f, vertex_colors=colors)

    def sample_surface(self, n, seed=0):
        """n points uniform over this mesh's area (ops.mesh_sample_surface on its device tensors; host arrays are refused like
        any CPU tensor) -> (points f32 [n, 3], face i64 [n], uv f32 [n, 2]); the same (n, seed) gives the same bits."""
        return ops.mesh_sample_surface(self.vertices, self.faces, n, seed)

    def distance_to(self, other: "Mesh", samples=ops.DISTANCE_SAMPLES, seed=0, threshold=None) -> dict:
        """How far this surface is from `other`'s, whatever their topologies (ops.mesh_distance on the two meshes' device
        tensors): Chamfer and Hausdorff distance, mean / rms / max in both directions and, with a threshold, precision, recall
        and F-score.  samples=None measures from the meshes' own vertices: what an option such as smooth or simplify did to the
        surface, without sampling noise."""
        return ops.mesh_distance(self.vertices, self.faces, other.vertices, other.faces, samples=samples, seed=seed, threshold=threshold)

    def winding_number(self, points):
        """The integer winding counts of this mesh around each point along the three coordinate axes (ops.mesh_winding on its
        device tensors; host arrays are refused like any CPU tensor) -> int32 [N, 3]: +1 inside a closed surface wound outward,
        0 outside, on every axis."""
        return ops.mesh_winding(points, self.vertices, self.faces)

    def contains(self, points):
        """Which points lie inside this mesh (ops.mesh_contains) -> bool [N]: at least two of the three axis counts nonzero."""
        return ops.mesh_contains(points, self.vertices, self.faces)

    def signed_distance(self, points):
        """The distance of each point to this mesh, negative inside (ops.mesh_signed_distance)
        -> (sd f64 [N], face i64 [N], closest f32 [N, 3])."""
        return ops.mesh_signed_distance(points, self.vertices, self.faces)

    def voxel_remesh(self, voxel_remesh) -> "Mesh":
        """The mesh rebuilt from its inside on a voxel lattice (ops.mesh_voxel_remesh): voxel_remesh = an int R in 8 .. 1024
        (cells along the longest side of the bounds) or a tuple (R, band_cells) (ops.voxel_rule).  Overlapping parts fuse, the
        holes where the extractor met the box close, and smooth, simplify and subdivide get one clean closed surface to work on.
        The step makes new vertices and new faces, so it carries nothing over: vertex_colors, vertex_normals and
        vertex_occlusion, `quads`, uvs and every baked map are dropped (TSR.extract_meshes(voxel_remesh=...) evaluates colours
        and normals at the final vertices instead)."""
        v, f = ops.mesh_voxel_remesh(self.vertices, self.faces, voxel_remesh)
        return self._derive(v, f)

    def fill_holes(self, fill_holes=True) -> "Mesh":
        """The mesh with its border loops capped by fans on the device (ops.mesh_fill_holes): fill_holes = True (every loop) or an
        int max_edges >= 3 (loops of at most that many edges; ops.holes_rule).  Every existing vertex and face stays exactly as
        it is; a loop of four or more edges gets one new vertex at its centroid and a face per edge, a loop of three one face.
        vertex_colors are extended by the mean of each loop's colours (attributes=).  Everything else is dropped: the vertex rows
        of vertex_normals and vertex_occlusion would be short, uvs, corner_normals, corner_tangents and the baked maps have no
        rows for the new faces, and `quads` no longer cover the faces.  NOT claimed: a fan is a good cap for a short or roughly
        planar, star-shaped loop, and nothing more -- a long loop that wraps round an edge or a corner of the extraction box
        gets a fan that cuts through the mesh; max_edges is the control, report() (its self-intersections) the check, and
        voxel_remesh the answer for such loops."""
        v, f, colors, _ = ops.mesh_fill_holes(self.vertices, self.faces, fill_holes, attributes=self.vertex_colors)
        return self._derive(v, f, vertex_colors=colors)

    def border_loops(self) -> dict:
        """The border loops of this mesh as plain Python (ops.mesh_border_loops on its device tensors; host arrays are refused
        like any CPU tensor): border_half_edges, loops, open_half_edges, pinched_vertices, and `lengths`, the sorted list of the
        loops' edge counts -- what fill_holes(max_edges) would fill."""
        r = ops.mesh_border_loops(self.vertices, self.faces)
        out = {k: r[k] for k in ("border_half_edges", "loops", "open_half_edges", "pinched_vertices")}
        out["lengths"] = sorted(r["lengths"].tolist())
        return out

    def report(self, self_intersections=True) -> dict:
        """What this mesh is (ops.mesh_report on its device tensors; host arrays are refused like any CPU tensor): the edge
        census, Euler number, genus, area, volume and -- with self_intersections -- how many pairs of faces pass through each
        other.  A plain dict, computed on every call: no field of the mesh, nothing is stored."""
        return ops.mesh_report(self.vertices, self.faces, self_intersections=self_intersections)

    def self_intersections(self, pairs=False) -> dict:
        """Which faces of this mesh pass through each other (ops.mesh_self_intersections)
        -> {"count", "faces": bool [Nf], "pairs": int64 [count, 2] or None}."""
        return ops.mesh_self_intersections(self.vertices, self.faces, pairs=pairs)

    # trimesh's names, computed on demand from report(self_intersections=False); never cached
    @property
    def is_watertight(self) -> bool:
        return self.report(False)["is_watertight"]

    @property
    def is_winding_consistent(self) -> bool:
        return self.report(False)["is_winding_consistent"]

    @property
    def euler_number(self) -> int:
        return self.report(False)["euler"]

    @property
    def area(self) -> float:
        return self.report(False)["area"]

    @property
    def volume(self) -> float:
        return self.report(False)["volume"]

    def ray_cast(self, origins, directions, t_min=0.0, t_max=math.inf):
        """The closest face of this mesh that each ray hits (ops.mesh_ray_cast on its device tensors; host arrays are refused
        like any CPU tensor) -> (t f64 [N], face i64 [N], uv f32 [N, 2]); no hit: t = +inf, face = -1."""
        return ops.mesh_ray_cast(origins, directions, self.vertices, self.faces, t_min, t_max)

    def ambient_occlusion(self, occlusion=True, seed=0, outward=1.0):
        """Ambient occlusion per vertex -> f32 [Nv], 1 = open, 0 = occluded (ops.mesh_occlusion on this mesh's device tensors;
        host arrays are refused): the points are the vertices, the normals outward * ops.vertex_normals(vertices, faces) --
        always the facet-average normals of THIS mesh, whether or not vertex_normals is set.  occlusion: True (64 directions),
        k or (k, max_distance) (ops.occlusion_rule); seed rotates the direction set; outward: +1 when the faces wind
        counter-clockwise seen from outside, -1 otherwise (TSR.WINDING_OUTWARD for the meshes of TSR.extract_meshes).  The
        result is not stored: assign it to vertex_occlusion to carry and export it."""
        ops.occlusion_rule(occlusion)
        if not (ops._is_real(outward) and math.isfinite(float(outward))):
            raise ValueError("outward must be a finite number (+1 or -1), got %r" % (outward,))
        ops._device_mesh(self.vertices, self.faces, "Mesh.ambient_occlusion")
        normals = float(outward) * ops.vertex_normals(self.vertices, self.faces)
        return ops.mesh_occlusion(self.vertices, normals, self.vertices, self.faces, occlusion, seed=seed)

    def thickness(self, thickness=True, cone=60.0, seed=0, outward=1.0):
        """Wall thickness per vertex -- the shape diameter -> (thickness f32 [Nv], thinnest f32 [Nv], valid int32 [Nv])
        (ops.mesh_thickness on this mesh's device tensors; host arrays are refused): the points are the vertices, the normals
        outward * ops.vertex_normals(vertices, faces) -- always the facet-average normals of THIS mesh.  thickness: True (32
        rays), k or (k, max_distance) (ops.thickness_rule); cone: the half-angle of the cone about the inward normal, in
        degrees; seed rotates the cone set; outward: +1 when the faces wind counter-clockwise seen from outside, -1 otherwise
        (TSR.WINDING_OUTWARD for the meshes of TSR.extract_meshes).  thickness is the weighted mean length of the rays that
        leave the body through the back of a face, thinnest the shortest of them, valid their number (+inf, +inf, 0 when none
        did).  The result is returned, not stored."""
        ops._thickness_rules(thickness, cone, None, seed, outward)   # a ValueError before anything is launched
        ops._device_mesh(self.vertices, self.faces, "Mesh.thickness")
        normals = float(outward) * ops.vertex_normals(self.vertices, self.faces)
        return ops.mesh_thickness_route()(self.vertices, normals, self.vertices, self.faces, thickness, cone=cone, seed=seed,
                                          outward=float(outward))

    def curvature(self, curvature=True, outward=1.0):
        """Mean and Gaussian curvature per vertex -> (mean f32 [Nv], gauss f32 [Nv], valid bool [Nv]) (ops.mesh_curvature on this
        mesh's device tensors; host arrays are refused): the discrete operators of Meyer et al., mean positive where the surface
        is convex.  curvature: True or the number of rings in 0 .. 8 the integrated curvature is summed over (ops.curvature_rule;
        a few rings take the lattice noise of an extracted mesh out); outward: +1 when the faces wind counter-clockwise seen from
        outside, -1 otherwise (TSR.WINDING_OUTWARD for the meshes of TSR.extract_meshes).  Vertices on a border or a
        non-manifold edge are invalid and NaN.  The result is returned, not stored."""
        return ops.mesh_curvature(self.vertices, self.faces, curvature, outward)

    def render(self, rays_o, rays_d, passes=("color",), ambient=0.3, light=None, outward=1.0):
        """Pictures of this mesh with everything it carries -- uvs and texture, normal map and its frame, occlusion map, vertex
        colours, normals and occlusion -- ray cast on the device (ops.mesh_render on its device tensors; host arrays are refused
        like any CPU tensor).  rays_o, rays_d float [n_images, H, W, 3] or [N, 3] -> {pass: tensor} with the rays' leading
        shape; passes: any of "color", "shaded", "opacity", "rgba", "depth", "normal", "occlusion", "face" (ops.mesh_render has
        their values and backgrounds).  outward: +1 when the faces wind counter-clockwise seen from outside, -1 otherwise
        (TSR.WINDING_OUTWARD for the meshes of TSR.extract_meshes); it orients the face normal a mesh without a normal map
        and vertex normals is shaded with.  A map without the uvs it belongs to is not used."""
        has_uvs = self.uvs is not None
        return ops.mesh_render_route()(rays_o, rays_d, self.vertices, self.faces, passes=passes, uvs=self.uvs,
                                       texture=self.texture if has_uvs else None,
                                       normal_map=self.normal_map if has_uvs else None, normal_map_space=self.normal_map_space,
                                       corner_normals=self.corner_normals, corner_tangents=self.corner_tangents,
                                       occlusion_map=self.occlusion_map if has_uvs else None, vertex_colors=self.vertex_colors,
                                       vertex_normals=self.vertex_normals, vertex_occlusion=self.vertex_occlusion,
                                       ambient=ambient, light=light, outward=outward)

    def to_trimesh(self):  # pragma: no cover (trimesh is optional)
        import trimesh

        return trimesh.Trimesh(vertices=self.vertices, faces=self.faces, vertex_colors=self.vertex_colors)

    def _map_image(self, name, missing, grey=False):
        """What texture_image makes, of any picture over the atlas; a grey one [res, res] gets three equal channels."""
        from PIL import Image

        from ..sf3d.bake import float32_to_uint8_np

        if getattr(self, name) is None:
            raise ValueError(missing)
        picture = _host(getattr(self, name)).astype(np.float32)
        if grey:
            picture = np.repeat(picture[:, :, None], 3, axis=2)
        return Image.fromarray(float32_to_uint8_np(picture, dither=False))

    def texture_image(self):
        """The baked texture as a uint8 RGB PIL picture: floor(256 x) clipped to 0..255, no dither (deterministic)."""
        return self._map_image("texture", "Mesh.texture_image: this mesh has no baked texture (TSR.bake_texture)")

    def normal_map_image(self):
        """The baked normal map as a uint8 RGB PIL picture, as texture_image makes one: floor(256 x) clipped to 0..255, no dither."""
        return self._map_image("normal_map", "Mesh.normal_map_image: this mesh has no baked normal map (TSR.bake_normal_map)")

    def occlusion_map_image(self):
        """The baked occlusion map as a uint8 RGB PIL picture with three equal channels (glTF reads the red one), quantised as
        normal_map_image quantises: floor(256 x) clipped to 0..255, no dither."""
        return self._map_image("occlusion_map", "Mesh.occlusion_map_image: this mesh has no baked occlusion map (TSR.bake_occlusion_map)", grey=True)

    def export(self, path, displacement=None):
        """Write .obj / .ply / .glb by extension (sculptmate_amd/meshio.py), the call upstream users make on the
        trimesh object their extract_mesh returns.  A baked mesh (uvs + texture) goes out textured: .glb with TEXCOORD_0 and the
        base-colour texture (glTF has one index per vertex, so positions are un-indexed to 3*Nf vertices there and only there),
        .obj with `vt` lines, `f v/vt` faces and a .mtl + .png beside the file (positions stay shared).  vertex_normals, when the
        mesh has them, go into every format (glTF NORMAL, `vn`, nx ny nz); the un-indexed .glb gets normals[faces] per corner.
        vertex_occlusion, when set, goes into .ply (a float property `ao`) and .glb (the custom attribute _OCCLUSION; the
        un-indexed .glb gets ao[faces] per corner); .obj has no slot for it.
        A baked normal map (TSR.bake_normal_map; uvs + normal_map, with or without a texture) goes the textured way too.  A
        tangent-space map: .glb gets normalTexture, NORMAL from corner_normals and TANGENT (VEC4) from corner_tangents, the frame
        it was baked in; .obj gets `map_Bump -bm 1 NAME_normal.png` in the .mtl and the PNG beside it.  An object-space map is
        never written as glTF's normalTexture (which is tangent space by definition): the .glb carries it as a further PNG image
        that no material refers to, named in the mesh's extras ({"images": {"normal_map_object": index}}); the .obj gets the
        same map_Bump line, to be read as object space by whoever asked for one.
        An unbaked mesh with quads (extract_meshes(isosurface="surface_nets")) goes into .obj as quads, `f a b c d`; .ply, .glb
        and every baked path write the triangles.
        A baked occlusion map (TSR.bake_occlusion_map; uvs + occlusion_map, with or without a texture or normal map) goes the
        textured way as well: .glb gets material.occlusionTexture (three equal channels; glTF reads the red one, strength at its
        default of 1), .obj gets `map_Ka NAME_ao.png` in the .mtl and the PNG beside it.
        displacement: a tsr.displacement.DisplacementMap baked over this mesh's atlas (TSR.bake_displacement_map; the mesh needs
        its uvs) goes the textured way as a 16-bit grey PNG: .obj gets `disp -mm <-scale/2> <scale> NAME_disp.png` in the .mtl
        and the PNG beside it; .glb gets it as a further image named in the mesh's extras with `scale` and `midlevel` (glTF has
        no core displacement slot, so it follows the object-space normal map).  None (default): every file is byte for byte
        what it was without the keyword.  .ply has no slot for it."""
        from .. import meshio

        ext = str(path).rsplit(".", 1)[-1].lower()
        writer = {"obj": meshio.write_obj, "ply": meshio.write_ply, "glb": meshio.write_glb}.get(ext)
        if writer is None:
            raise ValueError(f"unsupported mesh format .{ext} (obj, ply, glb)")
        if displacement is not None and self.uvs is None:
            raise ValueError("Mesh.export: a displacement map belongs to an atlas; this mesh has no uvs (TSR.bake_displacement_map returns the mesh with them)")
        baked = self.texture is not None or self.normal_map is not None or self.occlusion_map is not None or displacement is not None
        if self.uvs is not None and baked and ext in ("glb", "obj"):
            v, f, uv = _host(self.vertices), _host(self.faces), _host(self.uvs)
            picture = None if self.texture is None else np.asarray(self.texture_image())
            vn = None if self.vertex_normals is None else _host(self.vertex_normals)
            bump = None if self.normal_map is None else np.asarray(self.normal_map_image())
            shade = None if self.occlusion_map is None else np.asarray(self.occlusion_map_image())
            if ext == "glb":
                extra = {} if self.vertex_occlusion is None else {"occlusion": _host(self.vertex_occlusion)[f.reshape(-1)]}
                if shade is not None:
                    extra["occlusion_tex"] = shade
                normals = None if vn is None else vn[f.reshape(-1)]
                if bump is not None:   # the frame the map was baked in, per corner
                    if self.corner_normals is not None:
                        normals = _host(self.corner_normals)
                    if self.normal_map_space == "tangent":
                        extra["normal_tex"] = bump
                        if self.corner_tangents is not None:
                            extra["tangents"] = _host(self.corner_tangents)
                    else:
                        extra["extra_images"] = {"normal_map_object": bump}
                meshio.write_glb(str(path), v[f.reshape(-1)], np.arange(f.size, dtype=np.int64).reshape(-1, 3), uvs=uv,
                                 basecolor_tex=picture, normals=normals, **extra)
                if displacement is not None:
                    meshio.add_glb_displacement(str(path), displacement.png_bytes(), displacement.scale, displacement.midlevel)
            else:
                extra = {} if bump is None else {"normal_map": bump}
                if shade is not None:
                    extra["occlusion_map"] = shade
                meshio.write_obj_textured(str(path), v, f, uv, picture, normals=vn, **extra)
                if displacement is not None:
                    meshio.add_obj_displacement(str(path), displacement.png_bytes(), displacement.scale)
            return
        extra = {} if self.vertex_occlusion is None or ext == "obj" else {"occlusion": _host(self.vertex_occlusion)}
        if ext == "obj" and self.quads is not None:   # the all-quad mesh of surface nets: `f a b c d` lines (.ply and .glb stay triangles)
            extra["quads"] = _host(self.quads)
        writer(str(path), self.vertices, self.faces, vertex_colors=self.vertex_colors, normals=self.vertex_normals, **extra)


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _mesh_pass_to_pil(name, image):
    """One view of a pass of TSR.render_mesh as a PIL image: the passes tsr/passes.py knows as it makes them, "shaded" as
    "color" (clipped first: a light can exceed 1), "occlusion" as "opacity" (L), "face" as mode I (int32, untouched)."""
    from PIL import Image

    if name == "face":
        return Image.fromarray(np.ascontiguousarray(image, dtype=np.int32))
    if name == "shaded":
        return render_pass_rules.to_pil("color", np.clip(np.nan_to_num(np.asarray(image, np.float32)), 0.0, 1.0))
    return render_pass_rules.to_pil("opacity" if name == "occlusion" else name, image)


class _PinnedPool:
    """Pinned host buffers for the mesh hand-off, recycled by size class (next power of two of the byte count).  A pinned
    allocation is a driver call of ~0.5 ms that can stall the device queue; mesh sizes differ from image to image, so an
    exact-size cache never hits."""

    def __init__(self):
        self.free = {}

    def take(self, shape, dtype):
        n = math.prod(int(d) for d in shape)
        esize = torch.empty((), dtype=dtype).element_size()
        nbytes = n * esize
        cap = 1 << (max(nbytes, 16) - 1).bit_length()   # at least one element of any dtype: an empty mesh array gets a real buffer
        lst = self.free.get(cap)
        buf = lst.pop() if lst else torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        view = buf[:max(nbytes, esize)].view(dtype)[:n].view(shape)
        return _PinnedLease(self, cap, buf), view

    def give(self, cap, buf):
        self.free.setdefault(cap, []).append(buf)


class _PinnedLease:
    """One pinned buffer on loan.  It goes back to the pool when the lease dies -- or, once `hand_over(array)` has tied it to
    the NumPy array that views it, when THAT array (and every view of it) is gone."""

    def __init__(self, pool, cap, buf):
        self.pool, self.cap, self.buf = pool, cap, buf

    def hand_over(self, array):
        pool, cap, buf = self.pool, self.cap, self.buf
        self.buf = None
        weakref.finalize(array, pool.give, cap, buf)

    def __del__(self):
        try:
            if self.buf is not None:
                self.pool.give(self.cap, self.buf)
        except Exception:  # interpreter shutdown
            pass


class PendingMesh:
    """A mesh whose device -> pinned-host copy is in flight (TSR.run_async)."""

    def __init__(self, host_tensors, done_event, leases=()):
        self._host = host_tensors
        self._done = done_event
        self._leases = leases
        self._mesh = None

    def done(self) -> bool:
        return self._done.query()

    def result(self) -> Mesh:
        """The arrays are views of pinned host buffers; a buffer returns to the pool when its array -- and every view or
        slice taken from it -- has been released (it does not matter whether the Mesh object itself is kept)."""
        if self._mesh is None:
            self._done.synchronize()
            arrays = [None if t is None else t.numpy() for t in self._host]
            for lease, a in zip(self._leases, [a for a in arrays if a is not None]):
                lease.hand_over(a)
            # later calls return the SAME Mesh: a second set of views would carry no lease, and the buffers could go back to
            # the pool (and be overwritten by a later run_async) while it is still alive
            self._leases, self._host = (), None
            self._mesh = Mesh(arrays[0], arrays[1], arrays[2], vertex_normals=arrays[3])
        return self._mesh
