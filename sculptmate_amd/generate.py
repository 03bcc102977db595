"""TripoGenerator: what `GUIPanel.py:11` imports from `TripoSR/generate.py` -- same constructor argument, public
attributes (`checkpoint_dir`, `chunk_size`, `mc_resolution`, `image_path`, `device`, `model`) and return codes
(generate.py:9-43), running on the MI355X kernels."""
import os

import torch

from ._facade import STATUS_FAILED, STATUS_NOT_LOADED, STATUS_OK, GeneratorFacade
from .tsr.system import TSR

ROOT_DIR = os.path.dirname(os.path.abspath(__file__))


class TripoGenerator(GeneratorFacade):
    """One attribute beyond the reference's: `precision`, the arithmetic of the transformer, read when the model is constructed
    (initiate_model):
      "bf16"   (default; BASELINE config 2) bf16 storage, fp32 accumulate -- the fast mode; the scene code moves by ~0.8 % against
               the fp32 reference, i.e. the mesh is within 1e-4 of it only GIVEN the same scene code;
      "fp16l2" the faster of the two modes that meet the 1e-4 vertex tolerance against the reference's fp32 CPU path end to end:
               fp32 storage, the Linears and the backbone's attention with two fp16 limbs per operand (22 bits), fp32 accumulate
               (~2.4x the forward time); an image whose activations leave the fp16 range is redone on three bf16 limbs;
      "bf16l3" the same tolerance with the fp32 exponent range: every matrix product with both operands split exactly into three
               bf16 limbs, fp32 accumulate (~3.6x the forward time);
      "fp32"   the exact-fp32 matrix instruction (slowest; the parity yard-stick).
    The environment variable SCULPT_PRECISION overrides the default for an add-on that cannot be edited.
    `bake_texture_resolution` (default 0): with the add-on's texture tick box set (generate_mesh(enable_texture=True)), a value
    above 0 bakes a UV texture of that size from the scene code (TSR.bake_texture; upstream's default is 2048) instead of one
    colour per vertex.
    `vertex_normals` (default None): "field" leaves smooth unit normals on the meshes in `last_meshes` (Mesh.vertex_normals, the
    gradient of the density field at each vertex: TSR.field_normals), "faces" the averaged facet normals; Mesh.export writes
    them.  The Blender sinks take none: Blender shades shared vertices smooth by itself.
    `keep_components` (default None): "largest", an int >= 1 (minimum faces) or a float in (0, 1) (fraction of the largest
    component's faces) drops the other connected components of every mesh -- the floaters around the object -- on the device
    before it is coloured, baked or handed to Blender (TSR.extract_meshes).
    `simplify` (default None): an int >= 1 (target faces) or a float in (0, 1) (ratio of the faces) reduces every mesh by
    quadric-error edge collapses on the device, after keep_components and before the colours, the bake and the normals
    (TSR.extract_meshes; ops.mesh_simplify).
    `smooth` (default None): an int n in 1 .. 1000 (iterations, lam = 0.5, mu = -0.53) or a tuple (n, lam, mu) smooths every mesh
    with Taubin's lambda|mu filter on the device, after keep_components and before simplify (TSR.extract_meshes;
    ops.mesh_smooth).
    `project` (default None): True (8 Newton steps inside one lattice cell), an int n in 1 .. 64 or a tuple (n, cells) moves the
    vertices of every mesh onto the iso-surface of the density field itself and undoes folded faces, as the last geometry
    step -- after keep_components, smooth, simplify and subdivide, before the colours, the bake and the normals
    (TSR.extract_meshes; ops.mesh_project).
    `subdivide` (default None): an int n in 1 .. 6 (levels of the Loop scheme) or a tuple (n, "loop" | "midpoint") refines every
    mesh 1 -> 4 faces per level on the device, after simplify and before project: the simplified mesh becomes the control cage
    of a semi-regular, multires-friendly surface (TSR.extract_meshes; ops.mesh_subdivide).  (n, "catmull_clark") is the
    all-quad scheme of Blender's Subdivision Surface and Multires modifiers: it refines the quads of isosurface="surface_nets",
    or turns every triangle into three quads, and the plain sink receives the refined quads (ops.mesh_catmull_clark).
    `voxel_remesh` (default None): an int R in 8 .. 1024 (cells along the longest side) or a tuple (R, band_cells) rebuilds every
    mesh from its inside on a voxel lattice, on the device, after keep_components and before smooth -- Blender's Voxel Remesh:
    overlapping parts fuse and the holes at the box close (TSR.extract_meshes; ops.mesh_voxel_remesh).
    `fill_holes` (default None): True (every border loop) or an int max_edges >= 3 caps the holes of every mesh -- the loops
    where the surface meets the box -- with fans, on the device, after keep_components and before voxel_remesh: Blender's
    Clean Up > Fill Holes (sides=).  Every existing vertex and face stays as it is.  A fan suits a short or roughly planar loop
    and nothing more: a long loop round a corner of the box gets a fan that cuts through the mesh, which `report` = "full"
    shows and `voxel_remesh` repairs (TSR.extract_meshes; ops.mesh_fill_holes).
    `report` (default None): True leaves what every final mesh is -- edge census, watertight, Euler number, genus, area, volume
    -- at `model.last_reports`, one dict per image, computed on the device before the hand-off; "full" adds the number of
    self-intersecting face pairs (TSR.extract_meshes; ops.mesh_report).  The meshes themselves do not change.
    `isosurface` (default "marching_cubes"): "surface_nets" extracts every mesh with surface nets on the device instead -- one
    vertex inside every cell the surface passes through, an all-quad mesh (Mesh.quads, which the plain Blender sink and
    Mesh.export's .obj receive) beside its triangles, no sliver triangles (TSR.extract_meshes; ops.surface_nets).
    `occlusion` (default None): True (64 directions), an int k in 1 .. 1024 or a tuple (k, max_distance) leaves the ambient
    occlusion of every final mesh against itself on the meshes in `last_meshes` (Mesh.vertex_occlusion, f32 [Nv], 1 = open:
    TSR.extract_meshes; ops.mesh_occlusion); Mesh.export writes it into .ply and .glb.  The Blender sinks take none.
    `normal_map` (default None): "tangent" or "object" adds a normal map baked from the density field to every mesh a texture
    is baked for (bake_texture_resolution > 0), at the texture's resolution and over its atlas (TSR.bake_normal_map): the
    surface detail that simplify removed, carried over to the low-poly mesh.  It is copied to the model (TSR.normal_map) before
    every generate_mesh; Mesh.export writes the map, and the textured Blender sink wires a tangent-space one to the material.
    `occlusion_map` (default None): True, an int k or a tuple (k, max_distance) adds an ambient-occlusion map to every mesh a
    texture is baked for, over the same atlas at the same resolution, baked against the mesh as it was before simplify
    (TSR.bake_occlusion_map; copied to the model as TSR.occlusion_map).  Mesh.export writes it (glTF occlusionTexture, `map_Ka`);
    the Blender sinks take none: the .glb carries it to Blender's own importer.
    `bake_project` (default None): True, an int n or a tuple (n, cells) (ops.project_rule) bakes the texture, and the normal map
    when `normal_map` is set, AT THE SURFACE: every texel is first projected from the low-poly face onto the field's
    iso-surface (TSR.bake_surface_maps; copied to the model as TSR.bake_project).
    `displacement_map` (default None): True, an int n or a tuple (n, cells) (ops.displacement_rule) bakes a displacement map --
    the height along the low-poly normal up to the field's iso-surface -- beside every baked texture, over its atlas
    (TSR.bake_displacement_map; copied to the model as TSR.displacement_map).  It comes back as the mesh's plain attribute
    `displacement`; Mesh.export(path, displacement=mesh.displacement) writes it.
    `thickness_map` (default None): True, an int k or a tuple (k, max_distance) (ops.thickness_rule) bakes a thickness map -- the
    wall thickness (shape diameter) of the mesh per texel -- beside every baked texture, over its atlas
    (TSR.bake_thickness_map; copied to the model as TSR.thickness_map).  It comes back as the mesh's plain attribute
    `thickness` (a tsr.thickness.ThicknessMap); its save(path) writes a 16-bit grey PNG.
    `curvature_map` (default None): True or an int r in 0 .. 8 (ops.curvature_rule: the rings the curvature is summed over) bakes a
    curvature map -- mean and Gaussian curvature of the mesh per texel -- beside every baked texture, over its atlas
    (TSR.bake_curvature_map; copied to the model as TSR.curvature_map).  It comes back as the mesh's plain attribute
    `curvature` (a tsr.curvature.CurvatureMap); its save(path) writes a 16-bit grey PNG.
    `atlas` (default "box"): "charts" unwraps every mesh a map is baked for with sf3d.unwrap.ChartUnwrapper -- charts that are
    connected pieces of surface -- instead of the box projection (copied to the model as TSR.atlas)."""

    def __init__(self, device):
        super().__init__(device, checkpoint_dir=ROOT_DIR + "/checkpoints/", chunk_size=8192, mc_resolution=256,
                         precision=os.environ.get("SCULPT_PRECISION", "bf16"))
        self.last_meshes = None  # headless callers read the result here (inside Blender it goes to the scene)
        self.bake_texture_resolution = 0
        self.vertex_normals = None
        self.keep_components = None
        self.simplify = None
        self.smooth = None
        self.project = None
        self.subdivide = None
        self.voxel_remesh = None
        self.fill_holes = None
        self.occlusion = None
        self.report = None
        self.isosurface = "marching_cubes"
        self.normal_map = None
        self.occlusion_map = None
        self.bake_project = None
        self.displacement_map = None
        self.thickness_map = None
        self.curvature_map = None
        self.atlas = "box"

    def _construct_model(self):
        model = TSR.from_pretrained(self.checkpoint_dir, config_name="config.yaml", weight_name="model.ckpt",
                                    precision=self.precision)
        model.renderer.set_chunk_size(self.chunk_size)
        return model.to(self.device)

    def generate_mesh(self, input_image, input_name=None, enable_texture=False):
        if self.model is None:
            return STATUS_NOT_LOADED
        try:
            with torch.no_grad():
                codes = self.model([input_image], device=self.device)
            self.model.normal_map = self.normal_map
            self.model.occlusion_map = self.occlusion_map
            self.model.bake_project = self.bake_project
            self.model.displacement_map = self.displacement_map
            self.model.thickness_map = self.thickness_map
            self.model.curvature_map = self.curvature_map
            self.model.atlas = self.atlas
            self.last_meshes = self.model.extract_mesh(codes, enable_texture=enable_texture, mesh_name=input_name,
                                                       resolution=self.mc_resolution,
                                                       bake_texture=int(self.bake_texture_resolution or 0),
                                                       normals=self.vertex_normals, isosurface=self.isosurface,
                                                       keep_components=self.keep_components, simplify=self.simplify,
                                                       smooth=self.smooth, project=self.project, subdivide=self.subdivide,
                                                       occlusion=self.occlusion, voxel_remesh=self.voxel_remesh,
                                                       report=self.report, fill_holes=self.fill_holes)
        except Exception as err:
            print(self.run_error_tag, err)
            return STATUS_FAILED
        return STATUS_OK

    def render_views(self, input_image, n_views=8, passes=None, **camera):
        """Turntable previews of what generate_mesh would build from `input_image`: a list of n_views PIL pictures, rendered
        from the scene code (TSR.render; camera: elevation_deg, camera_distance, fovy_deg, height, width).  With `passes` (any of
        "color", "opacity", "rgba", "depth", "normal": TSR.render_passes) a list of n_views dicts {pass: PIL picture} instead.
        Failures follow generate_mesh's convention: STATUS_NOT_LOADED without a model, STATUS_FAILED (message printed) when
        rendering fails."""
        if self.model is None:
            return STATUS_NOT_LOADED
        try:
            with torch.no_grad():
                codes = self.model([input_image], device=self.device)
            if passes is not None:
                return self.model.render_passes(codes, n_views=n_views, passes=passes, return_type="pil", **camera)[0]
            return self.model.render(codes, n_views=n_views, return_type="pil", **camera)[0]
        except Exception as err:
            print(self.run_error_tag, err)
            return STATUS_FAILED

    def render_mesh_views(self, mesh, n_views=8, passes=None, **camera):
        """Turntable previews of a finished mesh -- one of last_meshes, with whatever was baked onto it -- under render_views'
        cameras (TSR.render_mesh; camera: elevation_deg, camera_distance, fovy_deg, height, width, and ambient / light): a list
        of n_views PIL pictures of the "shaded" pass, or with `passes` a list of n_views dicts {pass: PIL picture}.  Failures
        follow render_views' convention: STATUS_NOT_LOADED without a model, STATUS_FAILED (message printed) when rendering fails."""
        if self.model is None:
            return STATUS_NOT_LOADED
        try:
            if passes is not None:
                return self.model.render_mesh(mesh, n_views=n_views, passes=passes, return_type="pil", **camera)
            views = self.model.render_mesh(mesh, n_views=n_views, passes=("shaded",), return_type="pil", **camera)
            return [v["shaded"] for v in views]
        except Exception as err:
            print(self.run_error_tag, err)
            return STATUS_FAILED
