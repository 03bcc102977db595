"""Mesh sink used inside Blender: the job of TSR.import_obj_blender
(/root/reference/TripoSR/tsr/system.py:127-168), with the per-loop Python colour loop
(system.py:143-146) replaced by one foreach_set.  Imported only when `bpy` is importable."""
import numpy as np


def import_obj_blender(verts, faces, vertex_colors=None, name="NewMesh"):
    import bpy

    mesh_data = bpy.data.meshes.new(name=name)
    mesh_data.from_pydata(verts.tolist(), [], faces.tolist())
    new_object = bpy.data.objects.new(name=name, object_data=mesh_data)
    bpy.context.collection.objects.link(new_object)
    if vertex_colors is None:
        return new_object
    if vertex_colors.shape[1] == 3:
        vertex_colors = np.hstack((vertex_colors, np.ones((vertex_colors.shape[0], 1), vertex_colors.dtype)))
    layer_name = "%s_VC" % name
    mesh_data.vertex_colors.new(name=layer_name)
    color_layer = mesh_data.vertex_colors[layer_name]
    loop_vert = np.empty(len(mesh_data.loops), np.int32)
    mesh_data.loops.foreach_get("vertex_index", loop_vert)
    color_layer.data.foreach_set("color", vertex_colors[loop_vert].astype(np.float32).ravel())
    mat = bpy.data.materials.new(name="VertexColorMaterial")
    mesh_data.materials.append(mat)
    mat.use_nodes = True
    nodes, links = mat.node_tree.nodes, mat.node_tree.links
    for node in list(nodes):
        nodes.remove(node)
    out_node = nodes.new(type="ShaderNodeOutputMaterial")
    bsdf = nodes.new(type="ShaderNodeBsdfPrincipled")
    vc = nodes.new(type="ShaderNodeVertexColor")
    vc.layer_name = layer_name
    links.new(vc.outputs["Color"], bsdf.inputs["Base Color"])
    links.new(bsdf.outputs["BSDF"], out_node.inputs["Surface"])
    bsdf.inputs["Roughness"].default_value = 1
    bsdf.inputs["IOR"].default_value = 1.00
    return new_object


def import_textured_blender(verts, faces, uvs, texture_image, name="NewMesh", normal_image=None):
    """The sink of a baked mesh (TSR.bake_texture): shared vertices, per-loop UVs (uvs f32 [3*Nf, 2] in face-corner order,
    origin bottom-left as Blender has it) and a material whose image texture feeds the Principled BSDF's Base Color;
    Roughness 1 and IOR 1.00 as the vertex-colour material above sets them.  Blender's UV layers are per loop, so nothing is
    un-indexed; the loop order must be faces.ravel() for uvs to land on the right corners, which is verified, not assumed.
    normal_image: a tangent-space normal map (Mesh.normal_map_image of TSR.bake_normal_map) -> a second image texture
    (colour space Non-Color) -> a Normal Map node -> the BSDF's Normal input; None (default): the node graph without them."""
    import bpy

    from ..sf3d.blender_sink import _image

    faces = np.asarray(faces)
    uvs = np.asarray(uvs, np.float32)
    if uvs.shape != (faces.size, 2):
        raise ValueError("import_textured_blender: uvs %s must be [3*Nf, 2] = [%d, 2]" % (uvs.shape, faces.size))
    mesh_data = bpy.data.meshes.new(name=name)
    mesh_data.from_pydata(np.asarray(verts).tolist(), [], faces.tolist())
    loop_vert = np.empty(len(mesh_data.loops), np.int32)
    mesh_data.loops.foreach_get("vertex_index", loop_vert)
    if loop_vert.size != faces.size or not np.array_equal(loop_vert, faces.reshape(-1)):
        raise RuntimeError("import_textured_blender: Blender's loops are not in face-corner order (%d loops for %d corners); "
                           "the UVs would land on the wrong corners" % (loop_vert.size, faces.size))
    new_object = bpy.data.objects.new(name=name, object_data=mesh_data)
    bpy.context.collection.objects.link(new_object)
    mesh_data.uv_layers.new(name="UVMap")
    mesh_data.uv_layers.active.data.foreach_set("uv", uvs.ravel())
    mat = bpy.data.materials.new(name="BakedTextureMaterial")
    mesh_data.materials.append(mat)
    mat.use_nodes = True
    nodes, links = mat.node_tree.nodes, mat.node_tree.links
    for node in list(nodes):
        nodes.remove(node)
    out_node = nodes.new(type="ShaderNodeOutputMaterial")
    bsdf = nodes.new(type="ShaderNodeBsdfPrincipled")
    tex = nodes.new(type="ShaderNodeTexImage")
    tex.image = _image(bpy, "%s_BaseColor" % name, texture_image.convert("RGBA"))
    links.new(tex.outputs["Color"], bsdf.inputs["Base Color"])
    links.new(bsdf.outputs["BSDF"], out_node.inputs["Surface"])
    bsdf.inputs["Roughness"].default_value = 1
    bsdf.inputs["IOR"].default_value = 1.00
    if normal_image is not None:
        nm_tex = nodes.new(type="ShaderNodeTexImage")
        nm_tex.image = _image(bpy, "%s_Normal" % name, normal_image.convert("RGBA"), non_color=True)
        nm = nodes.new(type="ShaderNodeNormalMap")
        links.new(nm_tex.outputs["Color"], nm.inputs["Color"])
        links.new(nm.outputs["Normal"], bsdf.inputs["Normal"])
    return new_object


def add_displacement_blender(obj, displacement, name=None):
    """A baked displacement map (tsr.displacement.DisplacementMap of TSR.bake_displacement_map) onto the first material of
    `obj`, an object one of the sinks above made with the map's atlas as its UV layer: a Non-Color image texture (the 16-bit
    picture as floats, code / 65535) -> a Displacement node with the map's midlevel and scale -> the material output's
    Displacement socket.  The material is set to displace ("BOTH": true displacement where the mesh is subdivided, bump
    elsewhere); nothing else of the node graph is touched.  -> the Displacement node."""
    import bpy

    name = name or obj.name
    materials = obj.data.materials
    if len(materials) == 0:
        raise ValueError("add_displacement_blender: the object has no material (import it with one of the sinks first)")
    mat = materials[0]
    code = np.flip(np.asarray(displacement.image(), np.float32) / np.float32(65535.0), axis=0)   # Blender's row 0 is the bottom
    res_y, res_x = code.shape
    img = bpy.data.images.new("%s_Displacement" % name, width=res_x, height=res_y)
    rgba = np.stack([code, code, code, np.ones_like(code)], axis=2)
    img.pixels.foreach_set(rgba.ravel())
    img.colorspace_settings.name = "Non-Color"
    nodes, links = mat.node_tree.nodes, mat.node_tree.links
    out_node = next((n for n in nodes if n.type in ("ShaderNodeOutputMaterial", "OUTPUT_MATERIAL")), None)
    if out_node is None:
        out_node = nodes.new(type="ShaderNodeOutputMaterial")
    tex = nodes.new(type="ShaderNodeTexImage")
    tex.image = img
    disp = nodes.new(type="ShaderNodeDisplacement")
    disp.inputs["Midlevel"].default_value = float(displacement.midlevel)
    disp.inputs["Scale"].default_value = float(displacement.scale)
    links.new(tex.outputs["Color"], disp.inputs["Height"])
    links.new(disp.outputs["Displacement"], out_node.inputs["Displacement"])
    mat.displacement_method = "BOTH"
    return disp
