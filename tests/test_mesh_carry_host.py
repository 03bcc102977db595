"""What every step that makes one Mesh from another keeps, re-indexes, replaces and drops -- for EVERY field a mesh can carry,
not only the ones the step is known to touch: a step that forgets a field fails here.  Host only: the device functions are
recorders, the model has no weights, the "device" is the CPU."""
import inspect

import numpy as np
import pytest
import torch

from sculptmate_amd import ops
from sculptmate_amd.tsr.spec import SMALL_CFG
from sculptmate_amd.tsr.system import TSR, Mesh, PendingMesh

FIELDS = ("vertex_colors", "vertex_normals", "vertex_occlusion", "uvs", "corner_normals", "corner_tangents", "texture", "normal_map",
          "normal_map_space", "occlusion_map", "occlusion_map_rule", "quads")
TENSORS = ("vertex_colors", "vertex_normals", "vertex_occlusion", "uvs", "corner_normals", "corner_tangents", "texture", "normal_map",
           "occlusion_map")

# how a field of the result relates to the input mesh; a field that a step does not list is None on its result
SAME, VI, CORNER, NEW, UVS, COPY = "the same object", "input[vi]", "input[corner]", "the new value", "own uvs, else new", "f32 copy"
_SURFACE = dict(vertex_colors=SAME, uvs=SAME, texture=SAME, quads=SAME)
CARRIES = {
    "keep_components": dict(vertex_colors=VI, vertex_normals=VI, vertex_occlusion=VI, uvs=CORNER, corner_normals=CORNER,
                            corner_tangents=CORNER, texture=SAME, normal_map=SAME, normal_map_space=SAME, occlusion_map=SAME,
                            occlusion_map_rule=SAME),
    "simplify": dict(vertex_colors=VI, vertex_normals=VI),
    "smooth": _SURFACE,
    "subdivide": dict(vertex_colors=NEW),
    "project_mesh": _SURFACE,
    "bake_texture": dict(uvs=NEW, texture=NEW),
    "bake_normal_map": dict(vertex_colors=SAME, texture=SAME, vertex_normals=SAME, vertex_occlusion=SAME, occlusion_map=SAME,
                            occlusion_map_rule=SAME, uvs=UVS, normal_map=NEW, normal_map_space=NEW, corner_normals=NEW,
                            corner_tangents=NEW),
    "bake_occlusion_map": dict(vertex_colors=SAME, texture=SAME, vertex_normals=SAME, vertex_occlusion=SAME, normal_map=SAME,
                               normal_map_space=SAME, corner_normals=SAME, corner_tangents=SAME, uvs=UVS, occlusion_map=NEW,
                               occlusion_map_rule=NEW),
    "render_mesh": dict(dict.fromkeys(TENSORS, COPY), normal_map_space=SAME),
    "result": dict(vertex_colors=NEW, vertex_normals=NEW),
}

RES = 4                       # below 150: the bakes do not reach ops.dilate_fill
FACE_INDEX = np.array([2, 0])         # reorders and drops
VERTEX_INDEX = np.array([3, 1, 0])    # not the identity
CORNER_INDEX = np.array([6, 7, 8, 0, 1, 2])


def _mesh(without=()):
    """4 vertices, 3 faces, every field a distinct value (but the fields in `without`)."""
    rng = np.random.default_rng(5)

    def f32(*shape):
        return rng.random(shape, dtype=np.float32)

    m = Mesh(f32(4, 3), np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1]]), f32(4, 3), uvs=f32(9, 2), texture=f32(RES, RES, 3),
             vertex_normals=f32(4, 3), vertex_occlusion=f32(4))
    m.corner_normals, m.corner_tangents = f32(9, 3), f32(9, 4)
    m.normal_map, m.normal_map_space = f32(RES, RES, 3), "tangent"
    m.occlusion_map, m.occlusion_map_rule = f32(RES, RES), (16, 0.5)
    m.quads = np.array([[0, 1, 2, 3]])
    for name in without:
        setattr(m, name, None)
    assert all((getattr(m, name) is None) == (name in without) for name in FIELDS)
    return m


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _is_value(got, want):
    if isinstance(want, (np.ndarray, torch.Tensor)):
        return got is want or (got is not None and _np(got).shape == _np(want).shape and np.array_equal(_np(got), _np(want)))
    return got == want


def _check(step, out, src, new=None):
    """Every one of the twelve fields of `out` is what CARRIES[step] says about it."""
    want = CARRIES[step]
    assert set(want) <= set(FIELDS)
    assert isinstance(out, Mesh)
    for name in FIELDS:
        got, had, rule = getattr(out, name), getattr(src, name), want.get(name)
        if rule == UVS:
            rule = SAME if had is not None else NEW
        if rule is None:
            assert got is None, (step, name)
        elif rule == SAME:
            assert got is had, (step, name)
        elif rule == VI:
            assert np.array_equal(got, had[VERTEX_INDEX]) and len(got) == len(VERTEX_INDEX), (step, name)
        elif rule == CORNER:
            assert np.array_equal(got, had[CORNER_INDEX]) and len(got) == len(CORNER_INDEX), (step, name)
        elif rule == NEW:
            assert _is_value(got, new[name]) and not _is_value(had, new[name]), (step, name)
        elif rule == COPY:
            if had is None:
                assert got is None, (step, name)
            else:
                assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.is_contiguous(), (step, name)
                assert _is_value(got, had), (step, name)
        else:
            raise AssertionError("unknown rule %r" % (rule,))


# ------------------------------------------------------------------------------------------------ the four Mesh methods
def test_keep_components(monkeypatch):
    src, v, f = _mesh(), np.zeros((3, 3), np.float32), np.array([[0, 1, 2], [0, 2, 1]])
    monkeypatch.setattr(ops, "mesh_keep_components", lambda vertices, faces, keep: (v, f, VERTEX_INDEX, FACE_INDEX))
    out = src.keep_components("largest")
    assert out.vertices is v and out.faces is f
    _check("keep_components", out, src)
    # the same through torch indices, as the device returns them
    monkeypatch.setattr(ops, "mesh_keep_components",
                        lambda vertices, faces, keep: (v, f, torch.from_numpy(VERTEX_INDEX), torch.from_numpy(FACE_INDEX)))
    tsrc = _mesh()
    for name in TENSORS:
        setattr(tsrc, name, torch.from_numpy(getattr(tsrc, name)))
    _check("keep_components", tsrc.keep_components("largest"), tsrc)
    # a mesh that carries nothing
    bare = Mesh(src.vertices, src.faces).keep_components("largest")
    assert all(getattr(bare, name) is None for name in FIELDS)


def test_simplify(monkeypatch):
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]])
    monkeypatch.setattr(ops, "mesh_simplify", lambda vertices, faces, rule: (v, f, VERTEX_INDEX))
    src = _mesh(without=("uvs", "texture"))
    out = src.simplify(0.5)
    assert out.vertices is v and out.faces is f
    _check("simplify", out, src)
    for baked in (_mesh(), _mesh(without=("uvs",)), _mesh(without=("texture",))):
        with pytest.raises(ValueError, match="Mesh.simplify: this mesh has a baked texture"):
            baked.simplify(0.5)
    with pytest.raises(ValueError) as rule_first:   # the rule is asked before the mesh is looked at
        _mesh().simplify("half")
    assert "baked texture" not in str(rule_first.value)


def test_smooth(monkeypatch):
    v = np.zeros((4, 3), np.float32)
    monkeypatch.setattr(ops, "mesh_smooth", lambda vertices, faces, rule: v)
    src = _mesh()
    out = src.smooth(3)
    assert out.vertices is v and out.faces is src.faces
    _check("smooth", out, src)


def test_subdivide(monkeypatch):
    v, f, colors = np.zeros((10, 3), np.float32), np.zeros((12, 3), np.int64), np.ones((10, 3), np.float32)
    seen = {}

    def subdivide(vertices, faces, rule, attributes=None):
        seen["attributes"] = attributes
        return v, f, colors

    monkeypatch.setattr(ops, "mesh_subdivide", subdivide)
    src = _mesh(without=("uvs", "texture"))
    out = src.subdivide(1)
    assert out.vertices is v and out.faces is f and seen["attributes"] is src.vertex_colors
    _check("subdivide", out, src, new=dict(vertex_colors=colors))
    for baked in (_mesh(), _mesh(without=("uvs",)), _mesh(without=("texture",))):
        with pytest.raises(ValueError, match="Mesh.subdivide: this mesh has a baked texture"):
            baked.subdivide(1)
    with pytest.raises(ValueError) as rule_first:
        _mesh().subdivide("twice")
    assert "baked texture" not in str(rule_first.value)


# ------------------------------------------------------------------------------------------ project_mesh and the bakes
class _Planes:
    """In place of ops.ChannelLastPlanes, whose constructor launches."""

    def __init__(self, planes):
        self.data = planes


@pytest.fixture
def model(monkeypatch):
    """A TSR without weights on the CPU "device": a stand-in decoder, and _atlas / _projected and the ops the bakes launch
    replaced by functions that return small CPU tensors -> (model, what those functions returned)."""
    m = TSR(SMALL_CFG)
    m.device, m.decoder = torch.device("cpu"), object()
    g = torch.Generator().manual_seed(7)
    made = dict(v=torch.rand((4, 3), generator=g), f=torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 1]]), uv=torch.rand((9, 2), generator=g),
                rast=object(), projected=torch.rand((4, 3), generator=g), vertex_normals=torch.rand((4, 3), generator=g),
                tangents=torch.rand((9, 4), generator=g), color=torch.rand((RES, RES, 3), generator=g),
                normal=torch.rand((RES, RES, 3), generator=g), ao=torch.rand((RES, RES), generator=g),
                mask=torch.ones((RES, RES), dtype=torch.bool))
    monkeypatch.setattr(m, "_atlas", lambda mesh, res, island_padding, unwrapper, keep_uvs=False: (
        made["v"], made["f"], mesh.uvs if keep_uvs and mesh.uvs is not None else made["uv"], made["rast"]))
    monkeypatch.setattr(m, "_projected", lambda v_pos, t_pos_idx, planes, threshold, project, resolution: made["projected"])
    monkeypatch.setattr(ops, "ChannelLastPlanes", _Planes)
    monkeypatch.setattr(ops, "vertex_normals", lambda v, f: made["vertex_normals"])
    monkeypatch.setattr(ops, "corner_tangents", lambda v, f, uv, n: made["tangents"])
    monkeypatch.setattr(ops, "bake_scene_color", lambda planes, mlp, v, f, rast, radius: (made["color"], made["mask"]))
    monkeypatch.setattr(ops, "bake_scene_normal", lambda planes, mlp, v, f, rast, radius, frame: (made["normal"], made["mask"]))
    monkeypatch.setattr(ops, "bake_occlusion_route", lambda: lambda v, f, n, rast, **kw: (made["ao"], made["mask"]))
    return m, made


CODE = torch.zeros((1, 3, 2, 2, 2))
# what a mesh that was never unwrapped lacks: the uvs and everything bound to them or to their atlas
_UNWRAPPED = ("uvs", "texture", "normal_map", "normal_map_space", "corner_normals", "corner_tangents", "occlusion_map", "occlusion_map_rule")


def test_project_mesh(model):
    m, made = model
    src = _mesh()
    out = m.project_mesh(src, CODE, resolution=8)
    assert out.vertices is made["projected"] and out.faces is src.faces
    _check("project_mesh", out, src)


def test_bake_texture(model):
    m, made = model
    for src in (_mesh(), _mesh(without=_UNWRAPPED)):
        out = m.bake_texture(src, CODE, texture_resolution=RES)
        assert out.vertices is src.vertices and out.faces is src.faces
        _check("bake_texture", out, src, new=dict(uvs=made["uv"], texture=made["color"]))
        assert out.uvs is made["uv"] and out.texture is made["color"]


@pytest.mark.parametrize("space", ["tangent", "object"])
def test_bake_normal_map(model, space):
    m, made = model
    new = dict(uvs=made["uv"], normal_map=0.5 + 0.5 * made["normal"], normal_map_space=space,
               corner_normals=(TSR.WINDING_OUTWARD * made["vertex_normals"])[made["f"].reshape(-1)], corner_tangents=made["tangents"])
    with_uvs = _mesh()
    with_uvs.normal_map_space = "tangent" if space == "object" else "object"   # the input's own tag is replaced, not carried
    for src in (with_uvs, _mesh(without=_UNWRAPPED)):
        out = m.bake_normal_map(src, CODE, resolution=RES, space=space)
        assert out.vertices is src.vertices and out.faces is src.faces
        _check("bake_normal_map", out, src, new=new)
        assert out.corner_tangents is made["tangents"]


def test_bake_occlusion_map(model):
    m, made = model
    new = dict(uvs=made["uv"], occlusion_map=made["ao"], occlusion_map_rule=ops.occlusion_rule((8, 0.25)))
    assert new["occlusion_map_rule"] != _mesh().occlusion_map_rule
    for src in (_mesh(), _mesh(without=_UNWRAPPED)):
        out = m.bake_occlusion_map(src, resolution=RES, occlusion=(8, 0.25))
        assert out.vertices is src.vertices and out.faces is src.faces
        _check("bake_occlusion_map", out, src, new=new)


class _Reached(Exception):
    pass


def test_the_resolution_default(model):
    """The texture's size, else for the occlusion map the normal map's, else 2048 -- seen by what _atlas is asked for."""
    m, made = model
    asked = []

    def atlas(mesh, res, island_padding, unwrapper, keep_uvs=False):
        asked.append(res)
        raise _Reached

    m._atlas = atlas
    sized = _mesh()
    sized.texture, sized.normal_map = np.zeros((6, 6, 3), np.float32), np.zeros((5, 5, 3), np.float32)
    for bake, args, src in ((m.bake_normal_map, (CODE,), sized), (m.bake_occlusion_map, (), sized),
                            (m.bake_normal_map, (CODE,), _mesh(without=("texture",))), (m.bake_occlusion_map, (), _mesh(without=("texture",))),
                            (m.bake_occlusion_map, (), _mesh(without=("texture", "normal_map"))),
                            (m.bake_normal_map, (CODE,), _mesh(without=("uvs",))), (m.bake_occlusion_map, (), _mesh(without=("uvs",)))):
        with pytest.raises(_Reached):
            bake(src, *args)
    assert asked == [6, 6, 2048, RES, 2048, 2048, 2048]
    with pytest.raises(ValueError, match="TSR.bake_normal_map: resolution must be positive"):
        m.bake_normal_map(sized, CODE, resolution=0)
    with pytest.raises(ValueError, match="TSR.bake_occlusion_map: resolution must be positive"):
        m.bake_occlusion_map(sized, resolution=0)


# --------------------------------------------------------------------------------- the device copy and the host hand-off
@pytest.mark.parametrize("without", [(), ("uvs", "texture", "vertex_occlusion")])
def test_render_mesh_copies_the_mesh_to_the_device(monkeypatch, without):
    m = TSR(SMALL_CFG)
    m.device = torch.device("cpu")
    seen = {}

    def render(self, rays_o, rays_d, **kw):
        seen["mesh"] = self
        return {"color": torch.zeros((2, 4, 4, 3))}

    monkeypatch.setattr(Mesh, "render", render)
    src = _mesh(without)
    m.render_mesh(src, 2, height=4, width=4)
    out = seen["mesh"]
    assert out is not src and out.vertices.dtype == torch.float32 and _is_value(out.vertices, src.vertices)
    assert isinstance(out.faces, torch.Tensor) and out.faces.is_contiguous() and _is_value(out.faces, src.faces)
    _check("render_mesh", out, src)


class _Event:
    def __init__(self):
        self.waited = 0

    def synchronize(self):
        self.waited += 1

    def query(self):
        return True


@pytest.mark.parametrize("bare", [False, True])
def test_pending_mesh_result(bare):
    v, f = torch.rand((4, 3)), torch.tensor([[0, 1, 2], [0, 2, 3]])
    c, n = (None, None) if bare else (torch.rand((4, 3)), torch.rand((4, 3)))
    event = _Event()
    pending = PendingMesh([v, f, c, n], event)
    out = pending.result()
    assert isinstance(out.vertices, np.ndarray) and np.shares_memory(out.vertices, v.numpy())
    assert isinstance(out.faces, np.ndarray) and np.shares_memory(out.faces, f.numpy())
    if bare:
        assert all(getattr(out, name) is None for name in FIELDS)
    else:
        _check("result", out, Mesh(None, None), new=dict(vertex_colors=c, vertex_normals=n))
        assert np.shares_memory(out.vertex_colors, c.numpy()) and np.shares_memory(out.vertex_normals, n.numpy())
    assert pending.result() is out and event.waited == 1 and pending.done()


# ------------------------------------------------------------------------------------------------- the record itself
def test_the_constructor_and_the_declared_fields():
    assert list(inspect.signature(Mesh.__init__).parameters) == ["self", "vertices", "faces", "vertex_colors", "uvs", "texture",
                                                                 "vertex_normals", "vertex_occlusion"]
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]])
    m = Mesh(v, f)
    assert m.vertices is v and m.faces is f and all(name in vars(m) and getattr(m, name) is None for name in FIELDS)
    uvs = np.zeros((3, 2), np.float32)
    m = type(m)(v, f, None, uvs=uvs)
    assert m.uvs is uvs and m.vertex_colors is None
    m.occlusion_map = "assigned later"
    assert m.occlusion_map == "assigned later"
    assert Mesh.__new__(Mesh).quads is None   # an object made without __init__


def test_the_declaration_is_the_twelve_fields():
    from sculptmate_amd.tsr import mesh

    assert sorted(mesh.FIELDS) == sorted(FIELDS) and len(set(mesh.FIELDS)) == 12
    assert sorted(mesh.TENSOR_FIELDS) == sorted(TENSORS)
    assert mesh.VERTEX_FIELDS == ("vertex_colors", "vertex_normals", "vertex_occlusion")
    assert mesh.CORNER_FIELDS == ("uvs", "corner_normals", "corner_tangents")
    assert mesh.ATLAS_FIELDS == ("texture", "normal_map", "occlusion_map")
    assert mesh.MAP_TAGS == {"normal_map": "normal_map_space", "occlusion_map": "occlusion_map_rule"}
    assert mesh.Mesh is Mesh and mesh.PendingMesh is PendingMesh


def test_the_carry_helper_refuses_an_undeclared_field():
    src = _mesh()
    v, f = src.vertices, src.faces
    with pytest.raises(ValueError, match="vertex_colours"):
        src._derive(v, f, ("vertex_colours",))
    with pytest.raises(ValueError, match="texure"):
        src._derive(v, f, ("uvs",), texure=src.texture)
    with pytest.raises(ValueError, match="vertices"):   # vertices and faces are arguments, not carried fields
        src._derive(v, f, ("vertices",))
    # a tag travels with its map; what is not named is None
    out = src._derive(v, f, ("normal_map", "occlusion_map"))
    assert out.normal_map is src.normal_map and out.normal_map_space == "tangent"
    assert out.occlusion_map is src.occlusion_map and out.occlusion_map_rule == (16, 0.5)
    assert all(getattr(out, name) is None for name in FIELDS if "map" not in name)
    # the indices re-index what is bound to them and nothing else
    out = src._derive(v, f, [name for name in FIELDS if name != "quads"], vertex_index=VERTEX_INDEX, face_index=FACE_INDEX)
    _check("keep_components", out, src)
    assert src._derive(v, f, ("quads",), vertex_index=VERTEX_INDEX, face_index=FACE_INDEX).quads is src.quads
