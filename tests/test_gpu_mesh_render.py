"""The mesh render on the device (csrc/mesh_ray.hip sculpt_surface_render; ops.mesh_render, Mesh.render, TSR.render_mesh): the
fused kernel against the composed route and the NumPy restatement (tests/_meshrenderref.py), bit for bit, in every pass."""
import numpy as np
import pytest
import torch

import _meshrenderref as MR
import _rayref as RR
import _tsrmodel
from sculptmate_amd import ops
from test_gpu_bake_occlusion import _same, _self_mesh

pytestmark = pytest.mark.gpu

ALL = tuple(MR.PASSES)
MATERIALS = ["none", "colors", "normals_occlusion", "texture", "texture_object", "texture_tangent_ao"]


def _dev(cuda, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def camera(P, F, n_images, H, W, spread=0.8):
    """Pinhole rays [n_images, H, W, 3] aimed at the mesh from 3 radii away, the picture 0.8 wide in the tangent of the view
    angle: the mesh's bounding sphere (0.35) and the one of its bounds (0.71 at most) stay inside, so the rim of the picture
    misses the mesh and, at 64 x 64, the corner tiles miss the grid's bounds.  Direction lengths are not 1."""
    used = np.asarray(P, np.float64)[np.unique(F)]
    centre = 0.5 * (used.min(0) + used.max(0))
    r = float(np.linalg.norm(used - centre, axis=1).max())
    O, D = [], []
    for k in range(n_images):
        back = np.array([0.3 + 0.5 * k, 0.2 - 0.4 * k, 1.0])
        back /= np.linalg.norm(back)
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        ys, xs = np.meshgrid((np.arange(H) + 0.5) / H * 2 - 1, (np.arange(W) + 0.5) / W * 2 - 1, indexing="ij")
        d = -back[None, None] + spread * (xs[..., None] * right + -ys[..., None] * up)
        O.append(np.broadcast_to(centre + 3.0 * r * back, (H, W, 3)))
        D.append(d * (1.0 + 0.25 * k))
    return np.stack(O).astype(np.float32), np.stack(D).astype(np.float32)


_meshes = {}


def _mesh(cuda, name):
    """The mesh with every attribute a material may draw on, host and device, computed once and shared, never modified.  The
    atlas is ops.uv_cell_atlas', the frame the one TSR.bake_normal_map builds; the maps are random, of sides 16, 3 and 1."""
    if name not in _meshes:
        P, F = _self_mesh(name)
        rng = np.random.default_rng(len(_meshes) + 3)
        v, f = _dev(cuda, P), _dev(cuda, F.astype(np.int64))
        uv, _ = ops.uv_cell_atlas(v, f)
        vn = ops.vertex_normals(v, f).contiguous()
        cn = vn[f.reshape(-1)].contiguous()
        ct = ops.corner_tangents(v, f, uv, cn)
        nv = len(P)
        host = dict(uvs=uv.cpu().numpy(), corner_normals=cn.cpu().numpy(), corner_tangents=ct.cpu().numpy(),
                    vertex_normals=(vn.cpu().numpy() * rng.uniform(0.5, 2.0, (nv, 1))).astype(np.float32),     # not unit: the rule normalises
                    vertex_colors=rng.uniform(0, 1, (nv, 4)).astype(np.float32),
                    vertex_occlusion=rng.uniform(0, 1, nv).astype(np.float32))
        for side in (1, 3, 16):
            host["rgb%d" % side] = rng.uniform(0, 1, (side, side, 3)).astype(np.float32)
            host["grey%d" % side] = rng.uniform(0, 1, (side, side)).astype(np.float32)
        _meshes[name] = (P, F, host, {k: _dev(cuda, a) for k, a in host.items()})
    return _meshes[name]


def _material(a, which):
    """The keyword arguments of one material combination from the arrays `a` (host or device)."""
    if which == "none":
        return {}
    if which == "colors":
        return dict(vertex_colors=a["vertex_colors"])
    if which == "normals_occlusion":
        return dict(vertex_normals=a["vertex_normals"], vertex_occlusion=a["vertex_occlusion"], vertex_colors=a["vertex_colors"][:, :3])
    if which == "texture":
        return dict(uvs=a["uvs"], texture=a["rgb3"], vertex_colors=a["vertex_colors"])      # the texture comes first
    if which == "texture_object":
        return dict(uvs=a["uvs"], texture=a["rgb1"], normal_map=a["rgb16"], normal_map_space="object", vertex_normals=a["vertex_normals"])
    return dict(uvs=a["uvs"], texture=a["rgb16"], normal_map=a["rgb3"], normal_map_space="tangent", corner_normals=a["corner_normals"],
                corner_tangents=a["corner_tangents"], occlusion_map=a["grey16"])


def _all_equal(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for p in want:
        _same(got[p], want[p], "%s, pass %s" % (what, p))


# ------------------------------------------------------------------------------------------------------------ the three routes
_casts = {}


def _rays(name):
    """The ray set of tests/_rayref.py for the mesh (aimed, random, from inside, AT vertices and edge midpoints, along edges and
    cell borders, in the planes of faces, zero directions, NaN and inf) and its brute-force hits, shared by the materials."""
    if name not in _casts:
        P, F = _self_mesh(name)
        O, D, parts = RR.ray_set(P, F, seed=23 + len(_casts), n_aimed=300, n_random=100, n_inside=60, n_axis=60, n_plane=30, n_scaled=30)
        _casts[name] = (O, D, parts, RR.ray_cast(O, D, P, F, want_ties=True))
    return _casts[name]


def test_the_ray_sets_hold_what_they_are_meant_to():
    """On the reference alone: hits, misses, ties (coincident faces, rays through edges and vertices) and the odd rays."""
    for name in ("icosphere", "cube", "doubled_cube"):
        O, D, parts, (t, face, uv, ties) = _rays(name)
        assert 0.2 < (face >= 0).mean() < 0.95 and np.isnan(t[parts["odd"]]).sum() == 4 and (face[parts["odd"]] == -1).all()
        assert (ties[parts["targets"]] > 1).any()
    assert (_rays("doubled_cube")[3][3][_rays("doubled_cube")[3][1] >= 0] >= 2).all()
    assert (_rays("doubled_cube")[3][1] < 12).all()       # the lower index of two coincident faces


@pytest.mark.parametrize("face_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("name", ["icosphere", "cube", "doubled_cube"])
def test_fused_equals_composed_equals_the_restatement(cuda, name, face_dtype):
    P, F, host, dev = _mesh(cuda, name)
    O, D, parts, cast = _rays(name)
    o, d, v = _dev(cuda, O), _dev(cuda, D), _dev(cuda, P)
    f = _dev(cuda, F.astype(np.int64)).to(face_dtype)
    for which in MATERIALS:
        kw = dict(ambient=0.25, outward=-1.0) if which == "colors" else {}
        if which == "texture":
            kw = dict(light=(1.0, -2.0, 0.5))
        got = ops.mesh_render(o, d, v, f, passes=ALL, **_material(dev, which), **kw)
        for p, (shape, dtype, _) in MR.PASSES.items():
            assert got[p].shape == (len(O),) + shape and got[p].dtype == (torch.int32 if p == "face" else torch.float32)
        _all_equal(got, ops.mesh_render_composed(o, d, v, f, passes=ALL, **_material(dev, which), **kw), "%s/%s fused vs composed" % (name, which))
        if face_dtype == torch.int32:
            want = MR.render(O, D, P, F, ALL, cast=cast[:3], **_material(host, which), **kw)
            _all_equal(got, want, "%s/%s fused vs restatement" % (name, which))
    assert np.array_equal(got["face"].cpu().numpy(), cast[1])
    hit = got["face"] >= 0
    assert bool((got["opacity"][hit] == 1).all()) and bool((got["opacity"][~hit] == 0).all())
    assert bool(torch.isnan(got["depth"][parts["odd"]]).sum() == 4)


def test_only_the_passes_asked_for_come_back_and_each_alone_is_the_same(cuda):
    P, F, host, dev = _mesh(cuda, "icosphere")
    o, d = (_dev(cuda, x) for x in camera(P, F, 1, 19, 23))
    v, f = _dev(cuda, P), _dev(cuda, F)
    full = ops.mesh_render(o, d, v, f, passes=ALL, **_material(dev, "texture_tangent_ao"))
    for p in ALL:
        one = ops.mesh_render(o, d, v, f, passes=p, **_material(dev, "texture_tangent_ao"))
        assert list(one) == [p]
        _same(one[p], full[p], "pass %s alone" % p)
    two = ops.mesh_render(o, d, v, f, passes=("face", "shaded", "face"), **_material(dev, "texture_tangent_ao"))
    assert list(two) == ["face", "shaded"]


# ------------------------------------------------------------------------------------------------------------ image sizes
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (8, 8), (19, 23), (64, 64)])
def test_image_sizes(cuda, H, W):
    P, F, host, dev = _mesh(cuda, "icosphere")
    n_images = 1 if H == 64 else 3
    O, D = camera(P, F, n_images, H, W)
    o, d, v, f = _dev(cuda, O), _dev(cuda, D), _dev(cuda, P), _dev(cuda, F)
    got = ops.mesh_render(o, d, v, f, passes=ALL, **_material(dev, "texture_tangent_ao"))
    for p, (shape, _, _) in MR.PASSES.items():
        assert got[p].shape == (n_images, H, W) + shape
    _all_equal(got, ops.mesh_render_composed(o, d, v, f, passes=ALL, **_material(dev, "texture_tangent_ao")), "%dx%d fused vs composed" % (H, W))
    _all_equal(got, MR.render(O, D, P, F, ALL, **_material(host, "texture_tangent_ao")), "%dx%d fused vs restatement" % (H, W))
    face = got["face"].cpu().numpy()
    if H * W > 1:
        assert (face >= 0).any() and (face < 0).any()
    else:
        assert (face >= 0).all()                 # the one pixel looks at the centre
    if H == 64:
        # whole tiles of hits in the middle, and the four corner tiles miss the grid's bounds: every ray of theirs passes the
        # bounds of the mesh at more than a hundredth of its size
        assert (face[0, 24:40, 24:40] >= 0).all()
        used = P[np.unique(F)].astype(np.float64)
        lo, hi = used.min(0) - 0.01, used.max(0) + 0.01
        for ys in (slice(0, 8), slice(56, 64)):
            for xs in (slice(0, 8), slice(56, 64)):
                oo, dd = O[0, ys, xs].reshape(-1, 3).astype(np.float64), D[0, ys, xs].reshape(-1, 3).astype(np.float64)
                with np.errstate(all="ignore"):
                    ta, tb = (lo - oo) / dd, (hi - oo) / dd
                assert (np.minimum(ta, tb).max(1) > np.maximum(ta, tb).min(1)).all()
                assert (face[0, ys, xs] == -1).all()


# ------------------------------------------------------------------------------------------------------------ per-ray values
def test_a_rays_value_depends_on_the_ray_alone(cuda):
    P, F, host, dev = _mesh(cuda, "icosphere")
    O, D = camera(P, F, 2, 19, 23)
    v, f = _dev(cuda, P), _dev(cuda, F)
    mat = _material(dev, "texture_tangent_ao")
    image = ops.mesh_render(_dev(cuda, O), _dev(cuda, D), v, f, passes=ALL, **mat)
    rows = ops.mesh_render(_dev(cuda, O.reshape(-1, 3)), _dev(cuda, D.reshape(-1, 3)), v, f, passes=ALL, **mat)
    flipped = ops.mesh_render(_dev(cuda, O[:, ::-1]), _dev(cuda, D[:, ::-1]), v, f, passes=ALL, **mat)
    n = O.size // 3
    rolled = ops.mesh_render(_dev(cuda, np.roll(O.reshape(-1, 3), 7, 0).reshape(O.shape)), _dev(cuda, np.roll(D.reshape(-1, 3), 7, 0).reshape(D.shape)),
                             v, f, passes=ALL, **mat)
    for p, (shape, _, _) in MR.PASSES.items():
        _same(rows[p].reshape(image[p].shape), image[p], "%s: [N, 3] vs image" % p)
        _same(flipped[p].flip(1), image[p], "%s: rows reversed" % p)
        _same(rolled[p].reshape((n,) + shape).roll(-7, 0).reshape(image[p].shape), image[p], "%s: rolled by 7" % p)


def test_bad_rays_get_the_background_and_leave_their_neighbours_alone(cuda):
    P, F, host, dev = _mesh(cuda, "icosphere")
    O, D = camera(P, F, 1, 16, 16, spread=0.2)                   # every ray of the clean picture hits
    v, f = _dev(cuda, P), _dev(cuda, F)
    mat = _material(dev, "texture_tangent_ao")
    clean = ops.mesh_render(_dev(cuda, O), _dev(cuda, D), v, f, passes=ALL, **mat)
    assert bool((clean["face"] >= 0).all())
    O2, D2 = O.copy(), D.copy()
    nonfinite = [(1, 2), (3, 11), (6, 6), (9, 1), (12, 14), (15, 15)]
    O2[0, 1, 2, 0] = np.nan
    D2[0, 3, 11, 2] = np.nan
    O2[0, 6, 6, 1] = np.inf
    D2[0, 9, 1, 0] = -np.inf
    D2[0, 12, 14] = np.nan
    O2[0, 15, 15] = np.inf
    zero = [(0, 0), (7, 8), (8, 7)]
    D2[0, 0, 0] = 0.0
    D2[0, 7, 8] = (0.0, -0.0, 0.0)
    D2[0, 8, 7] = 0.0
    got = ops.mesh_render(_dev(cuda, O2), _dev(cuda, D2), v, f, passes=ALL, **mat)
    _all_equal(got, ops.mesh_render_composed(_dev(cuda, O2), _dev(cuda, D2), v, f, passes=ALL, **mat), "bad rays, fused vs composed")
    _all_equal(got, MR.render(O2, D2, P, F, ALL, **_material(host, "texture_tangent_ao")), "bad rays, fused vs restatement")
    bad = np.zeros((16, 16), bool)
    for y, x in nonfinite + zero:
        bad[y, x] = True
        for p, (shape, _, bg) in MR.PASSES.items():
            value = got[p][0, y, x].cpu().numpy()
            if p == "depth" and (y, x) in nonfinite:
                assert np.isnan(value), (p, y, x)
            else:
                assert (value == bg).all(), (p, y, x, value)
    keep = torch.from_numpy(~bad).to(cuda)
    for p in ALL:
        _same(got[p][0][keep], clean[p][0][keep], "%s: the neighbours" % p)


def test_uvs_on_zero_and_one_and_maps_of_side_one(cuda):
    P, F = _self_mesh("cube")
    nf = len(F)
    rng = np.random.default_rng(9)
    uvs = np.tile(np.array([[0, 1], [1, 1], [0, 0]], np.float32), (nf, 1))     # every corner on the rim of the atlas
    # at every vertex from three sides, at edge midpoints and at face centres: U and V are 0, 1 and in between
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    targets = np.concatenate([P, np.float32(0.5) * (P[e[:, 0]] + P[e[:, 1]]), (P[F[:, 0]] + P[F[:, 1]] + P[F[:, 2]]) / np.float32(3)])
    O = np.concatenate([targets + (targets - np.float32(0.5)) * np.float32(4), targets + np.float32([0, 0, 3]),
                        targets - np.float32([0, 3, 0]), targets + np.float32([3, 0, 0])]).astype(np.float32)
    D = (np.concatenate([targets] * 4) - O).astype(np.float32)
    v, f, o, d = _dev(cuda, P), _dev(cuda, F), _dev(cuda, O), _dev(cuda, D)
    for side in (1, 2, 16):
        host = dict(uvs=uvs, texture=rng.uniform(0, 1, (side, side, 3)).astype(np.float32),
                    normal_map=rng.uniform(0, 1, (side, side, 3)).astype(np.float32), normal_map_space="object",
                    occlusion_map=rng.uniform(0, 1, (side, side)).astype(np.float32))
        dev = {k: (a if isinstance(a, str) else _dev(cuda, a)) for k, a in host.items()}
        got = ops.mesh_render(o, d, v, f, passes=ALL, **dev)
        _all_equal(got, ops.mesh_render_composed(o, d, v, f, passes=ALL, **dev), "side %d fused vs composed" % side)
        _all_equal(got, MR.render(O, D, P, F, ALL, **host), "side %d fused vs restatement" % side)
        if side == 1:
            hit = got["face"] >= 0
            assert int(hit.sum()) > 50
            # a map of side 1 is its one texel T wherever it is read, up to the roundings of the blend of T with itself: six
            # operations on values of at most T, and (1 - fx) + fx is 1 within one rounding -- 8 x 2^-24 T covers them
            for value, texel in ((got["color"][hit], dev["texture"][0, 0]), (got["occlusion"][hit], dev["occlusion_map"][0, 0])):
                assert bool(((value - texel).abs() <= 8 * 2.0 ** -24 * texel).all())
            assert bool((got["color"][hit] == dev["texture"][0, 0]).all(-1).any())       # and exactly T where the fractions are 0
    t, face, uv = RR.ray_cast(O, D, P, F)
    w1, w2 = uv[face >= 0, 0], uv[face >= 0, 1]
    U = MR.interp(np.float32(0), np.float32(1), np.float32(0), (np.float32(1) - w1) - w2, w1, w2)
    V = MR.interp(np.float32(1), np.float32(1), np.float32(0), (np.float32(1) - w1) - w2, w1, w2)
    seen = {(float(a), float(b)) for a, b in zip(U, V) if a in (0, 1) and b in (0, 1)}
    assert len(seen) >= 3, seen            # corners of the atlas themselves were looked up


def test_a_mesh_without_faces_and_no_rays(cuda):
    P, F, host, dev = _mesh(cuda, "icosphere")
    O, D = camera(P, F, 2, 5, 7)
    D[1, 2, 3] = np.nan
    v, o, d = _dev(cuda, P), _dev(cuda, O), _dev(cuda, D)
    none = _dev(cuda, F[:0])
    for fn in (ops.mesh_render, ops.mesh_render_composed):
        got = fn(o, d, v, none, passes=ALL, vertex_colors=dev["vertex_colors"])
        for p, (shape, _, bg) in MR.PASSES.items():
            value = got[p].cpu().numpy()
            assert value.shape == (2, 5, 7) + shape
            if p == "depth":
                assert np.isnan(value[1, 2, 3]) and np.isnan(value).sum() == 1 and (value[~np.isnan(value)] == 0).all()
            else:
                assert (value == bg).all(), p
        empty = fn(o[:0], d[:0], v, _dev(cuda, F), passes=ALL)
        assert all(empty[p].shape == (0, 5, 7) + MR.PASSES[p][0] for p in ALL)
        flat = fn(o.reshape(-1, 3)[:0], d.reshape(-1, 3)[:0], v, _dev(cuda, F), passes=("rgba",))
        assert flat["rgba"].shape == (0, 4)
    with pytest.raises(ops.SculptError, match="shape"):
        ops.mesh_render(o, d, v, _dev(cuda, F), uvs=dev["uvs"][:-1], texture=dev["rgb3"])
    with pytest.raises(ops.SculptError, match="shape"):
        ops.mesh_render(o, d, v, _dev(cuda, F), vertex_normals=dev["vertex_normals"][1:])


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model(cuda):
    out = _tsrmodel.small_model(cuda, 32, enable_texture=True)
    m = out["m"]
    low = m.extract_meshes(out["codes"], enable_texture=True, resolution=32, threshold=out["threshold"], bake_texture=64,
                           keep_components="largest", simplify=0.5)[0]
    low = m.bake_normal_map(low, out["codes"][0])
    out["low"] = m.bake_occlusion_map(low, occlusion=8)
    return out


def test_render_mesh_end_to_end(model, monkeypatch):
    from sculptmate_amd.tsr.cameras import get_spherical_cameras

    m, low = model["m"], model["low"]
    assert low.texture is not None and low.normal_map_space == "tangent" and low.occlusion_map is not None
    views = m.render_mesh(low, n_views=2, height=32, width=32, passes=ALL)
    assert len(views) == 2 and all(list(v) == list(ALL) for v in views)
    for view in views:
        for p, (shape, _, _) in MR.PASSES.items():
            assert view[p].shape == (32, 32) + shape and view[p].is_cuda and view[p].dtype == (torch.int32 if p == "face" else torch.float32)
    rays_o, rays_d = get_spherical_cameras(2, 0.0, 1.9, 40.0, 32, 32)
    rays_o, rays_d = rays_o.to(low.vertices.device), rays_d.to(low.vertices.device)
    t, face, _ = low.ray_cast(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3))
    got_face = torch.stack([v["face"] for v in views])
    assert torch.equal(got_face.reshape(-1).long(), face)
    hit = got_face >= 0
    print("hit pixels: %d of %d" % (int(hit.sum()), hit.numel()))
    assert int(hit.sum()) > 50            # under render's default cameras the model's box fills the picture
    _same(torch.stack([v["depth"] for v in views]).reshape(-1)[hit.reshape(-1)], t.float()[hit.reshape(-1)], "depth vs Mesh.ray_cast")
    by_hand = ops.mesh_render(rays_o, rays_d, low.vertices, low.faces, passes=("color", "normal", "shaded"), uvs=low.uvs, texture=low.texture,
                              normal_map=low.normal_map, normal_map_space="tangent", corner_normals=low.corner_normals,
                              corner_tangents=low.corner_tangents, occlusion_map=low.occlusion_map, outward=m.WINDING_OUTWARD)
    for p in ("color", "normal", "shaded"):
        _same(torch.stack([v[p] for v in views])[hit], by_hand[p][hit], "%s vs ops.mesh_render by hand" % p)
    colour = torch.stack([v["color"] for v in views])
    assert float(colour[hit].min()) >= 0.0 and float(colour[hit].max()) <= 1.0 + 1e-6
    # from further away with a wider lens the rim of the picture is background
    far = m.render_mesh(low, n_views=2, camera_distance=3.5, fovy_deg=60.0, height=32, width=32, passes=("color", "face", "depth"))
    off = torch.stack([v["face"] for v in far]) < 0
    assert 0 < int(off.sum()) < off.numel()
    assert bool((torch.stack([v["color"] for v in far])[off] == 1).all()) and bool((torch.stack([v["depth"] for v in far])[off] == 0).all())
    length = torch.stack([v["normal"] for v in views])[hit].norm(dim=-1)
    assert float((length - 1).abs().max()) < 1e-5
    # Mesh.render is the same call, and both routes give the same pictures
    direct = low.render(rays_o, rays_d, passes=("rgba",), outward=m.WINDING_OUTWARD)["rgba"]
    _same(direct, torch.stack([v["rgba"] for v in views]), "Mesh.render")
    other = "composedrender" if ops.mesh_render_route() is ops.mesh_render else "fusedrender"
    monkeypatch.setenv("SCULPT_DISTANCE_FORM", other)
    assert ops.mesh_render_route() is (ops.mesh_render_composed if other == "composedrender" else ops.mesh_render)
    again = m.render_mesh(low, n_views=2, height=32, width=32, passes=ALL)
    monkeypatch.delenv("SCULPT_DISTANCE_FORM")
    for a, b in zip(again, views):
        _all_equal(a, b, "the other route")
    # the conversions
    host = m.render_mesh(low, n_views=2, height=32, width=32, passes=ALL, return_type="np")
    for a, b in zip(host, views):
        assert all(isinstance(a[p], np.ndarray) for p in ALL)
        _all_equal(a, {p: b[p].cpu().numpy() for p in ALL}, "np")
    pil = m.render_mesh(low, n_views=2, height=32, width=32, passes=ALL, return_type="pil")
    modes = {"color": "RGB", "shaded": "RGB", "opacity": "L", "rgba": "RGBA", "depth": "F", "normal": "RGB", "occlusion": "L", "face": "I"}
    for view in pil:
        assert {p: view[p].mode for p in ALL} == modes and all(view[p].size == (32, 32) for p in ALL)
    assert np.array_equal(np.asarray(pil[0]["face"]), host[0]["face"])
    assert np.array_equal(np.asarray(pil[0]["color"]), (host[0]["color"] * 255.0).astype(np.uint8))


def test_generator_render_mesh_views(model):
    from sculptmate_amd._facade import STATUS_FAILED
    from sculptmate_amd.generate import TripoGenerator

    g = TripoGenerator(model["low"].vertices.device)
    g.model = model["m"]
    shaded = g.render_mesh_views(model["low"], n_views=2, height=16, width=16)
    assert len(shaded) == 2 and all(im.mode == "RGB" and im.size == (16, 16) for im in shaded)
    views = g.render_mesh_views(model["low"], n_views=2, passes=("depth", "face"), height=16, width=16)
    assert len(views) == 2 and list(views[0]) == ["depth", "face"]
    assert g.render_mesh_views(model["low"], n_views=2, passes=("nope",)) == STATUS_FAILED
