"""Triangle remeshing on the device (sf3d/remesh_device.py, csrc/remesh_device.hip): the invariants tests/test_remesh.py asserts
for the host remesher, with the same thresholds, on the device path; determinism; agreement in kind with the host remesher on a
large marching-cubes mesh; the split capacity protocol when its first guess is too small; refused input; the SF3D facade with
`device_remesher` as its remesher."""
import numpy as np
import pytest
import torch

from sculptmate_amd import _lib
from sculptmate_amd.sf3d import remesh as rm
from sculptmate_amd.sf3d import remesh_device as rd
from test_remesh import edge_lengths, icosahedron, icosphere, open_sheet, signed_volume, topology, torus, torus_distance

pytestmark = pytest.mark.gpu


def dev(v, f):
    return torch.from_numpy(np.asarray(v, np.float32)).cuda(), torch.from_numpy(np.asarray(f, np.int32)).cuda()


def host(v, f):
    return v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int32)


def decimate(v, f, **kw):
    vo, fo, _, _ = rd.decimate_device(*dev(v, f), **kw)
    return host(vo, fo)


def remesh(v, f, i, h, project=True):
    return host(*rd.remesh_botsch_device(*dev(v, f), i, h, project))


def boundary_vertices(f):
    d = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0), 1)
    e, cnt = np.unique(d, axis=0, return_counts=True)
    return np.unique(e[cnt == 1])


# -------------------------------------------------------------------------------- the host's thresholds on the device path
def test_subdivide_device_is_the_host_subdivision(cuda):
    v, f = icosahedron()
    v = v.astype(np.float32).astype(np.float64)  # what the device holds
    hv, hf = rm.subdivide(v, f, 1)
    dv, df = rd.subdivide_device(*dev(v, f), iters=1)
    assert np.array_equal(df.cpu().numpy(), hf)  # same numbering, same template
    assert np.array_equal(dv.cpu().numpy(), hv.astype(np.float32))  # fp32 midpoints = the fp64 ones rounded once
    hv, hf = rm.subdivide(v, f, 3)
    dv, df = rd.subdivide_device(*dev(v, f), iters=3)
    assert np.array_equal(df.cpu().numpy(), hf) and np.allclose(dv.cpu().numpy(), hv, atol=1e-6)
    chi, nb = topology(*host(dv, df))
    assert chi == 2 and nb == 0
    dv, df = rd.subdivide_device(*dev(v, f), iters=0)
    assert np.array_equal(df.cpu().numpy(), f)


@pytest.mark.parametrize("ratio", [0.5, 0.1, 0.02])
def test_decimate_sphere_meets_budget_and_stays_a_sphere(cuda, ratio):
    v, f = icosphere(4)
    vo, fo = decimate(v, f, face_ratio=ratio)
    target = int(np.floor(ratio * len(f)))
    assert target - 1 <= len(fo) <= target
    chi, nb = topology(vo, fo)
    assert chi == 2 and nb == 0
    assert signed_volume(vo, fo) > 0
    rad = np.linalg.norm(vo, axis=1)
    assert rad.max() <= 1 + 1e-6 and rad.min() > (0.55 if ratio < 0.05 else 0.8)  # (fp32 positions: 1e-6, not 1e-12)
    el = edge_lengths(vo, fo)
    assert el.max() / el.min() < 6


def test_decimate_keeps_genus_and_boundary(cuda):
    v, f = torus(48, 24)
    vo, fo = decimate(v, f, face_ratio=0.25)
    chi, nb = topology(vo, fo)
    assert chi == 0 and nb == 0 and len(fo) <= len(f) // 4
    assert torus_distance(vo).max() < 0.08
    v, f = open_sheet(33)
    chi0, nb0 = topology(v, f)
    vo, fo = decimate(v, f, face_ratio=0.2)
    chi, nb = topology(vo, fo)
    assert chi == chi0 == 1 and 0 < nb < nb0 and len(fo) <= int(0.2 * len(f))
    assert vo[:, :2].min() >= -1e-6 and vo[:, :2].max() <= 1 + 1e-6
    a, b, c = vo[fo[:, 0]], vo[fo[:, 1]], vo[fo[:, 2]]
    area = 0.5 * ((b - a)[:, 0] * (c - a)[:, 1] - (b - a)[:, 1] * (c - a)[:, 0])
    assert (area > 0).all() and 0.85 < area.sum() <= 1 + 1e-6


def test_decimate_stops_when_nothing_can_collapse(cuda):
    f4 = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32)
    v4 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    vo, fo = decimate(v4, f4, num_faces=0)
    assert len(fo) == 4 and len(vo) == 4
    vo, fo = decimate(*icosahedron(), num_faces=0)
    chi, nb = topology(vo, fo)
    assert chi == 2 and nb == 0 and len(fo) == 4


def test_remesh_botsch_sphere_edge_band_valence_and_surface(cuda):
    v, f, _, _ = rm.decimate(*icosphere(5), face_ratio=0.12)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    h = float(edge_lengths(v, f).mean())
    vo, fo = remesh(v, f, 10, None)
    chi, nb = topology(vo, fo)
    assert chi == 2 and nb == 0 and signed_volume(vo, fo) > 0.95 * signed_volume(v, f)
    el = edge_lengths(vo, fo)
    assert abs(el.mean() / h - 1) < 0.15
    assert ((el > 0.8 * h * 0.9) & (el < 4 / 3 * h * 1.1)).mean() > 0.97 and el.min() > 0.45 * h and el.max() < 1.6 * h
    val = np.bincount(fo.ravel())
    assert ((val >= 5) & (val <= 7)).mean() > 0.95 and val.min() >= 4 and val.max() <= 8
    rad = np.linalg.norm(vo, axis=1)
    assert rad.max() <= 1 + 1e-6 and rad.min() >= 1 - 0.6 * h * h
    vf, ff = remesh(v, f, 10, 0.5 * h)
    assert 3.2 < len(ff) / len(fo) < 4.8
    assert abs(edge_lengths(vf, ff).mean() / (0.5 * h) - 1) < 0.15


def test_remesh_botsch_torus_and_open_sheet(cuda):
    v, f = torus(64, 16)
    vo, fo = remesh(v, f, 10, None)
    chi, nb = topology(vo, fo)
    assert chi == 0 and nb == 0
    assert torus_distance(vo).max() < 0.02
    el = edge_lengths(vo, fo)
    assert el.max() / el.min() < 3.0
    v, f = open_sheet(25, jitter=0.4)
    v32 = v.astype(np.float32).astype(np.float64)
    bverts = lambda vv, ff: {tuple(vv[i]) for i in boundary_vertices(ff)}  # noqa: E731  (bit-exact: boundary vertices never move)
    vo, fo = remesh(v, f, 10, None)
    chi, nb = topology(vo, fo)
    assert chi == 1
    assert bverts(v32, f) <= bverts(vo, fo)
    assert np.abs(vo[:, 2] - 0.1 * np.sin(3 * vo[:, 0]) * np.cos(2 * vo[:, 1])).max() < 2e-3


def _isosurface(seed, n=28):
    from oracle import capi

    rng = np.random.default_rng(seed)
    g = np.linspace(-1, 1, n)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    vol = np.zeros((n, n, n))
    for _ in range(6):
        k = rng.uniform(1.0, 3.5, 3)
        ph = rng.uniform(0, 2 * np.pi, 3)
        vol += rng.uniform(0.5, 1.0) * np.sin(k[0] * X + ph[0]) * np.sin(k[1] * Y + ph[1]) * np.sin(k[2] * Z + ph[2])
    v, f = capi.marching_cubes(vol.astype(np.float32), 0.15)[:2]
    return v.astype(np.float64), f.astype(np.int32)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_isosurface_meshes_with_borders_keep_their_topology(cuda, seed):
    from scipy.spatial import cKDTree

    v, f = _isosurface(seed)
    chi0, nb0 = topology(v, f)
    vd, fd = decimate(v, f, face_ratio=0.4)
    chi1, nb1 = topology(vd, fd)
    assert chi1 == chi0 and (nb1 > 0) == (nb0 > 0) and len(fd) <= int(0.4 * len(f)) + 1
    vr, fr = remesh(vd, fd, 10, None)
    chi2, nb2 = topology(vr, fr)
    assert chi2 == chi0 and (nb2 > 0) == (nb0 > 0)
    h = edge_lengths(vd, fd).mean()
    assert cKDTree(vd).query(vr)[0].max() < 1.5 * h
    assert cKDTree(v).query(vr)[0].max() < 2.5 * h
    el = edge_lengths(vr, fr)
    assert ((el > 0.7 * h) & (el < 1.45 * h)).mean() > 0.9


def test_small_components_never_disappear(cuda):
    vs, fs = icosahedron()
    tri_v = np.array([[5, 0, 0], [6, 0, 0], [5, 1, 0]], np.float64)
    quad_v = np.array([[8, 0, 0], [9, 0, 0], [9, 1, 0], [8, 1, 0]], np.float64)
    v = np.concatenate([vs, tri_v, quad_v], 0)
    f = np.concatenate([fs, [[12, 13, 14]], [[15, 16, 17], [15, 17, 18]]], 0).astype(np.int32)
    chi0, nb0 = topology(v, f)
    vo, fo = decimate(v, f, num_faces=0)
    chi, nb = topology(vo, fo)
    assert chi == chi0 and nb > 0
    assert len(fo) == 4 + 1 + 1
    vr, fr = remesh(v, f, 5, 3.0)
    assert topology(vr, fr)[0] == chi0


# -------------------------------------------------------------------------------------------------------------- determinism
def test_deterministic_and_zero_iterations_is_identity(cuda):
    v, f = _isosurface(1)
    runs = [rd.remesh_botsch_device(*dev(v, f), 4, None) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    runs = [rd.decimate_device(*dev(v, f), face_ratio=0.3)[:2] for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    vt, ft = torus(32, 12)
    v0, f0 = rd.remesh_botsch_device(*dev(vt, ft), 0, None)
    assert np.array_equal(v0.cpu().numpy(), vt.astype(np.float32)) and np.array_equal(f0.cpu().numpy(), ft)


# ---------------------------------------------------------------------------------------------- agreement with the host path
def test_large_isosurface_agrees_with_the_host_remesher(cuda):
    """~10^6 faces from the project's own GPU marching cubes at 256^3 (open rims where the surface leaves the grid), through
    triangle_remesh at the add-on's 'high' budget on both paths."""
    from sculptmate_amd import ops
    from sculptmate_amd.sf3d.system import Mesh

    n = 256
    rng = np.random.default_rng(7)
    g = torch.linspace(-1, 1, n, device=cuda, dtype=torch.float32)
    X, Y, Z = torch.meshgrid(g, g, g, indexing="ij")
    vol = torch.zeros((n, n, n), device=cuda)
    for _ in range(6):
        k = rng.uniform(1.5, 4.0, 3)
        ph = rng.uniform(0, 2 * np.pi, 3)
        vol += float(rng.uniform(0.5, 1.0)) * torch.sin(k[0] * X + ph[0]) * torch.sin(k[1] * Y + ph[1]) * torch.sin(k[2] * Z + ph[2])
    v, f = ops.marching_cubes(vol.contiguous(), 0.1)
    del vol, X, Y, Z
    assert 5e5 < f.shape[0] < 3e6, f.shape
    chi0, nb0 = topology(v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64))
    assert nb0 > 0
    mesh = Mesh(v.float().contiguous(), f.long().contiguous())
    budget = round(0.75 * v.shape[0])
    hm = rm.native_remesher(mesh, "triangle", budget)
    dm = rd.device_remesher(mesh, "triangle", budget)
    assert dm.v_pos.is_cuda and dm.v_pos.dtype == torch.float32 and dm.t_pos_idx.dtype == f.long().dtype
    hv, hf = hm.v_pos.cpu().numpy().astype(np.float64), hm.t_pos_idx.cpu().numpy()
    dv, df = dm.v_pos.cpu().numpy().astype(np.float64), dm.t_pos_idx.cpu().numpy()
    assert abs(len(dv) / len(hv) - 1) <= 0.10, (len(dv), len(hv))
    chi_h, _ = topology(hv, hf)
    chi_d, nb_d = topology(dv, df)
    assert chi_d == chi_h == chi0 and nb_d > 0
    # each path remeshes at the mean edge length of its own decimated mesh: the band share of each against its own h
    def band(vv, ff, h):
        el = edge_lengths(vv, ff)
        return ((el >= 0.8 * h) & (el <= 4 / 3 * h)).mean()

    vdec, fdec, _, _ = rd.decimate_device(v, f, face_ratio=budget / v.shape[0])
    vdec_h, fdec_h, _, _ = rm.decimate(v.cpu().numpy(), f.cpu().numpy(), face_ratio=budget / v.shape[0])
    hh = float(edge_lengths(vdec_h, fdec_h).mean())  # undirected-edge mean: the same on both sides
    hd = float(edge_lengths(vdec.cpu().numpy().astype(np.float64), fdec.cpu().numpy()).mean())
    assert band(dv, df, hd) >= band(hv, hf, hh) - 0.02, (band(dv, df, hd), band(hv, hf, hh))


# -------------------------------------------------------------------------------------------------------------- capacity
def test_split_capacity_retry_when_the_first_guess_is_too_small(cuda):
    """h = 1/4 of the mean edge: the first split sweep quadruples the faces, past the 1.5x first guess of the face and vertex
    buffers; the emit runs again into exact buffers and the result is the same as with buffers that fit at once."""
    v, f = torus(40, 16)
    h = 0.25 * float(edge_lengths(v, f).mean())
    vo, fo = rd.remesh_botsch_device(*dev(v, f), 3, h)
    st = rd.last_stats()
    assert st["capacity_retries"] >= 1, st
    vo, fo = host(vo, fo)
    chi, nb = topology(vo, fo)
    assert chi == 0 and nb == 0
    assert 10 < len(fo) / len(f) < 24
    old = rd.CAPACITY_GROWTH
    try:
        rd.CAPACITY_GROWTH = 64.0  # everything fits at the first attempt
        vb, fb = rd.remesh_botsch_device(*dev(v, f), 3, h)
        assert rd.last_stats()["capacity_retries"] == 0
    finally:
        rd.CAPACITY_GROWTH = old
    assert np.array_equal(vb.cpu().numpy().astype(np.float64), vo) and np.array_equal(fb.cpu().numpy(), fo)


# ------------------------------------------------------------------------------------------------------------- bad input
def test_bad_input_is_refused_with_the_host_messages(cuda):
    from sculptmate_amd.sf3d.system import Mesh

    v, f = icosahedron()
    with pytest.raises(_lib.SculptError, match="CUDA/HIP tensor"):
        rd.remesh_botsch_device(torch.from_numpy(v), torch.from_numpy(f), 1)
    with pytest.raises(_lib.SculptError, match="CUDA/HIP tensor"):
        rd.device_remesher(Mesh(torch.from_numpy(v).float(), torch.from_numpy(f).long()), "triangle", 10)
    bad = f.copy()
    bad[3, 1] = 99
    for fn, hostfn in ((lambda: rd.decimate_device(*dev(v, bad), 0.5), lambda: rm.decimate(v, bad, 0.5)),
                       (lambda: rd.remesh_botsch_device(*dev(v, bad), 1), lambda: rm.remesh_botsch(v, bad, 1)),
                       (lambda: rd.subdivide_device(*dev(v, bad), 1), lambda: rm.subdivide(v, bad, 1))):
        with pytest.raises(_lib.SculptError) as h_err:
            hostfn()
        with pytest.raises(_lib.SculptError) as d_err:
            fn()
        assert str(d_err.value) == str(h_err.value)
    deg = f.copy()
    deg[0] = [1, 1, 2]
    with pytest.raises(_lib.SculptError, match="degenerate") as d_err:
        rd.decimate_device(*dev(v, deg), 0.5)
    with pytest.raises(_lib.SculptError) as h_err:
        rm.decimate(v, deg, 0.5)
    assert str(d_err.value) == str(h_err.value)
    nanv = v.copy()
    nanv[2, 0] = np.nan
    with pytest.raises(_lib.SculptError) as d_err:
        rd.remesh_botsch_device(*dev(nanv, f), 1)
    with pytest.raises(_lib.SculptError) as h_err:
        rm.remesh_botsch(nanv, f, 1)
    assert str(d_err.value) == str(h_err.value)
    # an empty mesh: an empty result from the operations, the remesher refuses it like the host one
    vo, fo = rd.remesh_botsch_device(*dev(np.zeros((0, 3)), np.zeros((0, 3), np.int32)), 2)
    assert vo.shape == (0, 3) and fo.shape == (0, 3)
    empty = Mesh(torch.zeros((0, 3), device=cuda), torch.zeros((0, 3), dtype=torch.long, device=cuda))
    with pytest.raises(ZeroDivisionError) as d_err:
        rd.device_remesher(empty, "triangle", 100)
    with pytest.raises(ZeroDivisionError) as h_err:
        rm.native_remesher(Mesh(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.long)), "triangle", 100)
    assert str(d_err.value) == str(h_err.value)
    m = Mesh(*[t for t in dev(v, f)])
    with pytest.raises(NotImplementedError) as d_err:
        rd.device_remesher(m, "quad", 100)
    with pytest.raises(NotImplementedError) as h_err:
        rm.native_remesher(m, "quad", 100)
    assert str(d_err.value) == str(h_err.value)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_fast3d_generator_with_the_device_remesher(cuda, tmp_path):
    """test_gpu_sf3d.py test_fast3d_generator_facade's host-remesher assertions, with SF3D.remesher = device_remesher."""
    import yaml
    from PIL import Image
    from safetensors.numpy import save_file

    from sculptmate_amd import synth
    from sculptmate_amd.sf3d import spec, system
    from sculptmate_amd.sf3d.generate import Fast3DGenerator
    from sculptmate_amd.sf3d.spec import SMALL_CFG
    from test_gpu_sf3d import _calibrated

    g = Fast3DGenerator(cuda)
    ck = tmp_path / "checkpoints"
    ck.mkdir()
    cfg = SMALL_CFG
    y = dict(cond_image_size=cfg["cond_image_size"], isosurface_resolution=cfg["isosurface_resolution"], radius=0.87,
             camera_embedder=dict(in_channels=25, out_channels=cfg["camera_embedder"]["out_channels"],
                                  conditions=["c2w_cond", "intrinsic_normed_cond"]),
             image_tokenizer=dict(pretrained_model_name_or_path="facebook/dinov2-large", width=56, height=56,
                                  modulation_cond_dim=cfg["image_tokenizer"]["modulation_cond_dim"]),
             tokenizer=dict(cfg["tokenizer"]),
             backbone={k: cfg["backbone"][k] for k in ("num_attention_heads", "attention_head_dim", "raw_triplane_channels",
                                                      "triplane_channels", "raw_image_channels", "num_latents", "num_blocks",
                                                      "num_basic_blocks", "cross_attention_dim")},
             post_processor=dict(cfg["post_processor"]),
             decoder=dict(in_channels=120, n_neurons=64, activation="silu",
                          heads=[{k: v for k, v in h.items() if v is not None} for h in cfg["decoder"]["heads"]]))
    (ck / "config.yaml").write_text(yaml.safe_dump(y))
    sd = synth.sf3d_state(0, cfg)
    save_file({k: np.ascontiguousarray(v) for k, v in sd.items()}, str(ck / "model.safetensors"))
    g.checkpoint_dir = str(ck)
    old = spec.DEFAULT_CFG["image_tokenizer"].copy()
    try:
        system.DEFAULT_CFG["image_tokenizer"].update(cfg["image_tokenizer"])
        assert g.initiate_model() == 0
    finally:
        system.DEFAULT_CFG["image_tokenizer"].clear()
        system.DEFAULT_CFG["image_tokenizer"].update(old)
    img = Image.fromarray(synth.image_rgba(5, 80), mode="RGBA")
    _, rgb = g.model.prepare_image(img)
    codes = g.model.scene_code(rgb.contiguous())
    g.model.load_state_dict(_calibrated(g.model, sd, codes))
    assert g.generate_mesh(img, "thing", remesh_option="none", texture_resolution=64, enable_texture=False) == 0
    nf_plain = g.last_mesh["faces"].shape[0]
    g.model.remesher = rd.device_remesher
    assert g.generate_mesh(img, "thing", remesh_option="triangle", texture_resolution=64, enable_texture=False) == 0
    assert rd.last_stats()["passes"] > 0  # the device path ran
    fr = np.asarray(g.last_mesh["faces"]).reshape(-1, 3)
    assert 0.2 * nf_plain < len(fr) < 0.8 * nf_plain, (nf_plain, len(fr))
    _, inv = np.unique(np.asarray(g.last_mesh["vertices"]), axis=0, return_inverse=True)
    fw = inv.reshape(-1)[fr].astype(np.int64)
    de = np.concatenate([fw[:, [0, 1]], fw[:, [1, 2]], fw[:, [2, 0]]], 0)
    assert len(np.unique(de[:, 0] * (int(fw.max()) + 2) + de[:, 1])) == len(de)
    assert g.generate_mesh(img, "thing", remesh_option="triangle", texture_resolution=64, enable_texture=True) == 0
    full = g.last_mesh
    assert full["faces"].shape[0] == len(fr) and full["uvs"].shape == (3 * len(fr), 2)
    assert full["basecolor_tex"].size == (64, 64) and full["bump_tex"].size == (64, 64)
    assert np.isfinite(np.asarray(full["vertices"])).all() and 0.0 <= np.asarray(full["uvs"]).min() and np.asarray(full["uvs"]).max() <= 1.0
