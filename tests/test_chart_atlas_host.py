"""The UV chart atlas rule on its NumPy restatement alone (tests/_chartref.py; no library, no GPU): what the rule promises of an
atlas, on the meshes the device tests compare bit for bit."""
import numpy as np
import pytest

import _chartref as cr

R = 256
BIG = ["cube", "icosphere", "nested", "torus", "helicoid", "soup"]
SMALL = ["one_face", "degenerate", "three_on_an_edge", "same_direction", "tall"]


@pytest.mark.parametrize("name,charts", [("cube", 6), ("icosphere", 6), ("nested", 18), ("torus", 10)])
def test_chart_counts_of_the_rule(name, charts):
    ref = cr.reference(name)
    assert ref["n_charts"] == charts
    assert ref["evicted"] == [0] and ref["rounds"] == 1 and ref["conflicts"] == 0
    assert (ref["layer"] == 0).all()


def test_helicoid_is_one_chart_that_overlaps_itself_and_ends_without_conflicts():
    ref = cr.reference("helicoid")
    assert ref["first_round_charts"] == 1
    assert ref["evicted"][0] > 0
    assert ref["evicted"][-1] == 0 and ref["rounds"] <= cr.MAX_ROUNDS and ref["conflicts"] == 0
    assert ref["n_charts"] > 1 and ref["layer"].max() >= 1


@pytest.mark.parametrize("name", BIG + SMALL)
def test_atlas_properties(name):
    v, f = cr.mesh(name)
    ref = cr.reference(name)
    uv = ref["uv"].reshape(-1, 3, 2).astype(np.float64)
    s, g = ref["scale"], 0.02 / cr.GUTTER_DIVISOR
    # all UVs in [0, 1]
    assert ref["uv"].min() >= 0.0 and ref["uv"].max() <= 1.0
    # orientation is kept: every face that has an area in 3-D has a positive one in UV
    c = v[f].astype(np.float64)
    n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    area3 = np.linalg.norm(n, axis=1)
    e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    area_uv = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    solid = area3 > 1e-9
    assert (area_uv[solid] > 0).all()
    # every UV edge is s times the projected edge, to the rounding of the fp32 UVs: each coordinate is within 2^-25 of its fp64
    # value (half an ulp below 1), a difference within 2^-24, the length within sqrt(2) 2^-24 < 2 * 2^-24
    d, pq = cr.directions(v, f)
    pq = pq.astype(np.float64)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        want = s * np.linalg.norm(pq[:, b] - pq[:, a], axis=1)
        got = np.linalg.norm(uv[:, b] - uv[:, a], axis=1)
        assert np.abs(got - want).max() <= 2 * 2.0 ** -24
    # no two padded chart rectangles intersect, on the integers
    ext, cell = ref["extent"], ref["cell"]
    wq, hq = cr.quant(s, ext[:, 0], g), cr.quant(s, ext[:, 1], g)
    x0, y0, x1, y1 = cell[:, 0], cell[:, 1], cell[:, 0] + wq, cell[:, 1] + hq
    assert x1.max() <= cr.ONE and y1.max() <= cr.ONE and x0.min() >= 0 and y0.min() >= 0
    order = np.argsort(y0, kind="stable")
    x0, y0, x1, y1 = x0[order], y0[order], x1[order], y1[order]
    for i in range(len(order)):            # rows are sorted by y: compare with the charts whose row can reach this one
        j = np.arange(i + 1, len(order))
        j = j[y0[j] < y1[i]]
        assert not ((x0[j] < x1[i]) & (x0[i] < x1[j]) & (y0[i] < y1[j])).any()
    # faces of one chart hold identical UV bits at shared vertices
    bits = ref["uv"].view(np.uint32).reshape(-1, 2)
    key = ref["chart"].astype(np.int64).repeat(3) * (len(v) + 1) + f.reshape(-1)
    o = np.argsort(key, kind="stable")
    same = key[o][1:] == key[o][:-1]
    assert (bits[o][1:][same] == bits[o][:-1][same]).all()
    # chart ids are the ranks of the smallest faces
    first = np.full(ref["n_charts"], len(f))
    np.minimum.at(first, ref["chart"], np.arange(len(f)))
    assert (np.diff(first) > 0).all() and first[0] == 0
    # an independent count over the final atlas: no sample strictly inside two faces
    assert cr.overlapping_samples(ref["uv"], R) == 0


def test_edge_cases_join_as_the_rule_says():
    assert cr.reference("one_face")["n_charts"] == 1
    deg = cr.reference("degenerate")
    assert deg["direction"][1] == 0                       # n = 0 takes d = 0 ...
    assert deg["direction"][0] == 4 and deg["n_charts"] == 2   # ... so the +z face across its manifold edge is not joined
    low, high = cr.rasterize(deg["uv"], R)
    assert not (low == 1).any() and not (high == 1).any()  # it covers no texel
    three = cr.reference("three_on_an_edge")
    assert three["n_charts"] == 3                         # a non-manifold edge joins nothing
    same = cr.reference("same_direction")
    assert same["n_charts"] == 2                          # inconsistent winding is never joined
    assert same["direction"].tolist() == [4, 5]
    tall = cr.reference("tall")
    assert tall["n_charts"] == 1
    r = tall["rect"][0]
    assert r[3] - r[2] > r[1] - r[0]                      # taller than wide in (p, q) ...
    assert tall["extent"][0, 0] >= tall["extent"][0, 1]   # ... turned: w >= h
    uv = tall["uv"].reshape(-1, 2)
    assert np.ptp(uv[:, 0]) > np.ptp(uv[:, 1])


def test_a_joined_pair_needs_direction_layer_and_a_manifold_edge():
    v, f = cr.mesh("tall")
    d, _ = cr.directions(v, f)
    pairs = cr.halfedge_pairs(f)
    assert len(pairs[0]) == 1
    layer = np.zeros(2, np.int32)
    assert cr.labels(2, pairs, d, layer, 4).tolist() == [0, 0]
    assert cr.labels(2, pairs, d, np.array([0, 1], np.int32), 4).tolist() == [0, 1]      # different layers
    assert cr.labels(2, pairs, d, np.array([4, 4], np.int32), 4).tolist() == [0, 1]      # singles
    assert cr.labels(2, pairs, np.array([4, 0], np.int32), layer, 4).tolist() == [0, 1]  # different directions


def test_the_strict_test_is_needed_on_the_torus():
    """Samples on shared edges are covered by two faces in fp32 and are strictly inside neither in fp64."""
    ref = cr.reference("torus")
    low, high = cr.rasterize(ref["uv"], R)
    assert ((low >= 0) & (low != high)).sum() > 0
    assert ref["evicted"] == [0]


def test_ordered_keys_round_trip_and_order():
    x = np.array([-np.inf, -2.5, -0.0, 0.0, 1e-30, 3.0, np.inf], np.float32)
    k = cr.f32_to_ordered(x)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert (cr.ordered_to_f32(k).view(np.uint32) == x.view(np.uint32)).all()


def test_scale_search_takes_the_first_feasible_step():
    ref = cr.reference("soup")
    ext = ref["extent"]
    order = np.argsort(-ext[:, 1].copy().view(np.int64), kind="stable")
    g = 0.02 / cr.GUTTER_DIVISOR
    s = ref["scale"]
    assert cr.evaluate(s, ext, order, g)[0]
    assert not cr.evaluate(s / 0.9375, ext, order, g)[0] or s == 2.0 ** round(np.log2(s))
    assert ref["rows"] > 1 and ref["n_charts"] > 1024     # more than one trip of the packer's scan


def test_setting_defaults_and_refusals():
    import torch

    from sculptmate_amd._lib import SculptError
    from sculptmate_amd.generate import TripoGenerator
    from sculptmate_amd.sf3d.unwrap import ChartUnwrapper
    from sculptmate_amd.tsr.spec import SMALL_CFG
    from sculptmate_amd.tsr.system import TSR

    assert TSR.atlas == "box" and TSR(SMALL_CFG).atlas == "box" and TripoGenerator(torch.device("cpu")).atlas == "box"
    m = TSR.__new__(TSR)          # not even an initialised model: the value is refused before anything else is looked at
    assert m.atlas == "box"
    m.atlas = "shelves"
    with pytest.raises(ValueError, match="atlas"):
        m._atlas(None, 64, 0.02, None)
    un = ChartUnwrapper()
    assert un.raster_resolution == 1024 and un.max_layers == 4 and un.last == {}
    assert ChartUnwrapper.GUTTER_DIVISOR == cr.GUTTER_DIVISOR and ChartUnwrapper.MAX_ROUNDS == cr.MAX_ROUNDS
    with pytest.raises(SculptError, match="no CPU fallback"):
        un(torch.zeros(3, 3), torch.zeros(3, 3), torch.tensor([[0, 1, 2]]), 0.02)
    with pytest.raises(ValueError):
        ChartUnwrapper(raster_resolution=0)
