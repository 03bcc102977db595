"""The geometry chain of TSR.extract_meshes (TSR._reshaped, TSR._check_geometry) without a GPU: which ops.mesh_* calls it makes,
in which order and with which arguments, on recorders in place of the device functions."""
import itertools
import math

import numpy as np
import pytest

ORDER = ("keep_components", "smooth", "simplify", "project")
VALUES = dict(keep_components="largest", smooth=3, simplify=0.5, project=True)
RULES = dict(keep_components="keep_rule", smooth="smooth_rule", simplify="simplify_rule", project="project_rule")


@pytest.fixture
def chain(monkeypatch):
    """A TSR without weights whose ops.mesh_* are recorders -- each returns its mesh with its own name appended -- and whose
    ops.*_rule note that they were asked before they answer.  -> (model, calls, rules asked)."""
    from sculptmate_amd import ops
    from sculptmate_amd.tsr import TSR
    from sculptmate_amd.tsr.spec import SMALL_CFG

    calls, asked = [], []

    def keep(v, f, rule):
        calls.append(("keep_components", v, f, rule))
        return v + ("keep_components",), f + ("keep_components",), None, None

    def smooth(v, f, rule):
        calls.append(("smooth", v, f, rule))
        return v + ("smooth",)

    def simplify(v, f, rule):
        calls.append(("simplify", v, f, rule))
        return v + ("simplify",), f + ("simplify",), None

    def project(planes, mlp, v, f, target, max_dist, **kw):
        calls.append(("project", v, f, dict(kw, planes=planes, mlp=mlp, target=target, max_dist=max_dist)))
        return v + ("project",), {}

    for name, fn in (("mesh_keep_components", keep), ("mesh_smooth", smooth), ("mesh_simplify", simplify), ("mesh_project", project)):
        monkeypatch.setattr(ops, name, fn)
    for option, name in RULES.items():
        def rule(x, option=option, real=getattr(ops, name)):
            asked.append(option)
            return real(x)

        monkeypatch.setattr(ops, name, rule)
    return TSR(SMALL_CFG), calls, asked


def test_every_subset_runs_its_steps_in_the_fixed_order(chain):
    m, calls, asked = chain
    for chosen in itertools.product((False, True), repeat=4):
        want = [name for name, on in zip(ORDER, chosen) if on]
        options = {name: VALUES[name] for name in want}
        del calls[:], asked[:]
        m._check_geometry(25.0, **options)
        assert sorted(asked) == sorted(want) and calls == []      # every set rule, no other, and nothing launched
        del asked[:]
        v, f = m._reshaped(("v",), ("f",), "planes", 25.0, 32, **options)
        assert [c[0] for c in calls] == want
        assert set(asked) <= set(want)                              # an unset option reaches neither its mesh_* nor its rule
        assert v == ("v",) + tuple(want)                            # each step was handed what the step before it returned
        assert f == ("f",) + tuple(n for n in want if n in ("keep_components", "simplify"))
        for before, (name, vin, fin, rule) in enumerate(calls):
            assert vin == ("v",) + tuple(want[:before])
            assert fin == ("f",) + tuple(n for n in want[:before] if n in ("keep_components", "simplify"))
            assert name == "project" or rule == VALUES[name]
    # explicit Nones are unset options
    assert m._reshaped(("v",), ("f",), "planes", 25.0, 32, **dict.fromkeys(ORDER)) == (("v",), ("f",))


@pytest.mark.parametrize("project,steps,cells", [(True, 8, 1.0), (3, 3, 1.0), ((3, 0.5), 3, 0.5)])
def test_project_receives_the_models_target_and_trust_radius(chain, project, steps, cells):
    m, calls, _ = chain
    cfg, R, threshold = m.renderer.cfg, 32, 1.75
    v, f = m._reshaped(("v",), ("f",), "planes", threshold, R, project=project)
    assert (v, f) == (("v", "project"), ("f",)) and len(calls) == 1
    got = calls[0][3]
    assert got["target"] == float(np.float32(math.log(threshold) - float(cfg.density_bias)))
    assert got["max_dist"] == cells * 2 * float(cfg.radius) / (R - 1)
    assert got["steps"] == steps and got["radius"] == cfg.radius and got["planes"] == "planes" and got["mlp"] is m.decoder
