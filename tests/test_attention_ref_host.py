"""tests/_attnref.py tried without a device: its bound holds for an emulation of the attention kernels' arithmetic and is exceeded
by every kind of fault the device tests are there to catch; and the table of tests/test_gpu_attention_forms.py audited against the
launch sites in csrc/attention.hip and attention_pipe.hip."""
import itertools
import os
import re

import numpy as np
import pytest

import _attnref as R
import test_gpu_attention_forms as T
from conftest import ROOT

HEADS, TQ = 2, 130
DEEP = (1025, 3089)
FAULT_TKS = (65, 129, 385, 1025)


def _case(Tk, pre):
    rng = np.random.default_rng(1000 * Tk + pre)
    scale = None if pre else T.SCALE
    q, k, v = R.operands(rng, TQ, Tk, HEADS, scale)
    return q, k, v, scale


@pytest.fixture(scope="module")
def refs():
    """The fp64 reference of every (Tk, entry) of this file, computed once."""
    out = {}
    for Tk in sorted(set(T.TKS) | set(DEEP) | set(FAULT_TKS)):
        for pre in (0, 1):
            q, k, v, scale = _case(Tk, pre)
            out[Tk, pre] = (q, k, v, scale, R.reference(q, k, v, HEADS, scale))
    return out


def test_the_bound_holds_for_the_emulation(refs):
    """Over every key count of the device tests and running maxima that lag by 0, 5 and 10 log2 units."""
    top = (0.0, "")
    for (Tk, pre), (q, k, v, scale, ref) in sorted(refs.items()):
        for lag in (0.0, 5.0, 10.0):
            w, where, text = R.worst(R.emulate(q, k, v, HEADS, scale, lag=lag), ref, label="Tk=%d pre=%d lag=%g" % (Tk, pre, lag))
            top = max(top, (w, text))
            assert w <= 1.0, text
    print("largest error / B of the emulation: %s" % top[1])


@pytest.mark.parametrize("kind,Tk", [("rescale", 449), ("rescale", 385), ("threshold", 385), ("census", 385)])
def test_the_bound_holds_for_the_emulation_on_the_built_operands(kind, Tk):
    """The spikes, the threshold scores and the key census of the device tests: huge scores give a one-hot row no slack, and M's
    16 bits (pre-scaled) stay inside the two u terms."""
    for pre in ((1,) if kind == "threshold" else (0, 1)):
        c = T.L(kind, TQ, Tk)
        q, k, v = T.MAKE[kind](np.random.default_rng(Tk + pre), c, bool(pre))
        scale = None if pre else T.SCALE
        ref = R.reference(q, k, v, HEADS, scale)
        for lag in (0.0, 5.0, 10.0):
            w, _, text = R.worst(R.emulate(q, k, v, HEADS, scale, lag=lag), ref, label="%s Tk=%d pre=%d lag=%g" % (kind, Tk, pre, lag))
            print(text)
            assert w <= 1.0, text


def test_the_row_sum_of_the_rounded_probabilities_stays_inside(refs):
    """Taking l from the bf16-rounded p is inside the contract: the bound must not be tighter than that."""
    for Tk in FAULT_TKS:
        for pre in (0, 1):
            q, k, v, scale, ref = refs[Tk, pre]
            for lag in (0.0, 10.0):
                w, _, text = R.worst(R.emulate(q, k, v, HEADS, scale, lag=lag, l_from_bf16=True), ref, label="Tk=%d pre=%d lag=%g, l from bf16 p" % (Tk, pre, lag))
                assert w <= 1.0, text


def _faults(q, k, v, Tk):
    """name -> (q, k, v) the faulty kernel effectively works on, or a function of the correct output."""
    j = Tk // 2
    dup = np.r_[0:j + 1, j:Tk]
    swap = np.arange(Tk)
    swap[[j, j - 1]] = swap[[j - 1, j]]
    pad_k, pad_v = np.vstack([k, k[Tk - 1:Tk]]), np.vstack([v, np.full((1, v.shape[1]), 7.0, np.float32)])
    return {
        "the last key dropped": (q, k[:-1], v[:-1]),
        "one key counted twice": (q, k[dup], v[dup]),
        "a masked padding key (7.0) weighted like a real key": (q, pad_k, pad_v),
        "two keys exchanged between P and V^T": (q, k, v[swap]),
    }


@pytest.mark.parametrize("Tk", FAULT_TKS)
def test_the_bound_has_teeth(refs, Tk):
    for pre in (0, 1):
        q, k, v, scale, ref = refs[Tk, pre]
        for name, (fq, fk, fv) in _faults(q, k, v, Tk).items():
            w, _, text = R.worst(R.emulate(fq, fk, fv, HEADS, scale, lag=10.0 if pre else 0.0), ref, label="Tk=%d pre=%d %s" % (Tk, pre, name))
            print(text)
            assert w > 1.0, "the bound does not see this fault: " + text
        good = R.emulate(q, k, v, HEADS, scale)
        for i, d in ((0, 0), (TQ - 1, 64 * HEADS - 1), (TQ // 2, 77)):
            off = good.copy()
            off[i, d] += 0.03
            w, where, text = R.worst(off, ref, label="Tk=%d pre=%d one element off by 0.03" % (Tk, pre))
            assert w > 1.0 and (where["query"], 64 * where["head"] + where["d"]) == (i, d), text


# ------------------------------------------------------------------------------------------------------- the table
def _launch_sites():
    """Every instantiation the launcher can start, as (kernel, nqb, pre), by a plain text scan of the two sources."""
    csrc = os.path.join(ROOT, "sculptmate_amd", "csrc")
    plain = open(os.path.join(csrc, "attention.hip")).read()
    pipe = open(os.path.join(csrc, "attention_pipe.hip")).read()
    found = [("plain", int(n), int(p == "true")) for n, p in re.findall(r"\bSCULPT_ATTN_LAUNCH\(\s*(\d+)\s*,\s*(true|false)\s*,", plain)]
    # the macro is the only launch of attention.hip; attention_pipe.hip launches by name
    assert len(re.findall(r"\bhipLaunchKernelGGL\s*\(", plain)) == 1
    assert re.search(r"define SCULPT_ATTN_LAUNCH\(NQB, PRE, SC\)\s*\\\s*hipLaunchKernelGGL\(\(attention_kernel<NQB, PRE>\)", plain)
    by_name = re.findall(r"\bhipLaunchKernelGGL\s*\(\s*\(\s*attention_pipe_kernel\s*<\s*(\d+)\s*>", pipe)
    assert len(by_name) == len(re.findall(r"\bhipLaunchKernelGGL\s*\(", pipe))
    return found + [("pipe", int(n), 1) for n in by_name]


def test_every_launch_site_has_exactly_one_row():
    found = _launch_sites()
    assert len(found) == len(set(found)), "the same instantiation is launched from two places"
    table = [tuple(f[k] for k in T.KEYS) for f, _, _ in T.FORMS.values()]
    assert len(table) == len(set(table)), "two rows name the same form"
    assert not set(found) - set(table), "instantiations without a row: %s" % sorted(set(found) - set(table))
    assert not set(table) - set(found), "rows for instantiations the launcher no longer has: %s" % sorted(set(table) - set(found))
    assert len(found) == 8
    assert set(T.UNREACHABLE_BY_DEFAULT) <= set(table)


def test_every_row_runs_its_kinds_shapes_and_token():
    for name, (form, token, launches) in T.FORMS.items():
        n, pre = form["nqb"], form["pre"]
        kinds = {c["kind"] for c in launches}
        assert kinds == set(T.KINDS) - (set() if pre else {"threshold"}), name
        assert all(c["heads"] == 2 for c in launches if c["token"] == "row"), name
        forced = [c for c in launches if c["token"] == "row"]
        assert set(T.TKS) <= {c["Tk"] for c in forced}, "%s misses key counts %s" % (name, sorted(set(T.TKS) - {c["Tk"] for c in forced}))
        assert {c["Tq"] for c in forced if c["kind"] == "random"} == {1, 32 * n - 1, 32 * n, 32 * n + 1, 64 * n + 1}, name
        assert any(c["Tk"] in DEEP for c in forced), name
        assert {(c["batch"], c["vt"]) for c in launches if c["kind"] == "batch"} == {(3, "side"), (3, "each")}, name
        assert {c["census"] for c in launches if c["kind"] == "census"} == {0, 1}, name
        # the token forces exactly this row: nqb, and the phase-separated loop where the pipelined one would run
        words = token.split(",")
        assert "nqb=%d" % n in words and (("nopipe" in words) == (form["kernel"] == "plain" and pre == 1 and n != 8)), name
        # a launch without a token reaches the row through the default rule, and only rows listed as unreachable have none
        free = [c for c in launches if c["token"] is None]
        key = tuple(form[k] for k in T.KEYS)
        assert bool(free) != (key in T.UNREACHABLE_BY_DEFAULT), name
        for c in free:
            assert T.default_nqb(c["Tq"], c["heads"], c["batch"], bool(pre)) == n, (name, c)
            assert form["kernel"] == ("pipe" if pre and n != 8 else "plain")


def test_the_default_rule_by_hand_and_what_it_never_reaches():
    """The shapes of the issue on 256 CUs, the restated rule against the source's constants, and a search for a pre-scaled shape
    that takes 256 queries per workgroup (there is none, on any CU count: cost(4) <= cost(8) always)."""
    src = open(os.path.join(ROOT, "sculptmate_amd", "csrc", "attention.hip")).read()
    assert re.search(r"const long w = prescaled \? 98 : 115;", src) and re.search(r"long best = cost8 \* 100;", src)
    assert re.search(r"for \(int c : \{6, 4\}\)", src) and re.search(r"if \(cost \* w < best\)", src)
    assert T.default_nqb(384, 16, 8, True) == 6 and T.default_nqb(384, 16, 8, False) == 6
    assert T.default_nqb(256, 16, 16, False) == 8 and T.default_nqb(256, 16, 16, True) == 4
    assert T.default_nqb(3072, 16, 1, True) == 6 and T.default_nqb(129, 2, 1, False) == 4
    for cus in (256, 304, 64, 8):
        for Tq, bh in itertools.product(list(range(1, 1100, 7)) + [3072, 27648], (1, 2, 12, 16, 48, 128, 256, 1000)):
            assert T.default_nqb(Tq, bh, 1, True, cus) != 8, (Tq, bh, cus)


def test_spike_keys_cover_the_halves_of_the_first_three_and_the_last_pair():
    assert T.spike_keys(449) == [0, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448]
    assert T.spike_keys(385) == [0, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384]
    assert T.spike_keys(640)[-4:] == [512, 575, 576, 639]
