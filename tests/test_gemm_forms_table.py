"""The table of tests/test_gpu_gemm_forms.py audited without a device: every launch in csrc/gemm.hip has a row or a reason, and every
row runs the K-tile counts and strides it is there for."""
import os
import re

import test_gpu_gemm_forms as T
from conftest import ROOT


def _launches_in_source():
    """Every launch in csrc/gemm.hip as a tuple of T.KEYS, by a plain text scan for the launch macro."""
    src = open(os.path.join(ROOT, "sculptmate_amd", "csrc", "gemm.hip")).read()
    epi = {v: k for k, v in T.EPI_NAME.items()}
    n_macro = len(re.findall(r"\bhipLaunchKernelGGL\s*\(", src))
    found, n_text = [], 0
    for m in re.finditer(r"\bhipLaunchKernelGGL\s*\(\s*\(\s*(gemm_bf16_kernel|gemm256_kernel)\s*<([^>]*)>", src):
        n_text += 1
        a = [s.strip() for s in m.group(2).split(",")]
        # the 256 family's launches sit in a macro whose epilogue is the parameter E: one launch per use of the macro
        epis = [epi[a[0]]] if a[0] in epi else [epi[e] for e in re.findall(r"\bSCULPT_G256\((SCULPT_EPI_\w+)\)", src)]
        assert epis, "a launch with epilogue %r and no use of its macro" % a[0]
        for e in epis:
            if m.group(1) == "gemm256_kernel":
                found.append(("g256", e, 256, 8, int(a[1]), 0, int(len(a) > 2 and a[2] == "true"), 0))
            else:
                bm = 128 if len(a) < 5 or a[4] == "BM_DEFAULT" else int(a[4])
                found.append(("g128", e, int(a[1]), int(a[2]), bm, int(len(a) > 6 and a[6] == "true"), 0, int(len(a) > 3 and a[3] == "true")))
    assert n_text == n_macro, "%d uses of the launch macro, %d of them launch a GEMM kernel this scan understands" % (n_macro, n_text)
    return found


def test_every_launch_of_the_launcher_is_accounted_for():
    """T.FORMS + T.CONV_FORMS + T.UNREACHABLE == the launches in the source, one for one: a new instantiation needs a row (or a reason),
    a removed one has to leave the table."""
    found = _launches_in_source()
    assert len(found) == len(set(found)), "the same instantiation is launched from two places"
    table = {tuple(f[k] for k in T.KEYS): n for n, (f, *_) in list(T.FORMS.items()) + list(T.CONV_FORMS.items())}
    assert len(table) == len(T.FORMS) + len(T.CONV_FORMS), "two rows name the same form"
    assert not set(table) & set(T.UNREACHABLE), "a row is also listed as unreachable"
    missing = set(found) - set(table) - set(T.UNREACHABLE)
    stale = (set(table) | set(T.UNREACHABLE)) - set(found)
    assert not missing, "launches no row reaches and no reason excuses: %s" % sorted(missing)
    assert not stale, "rows / reasons for instantiations the launcher no longer has: %s" % sorted(stale)
    assert len(found) == 28 and len(T.UNREACHABLE) == 4      # 24 uses of the macro, the two in SCULPT_G256 x three epilogues
    # `nw8` is still the constant the reasons lean on
    src = open(os.path.join(ROOT, "sculptmate_amd", "csrc", "gemm.hip")).read()
    assert re.search(r"const bool nw8 = true\b", src)


def test_every_row_runs_its_k_tile_counts_and_strides():
    """K-tile counts 1 .. 5 for every row of the 128 family, 2 .. 5 for the 256 family (its kernels need two K-tiles), and a deep
    launch (K = 4096) in each family; the 4-wave rows exist only at K >= 2048 and say so.  Every row has a launch with lda > K and
    one with ldo > N; every row of the 256 family but the residual form (fp32 output, never staged) asserts staged stores."""
    deep = {"g128": False, "g256": False}
    for name, (form, _, launches) in T.FORMS.items():
        counts = {c["K"] // 64 for c in launches}
        if form["nw"] == 4:
            assert min(counts) >= 32, name
        else:
            want = set(range(1, 6)) if form["family"] == "g128" else set(range(2, 6))
            assert want <= counts, "%s runs K-tile counts %s, not %s" % (name, sorted(counts), sorted(want - counts))
        deep[form["family"]] |= 64 in counts
        assert any(c["lda"] for c in launches) and any(c["ldo"] for c in launches), "%s: no launch with lda > K / ldo > N" % name
        if form["family"] == "g256" and not form["res"]:
            assert any(c["expect"].get("stage") == 1 for c in launches) and any(c["expect"].get("stage") == 0 for c in launches), name
    assert all(deep.values()), deep
