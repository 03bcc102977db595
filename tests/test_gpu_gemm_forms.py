"""Every tile form of the bf16 GEMM launcher (csrc/gemm.hip: sculpt_gemm_bf16_ln, sculpt_conv3x3_bf16), reached on purpose and held,
element by element, to the fp64 bounds of tests/_gemmref.py.

FORMS is the table: one row per instantiation the launcher can launch -- its fields as sculpt_gemm_last_form reports them, the
SCULPT_GEMM_TILE token that forces it where the default rules of a 256-CU chip send no shape there, and the launches that reach
it.  Every launch asserts ops.gemm_last_form() against its row BEFORE any number is looked at, so a changed dispatch rule fails
here instead of quietly moving a shape to another kernel.  UNREACHABLE lists the instantiations nothing can reach;
tests/test_gemm_forms_table.py (no device needed) counts the launches in the source against both and audits the table's coverage.

Launch shapes: the smallest the rules allow; K small unless the case is about K; every row runs K-tile counts 1 .. 5 (the 3-stage
ring's indices and counted waits; 2 .. 5 in the 256 family, whose kernels need two; the 4-wave rows exist only at K >= 2048), and
each family has a deep launch (K = 4096) -- tests/test_gemm_forms_table.py checks that of the table.  Launches whose fp64
reference would pass ~5 GFLOP are referenced on a subset of rows (every tile edge and a stride: _gemmref.edge_rows); the
sentinel checks and the bit identities between outputs still cover every element."""
import math

import numpy as np
import pytest
import torch

import _gemmref as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NONE, GELU, GEGLU, RELU = G.EPI_NONE, G.EPI_GELU, G.EPI_GEGLU, G.EPI_RELU
EPI_NAME = {NONE: "SCULPT_EPI_NONE", GELU: "SCULPT_EPI_GELU", GEGLU: "SCULPT_EPI_GEGLU", RELU: "SCULPT_EPI_RELU"}


def F(family, epi, bw, nw, bm, ks=0, res=0, conv=0):
    return {"family": family, "epi": epi, "bw": bw, "nw": nw, "bm": bm, "ks": ks, "res": res, "conv": conv}


def L(M, N, K, outs="f", **kw):
    """One launch.  outs: letters of f (fp32), b (bf16), t (transposed bf16).  kw: split (n_split), bias (default True), res
    ("out" / "in" place / None), ln (LayerNorm fold), stats (stats_out), offset (added to the residual rows), lda / ldo (extra
    elements of row stride: A wider than K, the outputs a column slice), token (overrides the row's), subset (rows subset
    reference), expect (further fields of the report: stage, gm), images (stacked single-image passes, rows-per-image = M)."""
    d = dict(M=M, N=N, K=K, outs=outs, split=None, bias=True, res=None, ln=False, stats=False, offset=0.0, lda=0, ldo=0, token=None,
             subset=False, expect={}, images=1)
    d.update(kw)
    return d


def forced(token, launches):
    """The launches under a forcing token (one that names its own keeps it)."""
    return [dict(c, token=c["token"] or token) for c in launches]


def staged(nout, launches):
    """The 256 family's launches with the `stage` each must report (one that names its own keeps it).  Staged stores: bf16
    outputs only, and every tile entirely token-major or entirely transposed -- no fp32 output, a bf16 output, a transposed
    output only behind a column split, the split on a tile boundary (nout columns).  The buffers of this file always meet the
    alignment half of the rule (row strides multiples of 8 elements, 16-byte aligned starts)."""
    out = []
    for c in launches:
        on = "f" not in c["outs"] and "b" in c["outs"] and ("t" not in c["outs"] or bool(c["split"])) and (not c["split"] or c["split"] % nout == 0)
        out.append(dict(c, expect=dict({"stage": int(on)}, **c["expect"])))
    return out


def plain_edges(Ms, N, bn, kmin=1, res=True, t=True, stats=True):
    """The edges of a NONE form in eight launches: K-tiles kmin .. 5, the rows Ms in turn, every combination of output pointers,
    the column split on and off a tile boundary, bias absent, residual in and out of place, LayerNorm fold, stats_out with the
    rows offset by ~100 sigma, lda > K, ldo > N."""
    ks = [64 * k for k in range(kmin, 6)]
    m = lambda i: Ms[i % len(Ms)]
    k = lambda i: ks[i % len(ks)]
    out = [L(m(0), N, k(0), "fbt" if t else "fb"),
           L(m(1), N, k(1), "f", bias=False, res="out" if res else None, stats=stats and res, offset=170.0 if res else 0.0, lda=8),
           L(m(2), N, k(2), "fb", res="in" if res else None, stats=stats and res, ldo=16),
           L(m(0), N, k(3), "b", ln=True, ldo=8),
           L(m(1), N, k(4), "f", ln=True, bias=False)]
    if t:
        out += [L(m(2), N, k(2), "bt", split=bn, ln=True),
                L(m(1), N, k(0) if kmin == 1 else k(1), "ft", split=bn + 16, lda=16),
                L(m(0), N, k(1), "fbt", split=N - 16, bias=False),
                L(m(2), N, k(3), "t"),
                L(m(1), N, k(4), "bt")]
    return out


def act_edges(Ms, N, kmin=1, res=False, t=True):
    """The edges of a GELU / RELU / GEGLU form: K-tiles, rows, output pointers, bias absent, LayerNorm fold, strides."""
    ks = [64 * k for k in range(kmin, 6)]
    m = lambda i: Ms[i % len(Ms)]
    k = lambda i: ks[i % len(ks)]
    out = [L(m(0), N, k(0), "fb"),
           L(m(1), N, k(1), "f", bias=False, lda=8, res="out" if res else None),
           L(m(2), N, k(2), "b", ln=True, ldo=8),
           L(m(0), N, k(3), "f", ln=True, ldo=16),
           L(m(1), N, k(4), "fb", ln=True, bias=False)]
    if t:
        out += [L(m(2), N, k(1), "fbt"), L(m(0), N, k(2), "bt", split=N // 2)]
    return out


# Shapes behind the default-rule launches, on 256 CUs (csrc/gemm.hip, the launcher):
#   small (64-row weight tile): (N/128) ceil(M/128) < 384;  underfilled: (N/64) ceil(M/128) < 256;  4 waves: K >= 2048, not underfilled
#   one round of 192 x 64: M % 192 == 0 and 192 <= (N/64)(M/192) <= 256
#   256 family: at least 512 tiles of 256 rows (N >= 4096 unless GEGLU); 192-row tiles: M % 192 == 0, K >= 1024, >= 192 tiles;
#   residual form: M % 192 == 0 and 192 <= (N/256)(M/192) <= 640
M128 = [1, 129, 127]
FORMS = {
    # ---- gemm_bf16_kernel, 8 waves
    "g128 GEGLU 128": (F("g128", GEGLU, 128, 8, 128), None, act_edges([1, 129, 255], 128, t=False) + [L(130, 192, 4096, "fb", ln=False)]),
    # not underfilled and not "one round": N = 1024 needs 1921 .. 2048 rows that are no multiple of 192; K < 2048
    "g128 NONE 64": (F("g128", NONE, 64, 8, 128), None,
                     [L(1921, 1024, 64, "fbt", res="out", stats=True), L(1921, 1024, 128, "t", lda=8),
                      L(2047, 1024, 192, "bt", split=512, ln=True), L(1921, 1024, 256, "b", bias=False, ldo=8),
                      L(1923, 1024, 320, "f", bias=False, res="in", stats=True, offset=170.0),
                      L(2047, 1024, 128, "ft", split=528, ldo=16), L(1921, 1024, 1984, "fb", subset=True)]),
    # at least 384 tiles of 128 x 128: 49152 columns for one row tile, 24576 for two, 16384 for three
    "g128 NONE 128": (F("g128", NONE, 128, 8, 128), None,
                      [L(1, 49152, 64, "fbt"), L(129, 24576, 128, "f", bias=False, res="out", stats=True, offset=170.0, lda=8),
                       L(127, 49152, 192, "fb", res="in", stats=True, ldo=16), L(129, 24576, 256, "b", ln=True, ldo=8),
                       L(1, 49152, 320, "f", ln=True, bias=False), L(129, 24576, 64, "bt", split=12288 + 16, ln=True),
                       L(257, 16384, 192, "fbt"), L(1, 49152, 256, "t"), L(129, 24576, 128, "ft", split=12288, lda=16),
                       L(129, 24576, 4096, "f", subset=True)]),
    "g128 GELU 64": (F("g128", GELU, 64, 8, 128), None, act_edges(M128, 256, res=True)),
    "g128 GELU 128": (F("g128", GELU, 128, 8, 128), None, [L(1, 49152, 64, "fb"), L(129, 24576, 192, "f", bias=False, res="out", lda=8),
                                                           L(257, 16384, 320, "b", ln=True, ldo=8), L(127, 49152, 128, "fbt", ln=True),
                                                           L(129, 24576, 256, "bt", split=12288, ldo=16)]),
    "g128 RELU 64": (F("g128", RELU, 64, 8, 128), None, act_edges(M128, 256, res=True)),
    "g128 RELU 128": (F("g128", RELU, 128, 8, 128), None, [L(1, 49152, 64, "fb"), L(129, 24576, 192, "f", bias=False, res="out", lda=8),
                                                           L(257, 16384, 320, "b", ln=True, ldo=8), L(127, 49152, 128, "fbt", ln=True),
                                                           L(129, 24576, 256, "bt", split=12288, ldo=16)]),
    # ---- 4 waves: only at K >= 2048 on a chip that is not underfilled, so K-tile counts 1 .. 5 do not exist for these rows
    # (32 and 64 K-tiles; the 8-wave rows of the same template run the small counts)
    "g128 NONE 64 nw4": (F("g128", NONE, 64, 4, 128), None, [L(1921, 1024, 2048, "fb", res="out", stats=True, subset=True, lda=8),
                                                             L(2047, 1024, 4096, "bt", split=528, subset=True, ldo=8)]),
    "g128 GELU 64 nw4": (F("g128", GELU, 64, 4, 128), None, [L(1921, 1024, 2048, "fb", subset=True, lda=8, ldo=16)]),
    "g128 RELU 64 nw4": (F("g128", RELU, 64, 4, 128), None, [L(1921, 1024, 2048, "fbt", subset=True, lda=16, ldo=8)]),
    # ---- fewer tiles than CUs: 64 x 64 tiles
    "g128 NONE 64 bm64": (F("g128", NONE, 64, 8, 64), None, plain_edges([1, 65, 63, 129], 256, 64)),
    # ---- one round of 192 x 64 tiles, k-split pairs (default) and the weight-row split (token)
    "g128 NONE 64 bm192 ks": (F("g128", NONE, 64, 8, 192, ks=1), None,
                              plain_edges([2304], 1024, 64) + [L(3072, 768, 4096, "fb", res="out", stats=True, subset=True),
                                                               L(2304, 1024, 256, "fb", res="out", stats=True, images=2)]),
    "g128 NONE 64 bm192": (F("g128", NONE, 64, 8, 192), "bm192,ks0", plain_edges([192, 384, 576], 256, 64)),
    # ---- gemm256_kernel: the default rules need >= 512 tiles; the edges run under the forcing token
    "g256 NONE 256": (F("g256", NONE, 256, 8, 256), None,
                      [L(8064, 4096, 128, "b", subset=True, expect={"stage": 1, "gm": "nonzero"}), L(8064, 4096, 192, "f", subset=True, expect={"stage": 0})] +
                      forced("256,no192", staged(256, plain_edges([1, 257, 255], 512, 256, kmin=2, res=False) + [L(300, 512, 4096, "bt", split=256, ln=False), L(257, 512, 192, "bt", split=256)]) +
                             [L(257, 512, 256, "b", token="256,no192,nostage", expect={"stage": 0})])),
    "g256 GELU 256": (F("g256", GELU, 256, 8, 256), None,
                      [L(8064, 4096, 128, "b", subset=True, expect={"stage": 1})] +
                      forced("256,no192", staged(256, act_edges([1, 257, 255], 512, kmin=2)))),
    "g256 GEGLU 256": (F("g256", GEGLU, 256, 8, 256), None,
                       [L(3968, 4096, 128, "b", subset=True, expect={"stage": 1}), L(3968, 4096, 320, "fb", ln=True, subset=True, expect={"stage": 0})] +
                       forced("256,no192", staged(128, act_edges([1, 257, 255], 256, kmin=2, t=False)))),
    "g256 NONE 192": (F("g256", NONE, 256, 8, 192), None,
                      [L(3072, 3072, 1024, "bt", split=2048, ln=True, subset=True, expect={"stage": 1}),
                       L(3072, 3072, 1024, "f", subset=True, expect={"stage": 0})] +
                      forced("256,192", staged(256, plain_edges([1, 193, 191], 512, 256, kmin=2, res=False) + [L(193, 512, 192, "bt", split=256)]))),
    "g256 GELU 192": (F("g256", GELU, 256, 8, 192), None,
                      [L(3072, 3072, 1024, "b", ln=True, subset=True, expect={"stage": 1})] +
                      forced("256,192", staged(256, act_edges([1, 193, 191], 512, kmin=2)))),
    "g256 GEGLU 192": (F("g256", GEGLU, 256, 8, 192), None,
                       [L(3072, 1536, 1024, "b", ln=True, subset=True, expect={"stage": 1}), L(3072, 1536, 1024, "f", ln=True, subset=True)] +
                       forced("256,192", staged(128, act_edges([1, 193, 191], 256, kmin=2, t=False)))),
    "g256 NONE 192 res": (F("g256", NONE, 256, 8, 192, res=1), None,
                          [L(9216, 1024, 128, "fb", res="in", stats=True, offset=170.0, subset=True),
                           L(9216, 1024, 128, "fb", res="out", stats=True, images=2, subset=True)] +
                          [L(193, 512, 320, "f", res="out", stats=True, bias=False, token="res", lda=8),
                           L(191, 512, 256, "fb", res="in", ln=True, token="res", ldo=16),
                           L(1, 256, 128, "fb", res="out", stats=True, token="res"),
                           L(193, 512, 192, "fb", res="out", stats=True, token="res"),
                           L(384, 512, 4096, "f", res="out", token="res")]),
}
# more than 512 tiles: the grouped tile order (gm > 0) of the 128 family (the 256 family's: "g256 NONE 256" above)
FORMS["g128 NONE 128"][2].append(L(2049, 3968, 128, "fb", expect={"gm": "nonzero"}))

# instantiations the launcher names and nothing reaches: `nw8` is the constant true (8-wave workgroups measured faster on every
# shape), so its four else-branches are dead
UNREACHABLE = {
    ("g128", GEGLU, 128, 4, 128, 0, 0, 0): "nw8 is the constant true",
    ("g128", GELU, 128, 4, 128, 0, 0, 0): "nw8 is the constant true",
    ("g128", RELU, 128, 4, 128, 0, 0, 0): "nw8 is the constant true",
    ("g128", NONE, 128, 4, 128, 0, 0, 0): "nw8 is the constant true",
}
# sculpt_conv3x3_bf16's four (numerics: test_gpu_u2net_layers.py); reached by test_conv_launches_fill_the_record
CONV_FORMS = {
    "conv RELU 64": (F("g128", RELU, 64, 8, 128, conv=1), (1, 24, 20, True)),
    "conv RELU 128": (F("g128", RELU, 128, 8, 128, conv=1), (2, 192, 128, True)),
    "conv NONE 64": (F("g128", NONE, 64, 8, 128, conv=1), (1, 24, 20, False)),
    "conv NONE 128": (F("g128", NONE, 128, 8, 128, conv=1), (2, 192, 128, False)),
}
KEYS = ("family", "epi", "bw", "nw", "bm", "ks", "res", "conv")

CASES = [(name, i) for name, (_, _, launches) in FORMS.items() for i in range(len(launches))]


def _bf16_np(t):
    """bf16 tensor -> uint16 patterns."""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _to_bf16_dev(x32, cuda, ld=0):
    """fp32 array -> device bf16 [rows][cols] view of a buffer whose rows are ld elements longer; and the rounded values (fp32)."""
    t = torch.from_numpy(x32).to(BF)
    buf = torch.zeros(t.shape[0], t.shape[1] + ld, dtype=BF, device=cuda)
    buf[:, :t.shape[1]] = t.to(cuda)
    return buf[:, :t.shape[1]], t.float().numpy()


def _operands(c, seed, cuda):
    M, N, K = c["M"] * c["images"], c["N"], c["K"]
    rows_w = 2 * N if c["epi"] == GEGLU else N
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((M, K), dtype=np.float32)
    if c["ln"]:
        h += 3.0 * rng.standard_normal((M, 1), dtype=np.float32)            # |mean| ~ 3 sigma
        low = np.arange(M - 1, -1, -5)                                       # the last row and every fifth before it: variance ~1e-4
        h[low] = (0.03 * np.sign(rng.standard_normal((len(low), 1))) + 0.01 * rng.standard_normal((len(low), K))).astype(np.float32)
    A_dev, A = _to_bf16_dev(h, cuda, c["lda"])
    W_dev, W = _to_bf16_dev((rng.standard_normal((rows_w, K), dtype=np.float32) / np.float32(math.sqrt(K))), cuda)
    bias = rng.standard_normal(rows_w, dtype=np.float32) if c["bias"] else None
    res = None
    if c["res"]:
        res = rng.standard_normal((M, N), dtype=np.float32) + np.float32(c["offset"]) * (1 + rng.standard_normal((M, 1), dtype=np.float32) / 8)
    fold = None
    if c["ln"]:
        st, _, _ = G.slice_stats64(h)
        fold = {"stats": st.astype(np.float32), "colsum": W.astype(np.float64).sum(1).astype(np.float32), "eps": 1e-5}
    return A_dev, A, W_dev, W, bias, res, fold


def _on_device(fn):
    """Run the launching part of a test.  A launch the library refuses (an argument check, no memory) is an ordinary failure of
    that one case.  An error that leaves the device unusable -- the stream no longer synchronises -- ends the session: nothing
    more is started on a device that has faulted."""
    try:
        return fn()
    except torch.OutOfMemoryError:
        raise
    except RuntimeError as e:      # SculptError is one
        try:
            torch.cuda.synchronize()
        except RuntimeError as e2:
            pytest.exit("the device reports an error, session stopped: %s / %s" % (e, e2), returncode=3)
        raise


def _launch(c, ops, cuda, monkeypatch, A_dev, W_dev, bias, res, fold, M, row0=0, rows_per_image=0):
    """One ops.gemm call on rows [row0, row0 + M) into fresh sentinel canvases -> (form, host canvases with the output top-left)."""
    N, outs = c["N"], c["outs"]
    split = c["split"]
    nq = split if split else N
    C0 = 8                                             # the output starts 8 columns into its buffer when ldo > N is asked for
    c0 = C0 if c["ldo"] else 0
    ld = c0 + nq + c["ldo"]
    dev = {}
    if "f" in outs:
        dev["f"] = torch.full((M + 3, ld), float("nan"), device=cuda)
    if "b" in outs:
        dev["b"] = torch.full((M + 3, ld), G.BF16_SENTINEL, dtype=torch.int16, device=cuda).view(BF)
    nt = (N - split if split else N)
    if "t" in outs:
        dev["t"] = torch.full((nt + 3, (M + 63) // 64 * 64 + 8), G.BF16_SENTINEL, dtype=torch.int16, device=cuda).view(BF)
    st_dev = torch.full((N // 64 + 1, M + 5, 2), float("nan"), device=cuda) if c["stats"] else None
    r_dev = None
    if res is not None:
        r = torch.from_numpy(res[row0:row0 + M]).to(cuda)
        if c["res"] == "in":
            dev["f"][:M, c0:c0 + N] = r
            r_dev = dev["f"][:M, c0:c0 + N]
        else:
            r_dev = r.contiguous()
    kw = {}
    if fold is not None:
        kw = dict(ln_stats=torch.from_numpy(np.ascontiguousarray(fold["stats"][:, row0:row0 + M])).to(cuda),
                  ln_colsum=torch.from_numpy(fold["colsum"]).to(cuda), ln_eps=fold["eps"])
    view = lambda k: dev[k][:M, c0:c0 + nq] if k in dev else None
    token = c["token"]
    if token:
        monkeypatch.setenv("SCULPT_GEMM_TILE", token)
    else:
        monkeypatch.delenv("SCULPT_GEMM_TILE", raising=False)
    call = lambda: ops.gemm(A_dev[row0:row0 + M], W_dev, bias=torch.from_numpy(bias).to(cuda) if bias is not None else None,
                            residual=r_dev, out_f32=view("f"), out_bf16=view("b"), out_t=dev["t"][:nt] if "t" in dev else None, M=M,
                            epilogue=c["epi"], n_split=split or 0, stats_out=st_dev, **kw)
    def run():
        if rows_per_image:
            with ops.single_image_tiles(rows_per_image):
                call()
        else:
            call()
        f = ops.gemm_last_form()
        torch.cuda.synchronize()
        return f

    form = _on_device(run)
    host = {}
    roll = lambda a: np.concatenate([a[:, c0:], a[:, :c0]], 1) if c0 else a
    if "f" in dev:
        host["out_f32"] = roll(dev["f"].cpu().numpy())
    if "b" in dev:
        host["out_bf16"] = roll(_bf16_np(dev["b"]))
    if "t" in dev:
        host["out_t"] = _bf16_np(dev["t"])
    if st_dev is not None:
        host["stats_out"] = st_dev.cpu().numpy()
    return form, host


def _assert_form(form, want, c, label):
    got = {k: form.get(k) for k in KEYS}
    assert got == want, "%s: the launcher took %r, the table says %r" % (label, form.get("text"), want)
    for k, v in c["expect"].items():
        assert (form[k] != 0) if v == "nonzero" else (form[k] == v), "%s: %s = %r in %r, expected %r" % (label, k, form[k], form["text"], v)


@pytest.mark.parametrize("name,i", CASES, ids=["%s #%d" % (n.replace(" ", "-"), i) for n, i in CASES])
def test_form_holds_the_bound_on_every_element(cuda, monkeypatch, name, i):
    from sculptmate_amd import ops

    want, token, launches = FORMS[name]
    c = dict(launches[i], epi=want["epi"])
    c["token"] = c["token"] or token
    label = "%s #%d M=%d N=%d K=%d outs=%s%s" % (name, i, c["M"] * c["images"], c["N"], c["K"], c["outs"], " [%s]" % c["token"] if c["token"] else "")
    A_dev, A, W_dev, W, bias, res, fold = _operands(c, 7919 * (sorted(FORMS).index(name) + 1) + i, cuda)
    Mi, B_ = c["M"], c["images"]
    M = Mi * B_
    form, host = _launch(c, ops, cuda, monkeypatch, A_dev, W_dev, bias, res, fold, M, rows_per_image=Mi if B_ > 1 else 0)
    _assert_form(form, want, c, label)
    tile = (want["bm"], 128 if (want["epi"] == GEGLU and want["family"] == "g256") else (64 if want["epi"] == GEGLU else want["bw"]))
    rows = G.edge_rows(M, want["bm"]) if c["subset"] else None
    sel = slice(None) if rows is None else rows
    ln = None if fold is None else dict(fold, stats=fold["stats"][:, sel])
    R = G.reference(A[sel], W, bias, None if res is None else res[sel], c["epi"], ln)
    w = G.check_every_element(R, M, c["N"], n_split=c["split"], tile=tile, rows=rows, label=label, **host)
    assert w["worst"] <= 1.0
    if B_ > 1:
        # the stacked launch against one launch per image: the same form, bit for bit (each is held to the bound through the stack)
        for b in range(B_):
            f1, h1 = _launch(c, ops, cuda, monkeypatch, A_dev, W_dev, bias, res, fold, Mi, row0=b * Mi)
            _assert_form(f1, want, c, label + " image %d" % b)
            for k, a in h1.items():
                s = host[k]
                if k == "out_t":
                    same = np.array_equal(a[:, :Mi], s[:a.shape[0], b * Mi:(b + 1) * Mi][:, :Mi])
                elif k == "stats_out":
                    same = np.array_equal(a[:-1, :Mi], s[:-1, b * Mi:(b + 1) * Mi])
                else:
                    same = np.array_equal(a[:Mi], s[b * Mi:(b + 1) * Mi])
                assert same, "%s: %s of image %d differs between the stacked and the single-image launch" % (label, k, b)


def _im2col_rows(x, n_img, H, W, rows):
    """Rows `rows` of the im2col matrix of channel-last x [n_img * H * W][64] for a 3 x 3, dilation 1, zero-padded convolution,
    K ordered [ky][kx][c]."""
    out = np.zeros((len(rows), 9 * 64), np.float32)
    for r, m in enumerate(rows):
        img, y, xx = m // (H * W), (m // W) % H, m % W
        for t in range(9):
            yy, x2 = y + t // 3 - 1, xx + t % 3 - 1
            if 0 <= yy < H and 0 <= x2 < W:
                out[r, t * 64:(t + 1) * 64] = x[(img * H + yy) * W + x2]
    return out


@pytest.mark.parametrize("name", sorted(CONV_FORMS))
def test_conv_launches_fill_the_record(cuda, name):
    """The implicit 3 x 3 convolution's four launches report themselves (conv=1), and a subset of rows holds the plain bound (the
    network's layers are held by test_gpu_u2net_layers.py)."""
    from sculptmate_amd import _lib, ops

    want, (n_img, H, W, relu) = CONV_FORMS[name]
    M, N = n_img * H * W, 128
    rng = np.random.default_rng(len(name) + M)
    x_dev, x = _to_bf16_dev(rng.standard_normal((M, 64), dtype=np.float32), cuda)
    w_dev, w = _to_bf16_dev(rng.standard_normal((N, 576), dtype=np.float32) / 24, cuda)
    bias = rng.standard_normal(N, dtype=np.float32)
    out = torch.full((M + 3, N + 8), float("nan"), device=cuda)
    b_dev = torch.from_numpy(bias).to(cuda)

    def run():
        _lib.check(_lib.lib.sculpt_conv3x3_bf16(ops._ptr(x_dev), 64, n_img, H, W, 64, 1, ops._ptr(w_dev), ops._ptr(b_dev), ops._ptr(out), None,
                                                N + 8, 0, N, RELU if relu else NONE, ops._stream()))
        f = ops.gemm_last_form()
        torch.cuda.synchronize()
        return f

    form = _on_device(run)
    assert {k: form.get(k) for k in KEYS} == want, (form.get("text"), want)
    rows = G.edge_rows(M, 128, stride=53)
    R = G.reference(_im2col_rows(x, n_img, H, W, rows), w, bias, None, RELU if relu else NONE)
    assert G.check_every_element(R, M, N, out_f32=out.cpu().numpy(), tile=(128, want["bw"]), rows=rows, label=name)["worst"] <= 1.0
