"""Every kernel the bf16 attention launcher can start (csrc/attention.hip: attention_launch), reached on purpose and held, element by
element, to the fp64 bound of tests/_attnref.py.

FORMS is the table: one row per instantiation -- its fields as sculpt_attention_last_form reports them, the SCULPT_ATTN_FORM token
that forces it, and its launches.  Every launch asserts ops.attention_last_form() against its row BEFORE any number is looked at,
so a changed cost rule or another CU count fails here instead of quietly moving a shape to another kernel.  A launch with
token=None goes through the default rule (default_nqb below restates it for 256 CUs); UNREACHABLE_BY_DEFAULT lists the forms no
shape reaches that way -- they run under their token only.  tests/test_attention_ref_host.py (no device needed) counts the launch
sites in the source against the table and audits what every row runs.

Shapes: 2 heads; Tq in {1, 32n - 1, 32n, 32n + 1, 64n + 1} for n = nqb (a last block of one row, the block edge itself); every Tk of
TKS in every row (the look-ahead tile pair missing, ragged, of the other key half only, complete), spread over the Tq values; one
deep launch per row.  Launch kinds (KINDS), every row runs each (the threshold kind exists for pre-scaled queries only):
  random     Q and K column slices of wider tensors, ldo > heads * 64, V^T padding columns of 7.0, O inside a NaN-patterned canvas
             that must come back untouched outside the Tq x heads*64 block
  rescale    spikes of hundreds of log2 units at the first and last key of each 64-key half of tile pairs 0, 1, 2 and of the last
             pair (the ragged tail included), rising from one to the next, so consecutive pairs jump; a first tile that is
             hugely negative for some queries; tiles whose p all underflow to 0
  threshold  scores on one coordinate: a 32-query block whose maximum rises by 9.5 between tile pairs (no rescale: PRE_THR = 10),
             another that sees 10.5
  census     K = 0 and an indicator V: O[i][d] = count_d / Tk, one key lost, doubled or misplaced moves an element by at least
             64 / (Tk + 64) of its value
  batch      three entries stacked at a row stride that is a multiple of 8 and not of 64, V^T side by side and one array per entry;
             bit-equal to the single launches of the same form
"""
import numpy as np
import pytest
import torch

import _attnref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HEADS = 2
SCALE = 0.125
TKS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 384, 385)
KINDS = ("random", "rescale", "threshold", "census", "batch")
KEYS = ("kernel", "nqb", "pre")
CUS = 256


def default_nqb(Tq, heads, batch, pre, cus=CUS):
    """The launcher's cost rule (attention_launch), restated: queries per workgroup / 32 that a launch takes without a token."""
    cdiv = lambda a, b: -(-a // b)
    bh = heads * batch
    nqb, best = 8, cdiv(cdiv(Tq, 256) * bh, cus) * 8 * 100
    for c in (6, 4):
        cost = cdiv(cdiv(Tq, 32 * c) * bh, cus) * c * (98 if pre else 115)
        if cost < best:
            best, nqb = cost, c
    return nqb


def tqs(n):
    return (1, 32 * n - 1, 32 * n, 32 * n + 1, 64 * n + 1)


def L(kind, Tq, Tk, **kw):
    """One launch.  token: "row" (the row's forcing token) or None (the default rule on 256 CUs); heads / batch: of the default-rule
    launches; vt: "side" / "each" (batch: V^T side by side or one array per entry); census: 0 (j % 64 == d) or 1 ((j // 64) % 64 == d)."""
    d = dict(kind=kind, Tq=Tq, Tk=Tk, token="row", heads=HEADS, batch=1, vt="side", census=0)
    d.update(kw)
    return d


def row_launches(n, pre, deep, default):
    t = tqs(n)
    out = [L("random", t[i % 5], Tk) for i, Tk in enumerate(TKS)] + [L("random", t[3], deep)]
    out += [L("rescale", t[3], 449), L("rescale", t[4], 385), L("rescale", t[1], 640)]
    if pre:
        out += [L("threshold", t[4], 385), L("threshold", t[3], 256)]
    out += [L("census", t[3], 385, census=0), L("census", t[1], 449, census=1)]
    out += [L("batch", t[3], 129, batch=3, vt="side"), L("batch", t[1], 65, batch=3, vt="each")]
    out += [L("random", Tq, 65, token=None, heads=h, batch=b) for Tq, h, b in default]
    return out


def F(kernel, nqb, pre):
    return {"kernel": kernel, "nqb": nqb, "pre": pre}


# The default rule on 256 CUs (cost = rounds of workgroups x queries per workgroup / 32; 128 or 192 queries must beat 256 by 15 %,
# 2 % with pre-scaled queries):
#   a small shape (fewer workgroups than CUs in every form): 4 -- one round each, 4 < 6 < 8
#   Tq = 384, 16 heads x 8 entries: 256 workgroups of 192 queries (one round, 6) against 384 of 128 (two rounds, 8) and 256 of 256 (8): 6
#   Tq = 256, 16 heads x 16 entries, not pre-scaled: 256 workgroups of 256 (8 = 800) against 512 of 128 (two rounds, 8 x 115 = 920): 8;
#   pre-scaled the same shape takes 4 (8 x 98 = 784 < 800)
SMALL, SIX, EIGHT = (129, HEADS, 1), (384, 16, 8), (256, 16, 16)
FORMS = {
    "plain nqb=4 pre=0": (F("plain", 4, 0), "nqb=4", row_launches(4, False, 1025, [SMALL])),
    "plain nqb=6 pre=0": (F("plain", 6, 0), "nqb=6", row_launches(6, False, 1025, [SIX])),
    "plain nqb=8 pre=0": (F("plain", 8, 0), "nqb=8", row_launches(8, False, 3089, [EIGHT])),
    "plain nqb=4 pre=1": (F("plain", 4, 1), "nqb=4,nopipe", row_launches(4, True, 1025, [])),
    "plain nqb=6 pre=1": (F("plain", 6, 1), "nqb=6,nopipe", row_launches(6, True, 1025, [])),
    "plain nqb=8 pre=1": (F("plain", 8, 1), "nqb=8", row_launches(8, True, 3089, [])),
    "pipe nqb=4 pre=1": (F("pipe", 4, 1), "nqb=4", row_launches(4, True, 1025, [SMALL])),
    "pipe nqb=6 pre=1": (F("pipe", 6, 1), "nqb=6", row_launches(6, True, 3089, [SIX])),
}
# Forms no shape reaches through the default rule, on any CU count: the phase-separated loop runs pre-scaled queries only under
# `nopipe` or at 256 queries, and a pre-scaled launch never takes 256 -- 128-query workgroups are at most twice as many, so
# cost(4) <= cost(8) always, and cost(4) x 98 < cost(8) x 100 (tests/test_attention_ref_host.py searches the rule for a counterexample)
UNREACHABLE_BY_DEFAULT = {
    ("plain", 4, 1): "pre-scaled queries at 128 queries run the pipelined kernel unless `nopipe` is set",
    ("plain", 6, 1): "pre-scaled queries at 192 queries run the pipelined kernel unless `nopipe` is set",
    ("plain", 8, 1): "cost(4) x 98 < cost(8) x 100 whenever cost(4) <= cost(8), which always holds",
}

CASES = [(name, kind) for name, (f, _, launches) in FORMS.items() for kind in KINDS if any(c["kind"] == kind for c in launches)]


# ------------------------------------------------------------------------------------------------------------ operands
def _pre_factor(pre):
    """Raw score -> the exponent's (log2) units."""
    return 1.0 if pre else SCALE * R.LOG2E


def _random(rng, c, pre):
    return R.operands(rng, c["Tq"], c["Tk"], c["heads"], None if pre else SCALE)


def spike_keys(Tk):
    """The first and last key of each 64-key half of tile pairs 0, 1, 2 and of the last pair, as far as they exist."""
    last = (Tk - 1) // 128
    keys = set()
    for tp in sorted({0, 1, 2, last}):
        for half in (0, 1):
            k0 = 128 * tp + 64 * half
            if k0 < Tk:
                keys |= {k0, min(k0 + 63, Tk - 1)}
    return sorted(keys)


def _rescale(rng, c, pre):
    """Coordinate 1 of every head carries the spikes: q_i[1] = a_i, k_j[1] = height_j / (2 f), so a query with a = 2 sees key j
    at height_j log2 units: 100 for the whole first tile (keys 0 .. 63), then 250, 400, ... at the spike keys in key order (every
    later spike above all before it: a rescale at each, in consecutive tile pairs); everything after a spike underflows to 0 until
    the next one.  a = -2: the first tile is hugely negative and the spikes never count; a = 0.5: spikes of 25 .. and no
    underflow of whole tiles at first; a = 0 and 2^-7: ordinary rows."""
    q, k, v = _random(rng, c, pre)
    f = _pre_factor(pre)
    a = np.array([2.0, -2.0, 0.5, 0.0, 2.0 ** -7, 2.0, -2.0], np.float32)
    height = np.zeros(c["Tk"], np.float32)
    height[:64] = 100.0
    for i, j in enumerate(spike_keys(c["Tk"])):
        height[j] = 250.0 + 150.0 * i
    for h in range(c["heads"]):
        q[:, 64 * h + 1] = a[np.arange(c["Tq"]) % len(a)]
        k[:, 64 * h + 1] = R.bf16_round(height / np.float32(2.0 * f))
    return q, k, v


def _threshold(rng, c, pre):
    """Scores on coordinate 0: q_i = a_i e_0, k_j = b_j e_0 (+ noise of ~0.02 log2 units on the others).  b = 0 in tile pair 0, 1 at
    four keys of each half of tile pair 1, 0 after.  a = 9.5 in the even 32-query blocks -- their maximum rises by 9.5 (+- noise)
    between the pairs, under PRE_THR = 10: no rescale, p up to 2^9.5 -- and 10.5 in the odd ones: a rescale.  Both exact in bf16."""
    assert pre
    Tq, Tk, D = c["Tq"], c["Tk"], c["heads"] * 64
    q = R.bf16_round(rng.standard_normal((Tq, D), dtype=np.float32) * np.float32(0.0025))
    k = R.bf16_round(rng.standard_normal((Tk, D), dtype=np.float32))
    v = R.bf16_round(rng.standard_normal((Tk, D), dtype=np.float32))
    a = np.where((np.arange(Tq) // 32) % 2 == 0, 9.5, 10.5).astype(np.float32)
    b = np.zeros(Tk, np.float32)
    b[[128, 131, 160, 191, 192, 200, 254, 255]] = 1.0
    for h in range(c["heads"]):
        q[:, 64 * h] = a
        k[:, 64 * h] = b
    # the construction itself, in fp64: per 32-query block and key half, the rise of the tile maximum from pair 0 to pair 1
    for h in range(c["heads"]):
        x = q[:, 64 * h:64 * h + 64].astype(np.float64) @ k[:, 64 * h:64 * h + 64].astype(np.float64).T
        for half in (0, 1):
            rise = x[:, 128 + 64 * half:192 + 64 * half].max(1) - x[:, 64 * half:64 + 64 * half].max(1)
            assert (np.abs(rise - a) < 0.4).all(), "the noise moved a rise across the threshold"
    return q, k, v


def _census(rng, c, pre):
    Tq, Tk, D = c["Tq"], c["Tk"], c["heads"] * 64
    q, _, _ = _random(rng, c, pre)
    k = np.zeros((Tk, D), np.float32)
    j = np.arange(Tk)
    col = (j // 64) % 64 if c["census"] else j % 64
    v = np.zeros((Tk, D), np.float32)
    for h in range(c["heads"]):
        v[j, 64 * h + col] = 1.0
    return q, k, v


MAKE = {"random": _random, "rescale": _rescale, "threshold": _threshold, "census": _census, "batch": _random}


# ------------------------------------------------------------------------------------------------------------- launches
def _on_device(fn):
    """Run the launching part of a test.  A launch the library refuses is an ordinary failure of that one case.  An error that
    leaves the device unusable -- the stream no longer synchronises -- ends the session: nothing more is started on a device
    that has faulted."""
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


def _bf(x32):
    return torch.from_numpy(np.ascontiguousarray(x32)).to(BF)


def _entry_stride(n):
    """Rows from one batch entry to the next: at least 8 more than n, a multiple of 8 and not of 64."""
    n = (n + 7) // 8 * 8 + 8
    return n + 8 if n % 64 == 0 else n


class Placed:
    """The operands of `batch` entries on the device, in the layouts the launcher has no other test for:
      Q, K     rows of the entries stacked at a row stride that is a multiple of 8 and not of 64 (pad rows of 3.0 between), each a
               column slice [8, 8 + D) of a tensor 24 columns wider (16-byte aligned start, ldq = ldk = D + 24)
      V^T      padding columns (past Tk, and between the entries) of 7.0; "side": one [D][ldvt] array, entry b at column
               b * vt_bs, vt_bs = round_up(Tk, 64) + 8 (a single entry: ldvt = round_up(Tk, 64), 8 more when Tk is odd); "each": one
               [D + 1][ldvt] array per entry, ldvt = round_up(Tk, 64) + 8
      O        a canvas of the NaN pattern BF16_SENTINEL, [rows + 3][4 + D + 8], the output at columns [4, 4 + D) (8-byte aligned
               start, ldo = D + 12)"""

    def __init__(self, cuda, qs, ks, vs, vt_mode):
        B, (Tq, D), Tk = len(qs), qs[0].shape, ks[0].shape[0]
        self.B, self.Tq, self.Tk, self.D = B, Tq, Tk, D
        self.rq = _entry_stride(Tq) if B > 1 else Tq
        self.rk = _entry_stride(Tk) if B > 1 else Tk
        qb = torch.full((self.rq * (B - 1) + Tq, D + 24), 3.0, dtype=BF)
        kb = torch.full((self.rk * (B - 1) + Tk, D + 24), 3.0, dtype=BF)
        tk64 = (Tk + 63) // 64 * 64
        if vt_mode == "side":
            self.vt_bs = tk64 + 8 if B > 1 else 0
            vt = torch.full((D, self.vt_bs * (B - 1) + tk64 + (8 if B == 1 and Tk % 2 else 0)), 7.0, dtype=BF)
        else:
            vt = torch.full((B, D + 1, tk64 + 8), 7.0, dtype=BF)
            self.vt_bs = vt.stride(0)
        for b in range(B):
            qb[b * self.rq:b * self.rq + Tq, 8:8 + D] = _bf(qs[b])
            kb[b * self.rk:b * self.rk + Tk, 8:8 + D] = _bf(ks[b])
            if vt_mode == "side":
                vt[:, b * self.vt_bs:b * self.vt_bs + Tk] = _bf(vs[b]).t()
            else:
                vt[b, :D, :Tk] = _bf(vs[b]).t()
        self.qb, self.kb, self.vt = qb.to(cuda), kb.to(cuda), vt.to(cuda)
        self.vt_mode = vt_mode
        self.o_rows = self.rq * (B - 1) + Tq
        self.cuda = cuda

    def canvas(self):
        return torch.full((self.o_rows + 3, 4 + self.D + 8), R.BF16_SENTINEL, dtype=torch.int16, device=self.cuda).view(BF)

    def launch(self, ops, heads, scale, entry=None):
        """All entries in one launch (entry None) or entry `entry` alone -> (form, host canvas as uint16 patterns)."""
        Tq, Tk, D = self.Tq, self.Tk, self.D
        o = self.canvas()
        Q, K, O = self.qb[:, 8:8 + D], self.kb[:, 8:8 + D], o[:, 4:4 + D]

        def run():
            if entry is None and self.B > 1:
                Vt = self.vt if self.vt_mode == "side" else self.vt[0]
                ops.attention(Q, K, Vt, O, Tq, Tk, heads, scale, batch=self.B, q_bs=self.rq * Q.stride(0), k_bs=self.rk * K.stride(0),
                              vt_bs=self.vt_bs, o_bs=self.rq * O.stride(0))
            else:
                b = entry or 0
                if self.B == 1:
                    Vt = self.vt
                elif self.vt_mode == "side":     # an array of its own: a single launch may read all ldvt columns of a row
                    Vt = self.vt[:, b * self.vt_bs:b * self.vt_bs + (Tk + 63) // 64 * 64].contiguous()
                else:
                    Vt = self.vt[b]
                ops.attention(Q[b * self.rq:], K[b * self.rk:], Vt, O[b * self.rq:], Tq, Tk, heads, scale)
            f = ops.attention_last_form()
            torch.cuda.synchronize()
            return f

        form = _on_device(run)
        return form, o.view(torch.int16).cpu().numpy().view(np.uint16)

    def split(self, host, entries=None):
        """The host canvas -> ([the Tq x D output of each entry as fp64], the canvas with those blocks cut out)."""
        outside = host.copy()
        outs = []
        for b in (range(self.B) if entries is None else entries):
            r0 = b * self.rq
            outs.append(R.bf16_bits_to_f64(host[r0:r0 + self.Tq, 4:4 + self.D]))
            outside[r0:r0 + self.Tq, 4:4 + self.D] = R.BF16_SENTINEL
        return outs, outside


def _assert_form(form, want, batch, Tq, heads, label):
    got = {k: form.get(k) for k in KEYS}
    assert got == want, "%s: the launcher took %r, the table says %r" % (label, form.get("text"), want)
    grid = (-(-Tq // (32 * want["nqb"])), heads * batch)
    assert form["batch"] == batch and form["grid"] == grid, "%s: %r, expected batch=%d grid=%dx%d" % (label, form["text"], batch, *grid)


def _set_token(monkeypatch, token):
    if token:
        monkeypatch.setenv("SCULPT_ATTN_FORM", token)     # read per call
    else:
        monkeypatch.delenv("SCULPT_ATTN_FORM", raising=False)


@pytest.mark.parametrize("name,kind", CASES, ids=["%s %s" % (n.replace(" ", "-"), k) for n, k in CASES])
def test_form_holds_the_bound_on_every_element(cuda, monkeypatch, name, kind):
    from sculptmate_amd import ops

    want, row_token, launches = FORMS[name]
    pre = bool(want["pre"])
    scale = None if pre else SCALE
    top = 0.0
    for i, c in enumerate(launches):
        if c["kind"] != kind:
            continue
        token = row_token if c["token"] == "row" else None
        label = "%s #%d %s Tq=%d Tk=%d heads=%d batch=%d%s" % (name, i, kind, c["Tq"], c["Tk"], c["heads"], c["batch"], " [%s]" % token if token else "")
        rng = np.random.default_rng(7919 * (sorted(FORMS).index(name) + 1) + i)
        B = c["batch"]
        ent = [MAKE[kind](rng, c, pre) for _ in range(B)]
        P = Placed(cuda, [e[0] for e in ent], [e[1] for e in ent], [e[2] for e in ent], c["vt"])
        _set_token(monkeypatch, token)
        form, host = P.launch(ops, c["heads"], scale)
        _assert_form(form, want, B, c["Tq"], c["heads"], label)
        outs, outside = P.split(host)
        assert (outside == R.BF16_SENTINEL).all(), "%s: %d element(s) outside the output were written, first at %s" % (
            label, int((outside != R.BF16_SENTINEL).sum()), tuple(int(v) for v in np.argwhere(outside != R.BF16_SENTINEL)[0]))
        for b, (got, (q, k, v)) in enumerate(zip(outs, ent)):
            ref = R.reference(q, k, v, c["heads"], scale)
            w, _, text = R.worst(got, ref, want["nqb"], label + (" entry %d" % b if B > 1 else ""))
            print(text)
            top = max(top, w)
            assert w <= 1.0, text
        if kind == "batch":
            # the same entries one launch each: the same kernel, bit for bit
            for b in range(B):
                f1, h1 = P.launch(ops, c["heads"], scale, entry=b)
                _assert_form(f1, want, 1, c["Tq"], c["heads"], label + " entry %d alone" % b)
                r0 = b * P.rq
                assert np.array_equal(h1[r0:r0 + P.Tq, 4:4 + P.D], host[r0:r0 + P.Tq, 4:4 + P.D]), "%s: entry %d differs between the batched and the single launch" % (label, b)
                assert (P.split(h1, [b])[1] == R.BF16_SENTINEL).all(), "%s: entry %d alone wrote outside its output" % (label, b)
    print("%s %s: largest error / B of the row's %s launches %.4f" % (name, kind, kind, top))


def test_refused_shapes_come_back_as_errors(cuda, monkeypatch):
    """What the launcher refuses -- a misaligned row stride, ldvt below round_up(Tk, 64), a V^T batch stride that is neither a column
    offset inside ldvt nor a whole array, extents past the 2 GiB buffer range -- is an error return, and nothing is launched: the
    last form stays what it was."""
    from sculptmate_amd import _lib, ops

    _set_token(monkeypatch, None)
    D = HEADS * 64
    q = torch.zeros(8, D + 8, dtype=BF, device=cuda)
    vt = torch.zeros(D, 64, dtype=BF, device=cuda)
    o = torch.zeros(8, D, dtype=BF, device=cuda)
    ops.attention(q[:, :D], q[:, :D], vt, o, 8, 8, HEADS, SCALE)
    torch.cuda.synchronize()
    before = ops.attention_last_form()
    assert before["kernel"] == "plain" and before["grid"] == (1, HEADS)
    with pytest.raises(_lib.SculptError, match="16-byte"):
        ops.attention(torch.zeros(8, D + 4, dtype=BF, device=cuda)[:, :D], q[:, :D], vt, o, 8, 8, HEADS, SCALE)
    with pytest.raises(_lib.SculptError, match="ldvt"):
        ops.attention(q[:, :D], q[:, :D], vt, o, 8, 65, HEADS, SCALE)
    with pytest.raises(_lib.SculptError, match="V\\^T batch stride"):
        ops.attention(q[:, :D], q[:, :D], vt, o, 2, 2, HEADS, SCALE, batch=2, q_bs=2 * (D + 8), k_bs=2 * (D + 8), vt_bs=32, o_bs=2 * D)
    with pytest.raises(_lib.SculptError, match="2 GiB"):
        # a K row stride of 2^23 elements x 128 rows x 2 B = 2 GiB: refused from the numbers alone, nothing is read
        _lib.check(_lib.lib.sculpt_attention_bf16(ops._ptr(q), D + 8, ops._ptr(q), 1 << 23, ops._ptr(vt), 64, ops._ptr(o), D, 8, 8, HEADS,
                                                  SCALE, ops._stream()))
    torch.cuda.synchronize()
    assert ops.attention_last_form() == before
