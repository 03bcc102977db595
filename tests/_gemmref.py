"""A plain fp64 restatement of the bf16 GEMM (sculptmate_amd/csrc/gemm.hip: sculpt_gemm_bf16_ln) and a checker that holds EVERY
element of every output of one launch to a bound -- test infrastructure in the manner of tests/_qemref.py and _renderref.py,
written for reading, not for speed.  NumPy on the CPU; torch only for erf in fp64.

The operation.  out[m][n] = epi(pre[m][n]) (+ residual[m][n]),
    plain           pre = sum_k a w + b
    LayerNorm fold  pre = rstd (sum_k a w - mean cs) + b,   rstd = 1 / sqrt(var + eps); mean and var of row m come from the
                    statistics array the kernel itself reads -- (mean, M2) of every 64-column slice, [K/64][rows][2] -- merged here
                    in fp64 by the parallel-variance formula (never from the rows: what the kernel is given is what counts)
    epi             NONE: pre;  GELU: gelu(pre);  RELU: max(pre, 0);  GEGLU: pre_v gelu(pre_g), W holds the N value rows first and
                    the N gate rows second;   gelu(x) = x (1 + erf(x / sqrt 2)) / 2
a, w are the exact values of the bf16 operands; everything here is fp64.

Error scale.  mag = sum_k |a||w| + |b| (fold: rstd (sum_k |a||w| + |mean cs|) + |b|): what an fp32 evaluation's rounding errors
are proportional to, whatever cancels in the sum.

Bounds, element by element (B = 5e-6, the project's figure for fp32 accumulation up to K = 4096 relative to this scale:
test_gemm_three_limb_bf16_is_fp32_equivalent; a blocked fp32 evaluation on the CPU stays below 1e-7 of mag for K = 64 .. 4096,
one dropped 32-wide k-step moves > 99.7 % of the elements by more than B mag -- tests/test_gemmref.py):
  fp32, NONE / RELU    |out - ref| <= B mag (+ B |r| with a residual: |r| joins mag).  max(., 0) has slope <= 1.
  fp32, GELU           |out - ref| <= 1.13 B mag + |pre| E_ERF + 3 u |gelu(pre)|                          (u = 2^-24)
                       1.13 >= max |gelu'| carries the pre-activation's bound through.  gelu = x/2 (1 + erf): an erf that is
                       wrong by at most 2 E_ERF moves it by |x|/2 . 2 E_ERF = |x| E_ERF.  The 2 is room for what the kernel's
                       erf (Abramowitz-Stegun 7.1.26 in fp32) does not share with the NumPy evaluation that E_ERF measures: a
                       hardware reciprocal and exp2 of one ulp each, and the rounded argument x / sqrt 2 (u |x| on the argument,
                       at most 0.3 u |x| on x/2 erf: a twentieth of |x| E_ERF).  3 u |gelu|: the roundings after the erf -- 1 + erf,
                       the product (x/2) (1 + erf) (x/2 itself is exact) and the residual's addition -- each at most u of the
                       result.
  fp32, GEGLU          |out - ref| <= |gelu(pre_g)| B mag_v + |pre_v| dgelu(pre_g) + dv dgelu + u |ref|, dv = B mag_v, dgelu =
                       the GELU bound above at the gate; u |ref|: the rounding of the product v gelu(g).
  E_ERF = 5.5e-7: the largest difference between the textbook formula evaluated in fp32 NumPy (erf_as32) and fp64 erf over
  2 400 001 points of [-6, 6], measured 5.48e-7 (at x = -0.036, where 1 - p t e cancels) -- measure_e_erf(), asserted by
  tests/test_gemmref.py.
  bf16 / transposed bf16, same launch as an fp32 output or as each other: the SAME accumulator is converted (gemm.hip, phase 2 of
                       both epilogues: out_f32, out_bf16 and out_t are all stores of `o`), so: bit-identical to round-to-nearest-
                       even of that launch's fp32 output, and to each other.
  bf16 / transposed bf16 of a launch without an fp32 output for those columns: the value converted lies within the fp32 bound b
                       of ref and rounding to nearest is monotonic, so  rne(ref - b) <= out <= rne(ref + b)  in bf16 order.
                       That is the fp32 bound plus the rounding of ONE bf16 conversion, exactly.  In absolute terms the rounding
                       is half a bf16 ulp = 2^(e - 8) for 2^e <= |x| < 2^(e + 1): between 2^-9 |x| and 2^-8 |x|.  (A flat
                       2^-9 |ref| is NOT a bound of a correct conversion: bf16 keeps 8 significant bits, so just above a power of
                       two half an ulp is 2^-8 |x| -- 1 + 3 . 2^-9 rounds to 1 + 2^-7 or 1, 2^-9 away at best; the stand-in of
                       test_gemmref.py, rounded correctly, misses a 2^-9 |ref| term on a quarter of its elements.  The interval
                       above is never looser than b + 2^-8 |ref| and is the tightest statement of "fp32 bound, then one rounding";
                       DESIGN.md 3.4.)  The normalised error reported for these is |out - ref| / (b + half ulp(|ref| + b)).
  stats_out            (mean, M2) of every 64-column slice of the fp32 output THE KERNEL WROTE, in fp64.  The kernel sums 16
                       values per lane ((a + b) + (c + d) per 4, a chain over <= 4 sub-tiles), two shuffle steps, and for the
                       64-row weight tile one merge of two 32-column halves: <= 8 roundings on any path of the sum, so
                         |mean' - mean| <= dm = 8 u mean|x| + u |mean|                                      (u = 2^-24)
                       M2 sums fl((x - mean')^2) by fma: each term carries <= 3 u, the sum <= 18 (chain 16 + 2 shuffles), and a
                       wrong centre adds 64 dm^2 exactly (sum (x - mean) = 0).  The merge M2a + M2b + 16 (mean_a - mean_b)^2 of the
                       64-row weight tile is first order in the half means' errors: 32 |d| . 2 dm with d the difference of the
                       half means (taken here in fp64 from the data):
                         |M2' - M2| <= 24 u M2 + 64 dm^2 + 64 |d| dm
                       On the rows of the test that used to hold these (|x| ~ 3.3, M2 ~ 64) this is 1.6e-6 and 1.8e-6 M2, inside
                       the 1e-5 asserted there.

Outside the output.  Every output lives in a wider and taller buffer prefilled with a sentinel (NaN for fp32; BF16_SENTINEL, a
signalling-NaN pattern no conversion produces, for bf16): check_every_element asserts that every element of the output was
overwritten and that every element outside still holds the sentinel -- the columns past N or n_split, the rows past M, the V^T
columns past M, the statistics rows past M and planes past N/64.
"""
import collections
import math

import numpy as np

B = 5e-6
U = 2.0 ** -24
E_ERF = 5.5e-7
GELU_SLOPE = 1.13
EPI_NONE, EPI_GELU, EPI_GEGLU, EPI_RELU = 0, 1, 2, 3
BF16_SENTINEL = 0x7FA5
LN_SLOT = 64

Ref = collections.namedtuple("Ref", "pre ref mag bound epilogue")


# ------------------------------------------------------------------------------------------------------------ bf16 bits
def bf16_bits_to_f64(bits):
    """uint16 bf16 patterns -> their exact values in fp64."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_rne_bits(x):
    """Round-to-nearest-even bf16 pattern (uint16) of finite x; x is rounded to fp32 first when it is fp64 -- exact for every
    use below: the fp32 outputs are fp32, and interval ends only need a monotonic rounding (fp64 -> fp32 -> bf16 is one)."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_order_key(bits):
    """int32 keys that order bf16 patterns as their values (-0 just below +0)."""
    b = np.asarray(bits, np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF) - 1, b)


def bf16_half_ulp(x):
    """Half a bf16 ulp at |x| (fp64): 2^(e - 8) for 2^e <= |x| < 2^(e + 1)."""
    ax = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return np.exp2(np.floor(np.log2(ax)) - 8.0)


# ------------------------------------------------------------------------------------------------------------- the maths
def erf64(x):
    import torch

    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def gelu64(x):
    return 0.5 * x * (1.0 + erf64(x / math.sqrt(2.0)))


def erf_as32(x):
    """Abramowitz-Stegun 7.1.26 in fp32 NumPy, in the kernel's order of operations (gemm.hip erf_as)."""
    f = np.float32
    x = np.asarray(x, np.float32)
    ax = np.abs(x)
    t = (f(1) / (f(0.3275911) * ax + f(1))).astype(np.float32)
    p = f(1.061405429) * t + f(-1.453152027)
    p = p * t + f(1.421413741)
    p = p * t + f(-0.284496736)
    p = p * t + f(0.254829592)
    e = np.exp2(f(-1.44269504088896340736) * ax * ax).astype(np.float32)
    return np.copysign(f(1) - p * t * e, x).astype(np.float32)


def gelu_as32(x):
    f = np.float32
    x = np.asarray(x, np.float32)
    return (f(0.5) * x * (f(1) + erf_as32(x * f(0.70710678118654752440)))).astype(np.float32)


def measure_e_erf(points=2_400_001):
    """The largest |erf_as32 - erf| over a dense fp32 grid of [-6, 6] and where."""
    x = np.linspace(-6.0, 6.0, points).astype(np.float32)
    d = np.abs(erf_as32(x).astype(np.float64) - erf64(x.astype(np.float64)))
    return float(d.max()), float(x[d.argmax()])


def merge_slice_stats(stats, rows):
    """stats [slots][>= rows][2] (mean, M2 of 64-column slices) -> (mean, var) of the whole rows, fp64, parallel-variance formula."""
    s = np.asarray(stats, np.float64)[:, :rows]
    mean = s[..., 0].mean(0)
    m2 = (s[..., 1] + LN_SLOT * (s[..., 0] - mean[None, :]) ** 2).sum(0)
    return mean, m2 / (LN_SLOT * s.shape[0])


def slice_stats64(x):
    """fp64 (mean, M2) of every 64-column slice of x [rows][cols] -> [cols/64][rows][2], and |d| of the two half means."""
    x = np.asarray(x, np.float64)
    sl = x.reshape(x.shape[0], -1, LN_SLOT)
    mean = sl.mean(-1)
    m2 = ((sl - mean[..., None]) ** 2).sum(-1)
    d = np.abs(sl[..., :32].mean(-1) - sl[..., 32:].mean(-1))
    return np.stack([mean.T, m2.T], -1), d.T, np.abs(sl).mean(-1).T


def reference(A, W, bias, residual, epilogue, ln=None):
    """A [M][K], W [N or 2N][K]: the exact bf16 operand values (any float dtype); bias [N or 2N] / residual [M][N] fp32 or None;
    ln: None or dict(stats=[K/64][>= M][2], colsum=[N or 2N], eps).  -> Ref(pre, ref, mag, bound, epilogue): fp64 arrays; pre / mag
    have 2N columns for GEGLU (value half first); bound is the per-element bound of the fp32 output (module docstring)."""
    A = np.asarray(A, np.float64)
    W = np.asarray(W, np.float64)
    M = A.shape[0]
    acc = A @ W.T
    mag = np.abs(A) @ np.abs(W).T
    b = np.zeros(W.shape[0]) if bias is None else np.asarray(bias, np.float64)
    if ln is not None:
        mean, var = merge_slice_stats(ln["stats"], M)
        rstd = 1.0 / np.sqrt(var + float(ln["eps"]))
        cs = np.asarray(ln["colsum"], np.float64)
        pre = rstd[:, None] * (acc - mean[:, None] * cs[None, :]) + b[None, :]
        mag = rstd[:, None] * (mag + np.abs(mean[:, None] * cs[None, :])) + np.abs(b)[None, :]
    else:
        pre = acc + b[None, :]
        mag = mag + np.abs(b)[None, :]

    def gelu_bound(p, m):
        return GELU_SLOPE * B * m + np.abs(p) * E_ERF + 3.0 * U * np.abs(gelu64(p))

    if epilogue == EPI_NONE:
        ref, bound = pre, B * mag
    elif epilogue == EPI_RELU:
        ref, bound = np.maximum(pre, 0.0), B * mag
    elif epilogue == EPI_GELU:
        ref, bound = gelu64(pre), gelu_bound(pre, mag)
    elif epilogue == EPI_GEGLU:
        N = W.shape[0] // 2
        pv, pg, gg = pre[:, :N], pre[:, N:], gelu64(pre[:, N:])
        dv, dg = B * mag[:, :N], gelu_bound(pg, mag[:, N:])
        ref = pv * gg
        bound = np.abs(gg) * dv + np.abs(pv) * dg + dv * dg + U * np.abs(ref)
    else:
        raise ValueError("unknown epilogue %r" % (epilogue,))
    if residual is not None:
        r = np.asarray(residual, np.float64)
        ref = ref + r
        bound = bound + B * np.abs(r)
        if epilogue in (EPI_NONE, EPI_RELU):
            mag = mag + np.abs(r)
    return Ref(pre, ref, mag, bound, epilogue)


# --------------------------------------------------------------------------------------------------------- the buffers
def canvas(kind, rows, cols, pad_rows=3, pad_cols=8, lead=None):
    """A sentinel-filled host buffer of rows + pad_rows by (lead or cols + pad_cols): float32 NaN ("f32") or uint16
    BF16_SENTINEL ("bf16").  The output is its top-left rows x cols corner."""
    shape = (rows + pad_rows, lead if lead is not None else cols + pad_cols)
    if kind == "f32":
        return np.full(shape, np.nan, np.float32)
    return np.full(shape, BF16_SENTINEL, np.uint16)


def _untouched(buf):
    return np.isnan(buf) if buf.dtype == np.float32 else buf == BF16_SENTINEL


def _check_region(name, buf, rows, cols):
    """Every element of buf[:rows, :cols] overwritten, every other one still the sentinel."""
    un = _untouched(buf)
    inside = un[:rows, :cols]
    assert not inside.any(), "%s: %d element(s) of the output were never written (or hold a NaN), first at %s" % (
        name, int(inside.sum()), tuple(int(v) for v in np.argwhere(inside)[0]))
    outside = ~un
    outside[:rows, :cols] = False
    assert not outside.any(), "%s: %d element(s) OUTSIDE the %d x %d output were written, first at %s" % (
        name, int(outside.sum()), rows, cols, tuple(int(v) for v in np.argwhere(outside)[0]))


def _where(idx, tile, rows=None):
    m, n = int(idx[0]), int(idx[1])
    if rows is not None:
        m = int(rows[m])
    bm, bn = tile
    return {"row": m, "col": n, "tile": (m // bm, n // bn), "in_tile": (m % bm, n % bn)}


def check_every_element(R, M, N, out_f32=None, out_bf16=None, out_t=None, stats_out=None, n_split=None, tile=(128, 128), rows=None,
                        label=""):
    """Hold one launch's outputs to the module's bounds, element by element.
      R          reference(...) of the launch (or of its rows `rows`, an index array: the deep launches whose fp64 reference would
                 be too large are referenced on a subset of rows -- tile edges and a stride; the sentinel checks and the bit
                 identities still cover every element)
      out_f32 / out_bf16   canvases whose top-left M x (n_split or N) corner is the token-major output
      out_t      bf16 canvas, output = its top-left (N - n_split or N) x M corner: the transposed result (of the columns >= n_split)
      stats_out  float32 [N/64 + pad][>= M + pad][2] prefilled with NaN
      tile       (activation rows, output columns) per workgroup, for the report only
    Returns {"worst": largest error / bound, "where": row, col, tile, in_tile, "output": name}; raises AssertionError."""
    split = n_split is not None and 0 < n_split < N
    nq = n_split if split else N
    ref, bound = R.ref, R.bound
    assert ref.shape == ((M if rows is None else len(rows)), N)
    sel = slice(None) if rows is None else np.asarray(rows)
    worst = {"worst": 0.0, "where": None, "output": None}

    def note(name, err, idx, off=0):
        if err > worst["worst"]:
            w = _where((idx[0], idx[1] + off), tile, rows)
            worst.update(worst=float(err), where=w, output=name)

    def fail(name, what, idx, off=0, extra=""):
        raise AssertionError("%s %s: %s at %s %s" % (label, name, what, _where((idx[0], idx[1] + off), tile, rows), extra))

    def interval(name, bits, r, b, off=0):
        # rne(ref - b) <= out <= rne(ref + b) in bf16 order
        lo, hi, k = bf16_order_key(bf16_rne_bits(r - b)), bf16_order_key(bf16_rne_bits(r + b)), bf16_order_key(bits)
        v = bf16_bits_to_f64(bits)
        nerr = np.abs(v - r) / (b + bf16_half_ulp(np.abs(r) + b))
        i = np.unravel_index(np.argmax(nerr), nerr.shape)
        note(name, nerr[i], i, off)
        bad = (k < lo) | (k > hi)
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            fail(name, "%d element(s) outside rne(ref -+ bound); first: got %.9g, ref %.9g, bound %.3g" % (
                int(bad.sum()), v[i], r[i], b[i]), i, off)

    f32 = None
    if out_f32 is not None:
        _check_region(label + " out_f32", out_f32, M, nq)
        f32 = out_f32[:M, :nq]
        err = np.abs(f32[sel].astype(np.float64) - ref[:, :nq]) / bound[:, :nq]
        i = np.unravel_index(np.argmax(err), err.shape)
        note("out_f32", err[i], i)
        if err[i] > 1.0:
            fail("out_f32", "%d element(s) over the bound; worst %.3f x bound: got %.9g, ref %.9g, bound %.3g" % (
                int((err > 1.0).sum()), err[i], f32[sel][i], ref[i], bound[i]), i)
    b16 = None
    if out_bf16 is not None:
        _check_region(label + " out_bf16", out_bf16, M, nq)
        b16 = out_bf16[:M, :nq]
        if f32 is not None:
            bad = b16 != bf16_rne_bits(f32)
            if bad.any():
                i = tuple(np.argwhere(bad)[0])
                raise AssertionError("%s out_bf16: %d element(s) are not round-to-nearest-even of this launch's fp32 output, first at %s: "
                                     "0x%04x for %.9g" % (label, int(bad.sum()), _where(i, tile), int(b16[i]), f32[i]))
        else:
            interval("out_bf16", b16[sel], ref[:, :nq], bound[:, :nq])
    if out_t is not None:
        nt = N - n_split if split else N
        _check_region(label + " out_t", out_t, nt, M)
        t = out_t[:nt, :M].T     # [M][nt]
        if not split and (f32 is not None or b16 is not None):
            want = bf16_rne_bits(f32) if f32 is not None else b16
            bad = t != want
            if bad.any():
                i = tuple(np.argwhere(bad)[0])
                raise AssertionError("%s out_t: %d element(s) differ from the token-major output of the same launch, first at %s" % (
                    label, int(bad.sum()), _where(i, tile)))
        else:
            c0 = n_split if split else 0
            interval("out_t", t[sel], ref[:, c0:], bound[:, c0:], off=c0)
    if stats_out is not None:
        assert f32 is not None and not split
        ns = N // LN_SLOT
        un = np.isnan(stats_out)
        assert not un[:ns, :M].any(), "%s stats_out: statistics of the output never written, first at %s" % (
            label, tuple(int(v) for v in np.argwhere(un[:ns, :M])[0]))
        outside = ~un
        outside[:ns, :M] = False
        assert not outside.any(), "%s stats_out: written outside [N/64][M], first at %s" % (
            label, tuple(int(v) for v in np.argwhere(outside)[0]))
        want, d, mabs = slice_stats64(f32)
        got = stats_out[:ns, :M].astype(np.float64)
        dm = 8.0 * U * mabs + U * np.abs(want[..., 0])
        dq = 24.0 * U * want[..., 1] + 64.0 * dm * dm + 64.0 * d * dm
        for name, e in (("stats_out.mean", np.abs(got[..., 0] - want[..., 0]) / dm), ("stats_out.M2", np.abs(got[..., 1] - want[..., 1]) / dq)):
            i = np.unravel_index(np.argmax(e), e.shape)     # (slice, row)
            if e[i] > worst["worst"]:
                worst.update(worst=float(e[i]), where=_where((i[1], i[0] * LN_SLOT), tile), output=name)
            assert e[i] <= 1.0, "%s %s: %.3f x bound at row %d, slice %d (%d over)" % (label, name, e[i], i[1], i[0], int((e > 1.0).sum()))
    print("%s: largest normalised error %.4f in %s at %s" % (label, worst["worst"], worst["output"], worst["where"]))
    return worst


def edge_rows(M, bm, stride=37):
    """Rows for a subset reference: the first and last rows of every activation tile edge that exists, plus a stride."""
    r = set(range(0, M, stride)) | {0, M - 1}
    for e in range(bm, M, bm):
        r |= {e - 1, e}
    return np.array(sorted(r))
