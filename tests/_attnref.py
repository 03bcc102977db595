"""A plain fp64 restatement of the bf16 attention (sculptmate_amd/csrc/attention.hip, attention_pipe.hip), a bound for every element
of its output, and an fp32 / bf16 emulation of the kernels' arithmetic that the bound is tried on without a device
(tests/test_attention_ref_host.py) -- test infrastructure in the manner of tests/_gemmref.py, written for reading, not for speed.
NumPy on the CPU.

The operation, per head (64 columns of Q, K, V), from the exact values of the bf16 operands:
    x_ij = q_i . k_j                       pre-scaled entry: the queries carry softmax_scale * log2(e); x is in log2 units
    x_ij = q_i . k_j * scale * log2(e)     the other entry (e^(s scale) = 2^(s scale log2 e)): the same units
    p = softmax_2(x) = 2^(x - max) / sum,   ref = p v,   A = p |v|,   S_id = sum_j p_ij |v_jd - ref_id|

The bound, per element, derived from the kernels' arithmetic (u = 2^-8):
    B = u A + u |ref| + c_acc A + c_exp S
  u A        the probabilities enter the second product rounded to bf16 ((__bf16)p: to nearest even, relative error <= 2^-8),
             while the row sum l is taken from the unrounded fp32 p: sum_j d_j p_j v_j / l with |d_j| <= u.
  u |ref|    the bf16 rounding of O.
  c_acc A    c_acc = (Tk + 64) 2^-24: the fp32 accumulation of P.V and of l over Tk keys (a relative error of l moves O by that
             much of |ref| <= A), the merge of the two key halves and 1 / l.
  c_exp S    c_exp = 2 ln2 . 70 . 2^-24 . max_j sum_c |q_ic k_jc| (the sum in the exponent's units): the fp32 accumulation of
             the 64 + 2 score terms (the pre-scaled kernels add -M_hi - M_lo, |M| <= max_j |x_ij|, inside the product: the 2),
             the fp32 rounding of m_new - m_run (pre-scaled) or of the v_pk_fma (scaled), the one ulp of v_exp_f32.  An error e_j
             of x_ij is a relative error ln2 e_j of p_ij, and sum_j p_j (1 + ln2 e_j) v_j / sum_j p_j (1 + ln2 e_j) - ref =
             sum_j p_j ln2 e_j (v_j - ref) to first order, at most ln2 max|e| S: weighted by S, not A -- a COMMON relative
             error of a row's p cancels against l, so a one-hot row gets no slack from huge scores.
Both u terms can be met at once: a pre-scaled one-hot row whose maximum needs more than M's 16 bits has p = 1 +- 2^-7 instead of
1, rounded to bf16 for the product and not for l, and its O is rounded again (the rescale launches of
tests/test_gpu_attention_forms.py reach 0.99 B that way; the emulation below keeps M to 16 bits for that reason).
"""
import collections
import math

import numpy as np

U = 2.0 ** -8
U32 = 2.0 ** -24
LOG2E = 1.4426950408889634
BF16_SENTINEL = 0x7FA5      # a NaN pattern no conversion produces
SCORE_TERMS = 70

Ref = collections.namedtuple("Ref", "ref A S mag bound")


def bf16_round(x):
    """fp32 values rounded to the nearest bf16 (ties to even), as fp32."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_bits_to_f64(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def exponent_scale(scale):
    """What a raw score q . k is multiplied by to be in the exponent's (log2) units."""
    return 1.0 if scale is None else float(np.float32(scale)) * LOG2E


def reference(q, k, v, heads, scale=None):
    """q [Tq][heads*64], k / v [Tk][heads*64]: the exact values of the bf16 operands; scale None: pre-scaled queries.
    -> Ref(ref, A, S, mag, bound): fp64 [Tq][heads*64] (mag: [Tq][heads], max_j sum_c |q k| in the exponent's units)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    Tq, Tk = q.shape[0], k.shape[0]
    f = exponent_scale(scale)
    ref, A, S = (np.zeros((Tq, heads * 64)) for _ in range(3))
    mag = np.zeros((Tq, heads))
    for h in range(heads):
        c = slice(64 * h, 64 * h + 64)
        x = (q[:, c] @ k[:, c].T) * f
        p = np.exp2(x - x.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        ref[:, c] = p @ v[:, c]
        A[:, c] = p @ np.abs(v[:, c])
        for d in range(64 * h, 64 * h + 64):
            S[:, d] = (p * np.abs(v[None, :, d] - ref[:, d, None])).sum(1)
        mag[:, h] = (np.abs(q[:, c]) @ np.abs(k[:, c]).T).max(1) * f
    c_acc = (Tk + 64) * U32
    c_exp = np.repeat(2.0 * math.log(2.0) * SCORE_TERMS * U32 * mag, 64, axis=1)
    bound = U * A + U * np.abs(ref) + c_acc * A + c_exp * S
    return Ref(ref, A, S, mag, bound)


def ratio(got, R):
    """|got - ref| / B per element (0 where the error is 0: B is 0 where every value of a column is 0)."""
    err = np.abs(np.asarray(got, np.float64) - R.ref)
    return np.where(err == 0.0, 0.0, err / np.maximum(R.bound, 1e-300))


def worst(got, R, nqb=4, label=""):
    """The largest error / B of one output, where it is, and a line of text for the log."""
    r = ratio(got, R)
    assert not np.isnan(r).any(), "%s: NaN in the output, first at %s" % (label, tuple(int(v) for v in np.argwhere(np.isnan(r))[0]))
    i = np.unravel_index(np.argmax(r), r.shape)
    q, col = int(i[0]), int(i[1])
    where = {"query": q, "block": q // (32 * nqb), "in_block": q % (32 * nqb), "head": col // 64, "d": col % 64}
    text = "%s: largest error / B %.4f at %s (got %.9g, ref %.9g, B %.3g; %d over)" % (
        label, r[i], where, np.asarray(got)[i], R.ref[i], R.bound[i], int((r > 1.0).sum()))
    return float(r[i]), where, text


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic
def emulate(q, k, v, heads, scale=None, lag=0.0, l_from_bf16=False):
    """The kernels' arithmetic in NumPy: scores in fp32; per 64-key tile of each key half (tile pairs of 128 keys, the halves
    merged at the end) a running maximum M that LAGS the true one by `lag` log2 units (the pre-scaled kernels let it lag by up to
    10: p <= 2^10) and, pre-scaled, is kept to 16 bits (so a one-hot row's p is not exactly 1); p = 2^(x - M) in fp32, summed in fp32 (l_from_bf16: from the bf16-rounded p instead -- allowed by the contract);
    p rounded to bf16 for the product; fp32 P.V; bf16 output.  Returns the output values as fp32."""
    f32 = np.float32
    q, k, v = (np.asarray(a, f32) for a in (q, k, v))
    Tq, Tk = q.shape[0], k.shape[0]
    sl = f32(exponent_scale(scale))
    out = np.zeros((Tq, heads * 64), f32)
    for h in range(heads):
        c = slice(64 * h, 64 * h + 64)
        x = (q[:, c] @ k[:, c].T).astype(f32)
        if scale is not None:
            x = (x * sl).astype(f32)
        state = []
        for kh in (0, 1):
            m_true = np.full(Tq, -np.inf, f32)
            M = np.zeros(Tq, f32)
            l = np.zeros(Tq, f32)
            o = np.zeros((Tq, 64), f32)
            for j0 in range(64 * kh, Tk, 128):
                j1 = min(j0 + 64, Tk)
                xt = x[:, j0:j1]
                first = not np.isfinite(m_true).any()
                m_true = np.maximum(m_true, xt.max(1))
                M_new = (m_true - f32(lag)).astype(f32)
                if scale is None:      # the pre-scaled kernels keep M as two bf16 parts (it enters the score product): 16 bits
                    hi = bf16_round(M_new)
                    M_new = np.where(np.isfinite(M_new), hi + bf16_round((M_new - hi).astype(f32)), M_new).astype(f32)
                alpha = np.ones(Tq, f32) if first else np.exp2((M - M_new).astype(f32)).astype(f32)
                M = M_new
                p = np.exp2((xt - M[:, None]).astype(f32)).astype(f32)
                pb = bf16_round(p)
                l = (l * alpha + (pb if l_from_bf16 else p).sum(1, dtype=f32)).astype(f32)
                o = (o * alpha[:, None] + (pb @ v[j0:j1, c]).astype(f32)).astype(f32)
            state.append((M, l, o, np.isfinite(m_true)))
        (M0, l0, o0, _), (M1, l1, o1, has1) = state
        M1 = np.where(has1, M1, f32(-np.inf)).astype(f32)
        m = np.maximum(M0, M1)
        a0 = np.exp2((M0 - m).astype(f32)).astype(f32)
        a1 = np.where(has1, np.exp2(np.where(has1, M1 - m, 0).astype(f32)), 0).astype(f32)
        inv = (f32(1) / (a0 * l0 + a1 * l1).astype(f32)).astype(f32)
        out[:, c] = bf16_round(((a0[:, None] * o0 + a1[:, None] * o1).astype(f32) * inv[:, None]).astype(f32))
    return out


def operands(rng, Tq, Tk, heads, scale=None):
    """Random bf16 operands of the size the transformers have: scores of unit variance in natural-log units.  fp32 arrays holding
    exact bf16 values; the pre-scaled queries carry 0.125 log2(e)."""
    D = heads * 64
    qf = 0.125 * LOG2E if scale is None else 1.0
    q = bf16_round(rng.standard_normal((Tq, D), dtype=np.float32) * np.float32(qf))
    k = bf16_round(rng.standard_normal((Tk, D), dtype=np.float32))
    v = bf16_round(rng.standard_normal((Tk, D), dtype=np.float32))
    return q, k, v
