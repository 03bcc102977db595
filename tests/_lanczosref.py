"""Pillow's 8-bit LANCZOS resample restated in Python / numpy, for the tests of the device front end.

Coefficients: plain Python floats (IEEE double) and math.sin -- libm's sin, the function the C side calls; numpy's vectorised sin
is another implementation and may differ in the last bit.  Passes: int32 accumulation, arithmetic shift, clamp."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def tables(in_size, out_size):
    """-> (ksize, bounds int32 [out, 2] = (xmin, taps), kk int32 [out, ksize])"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ss = 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            kk[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
    return ksize, bounds, kk


def apply_pass(a, bounds, kk, axis):
    """One pass over `axis` (0 or 1) of a uint8 [H, W, C] array with the tables of that axis."""
    a = np.moveaxis(a, axis, 0).astype(np.int32)
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
        for x in range(n):
            acc += a[lo + x] * kk[i, x]
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(a, out_h, out_w, table_fn=tables):
    """Image.resize((out_w, out_h), LANCZOS) of a uint8 [H, W] or [H, W, C] array: the horizontal pass, then the vertical one;
    a pass whose size does not change is skipped.  table_fn: where the tables come from (this module, or the library)."""
    flat = a.ndim == 2
    if flat:
        a = a[:, :, None]
    if a.shape[1] != out_w:
        _, b, k = table_fn(a.shape[1], out_w)
        a = apply_pass(a, b, k, 1)
    if a.shape[0] != out_h:
        _, b, k = table_fn(a.shape[0], out_h)
        a = apply_pass(a, b, k, 0)
    return a[:, :, 0] if flat else a
