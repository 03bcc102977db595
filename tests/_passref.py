"""The render passes restated in numpy for tests/test_render_passes_host.py and tests/test_gpu_render_passes.py: the raw per-ray
sums of csrc/render.hip from given per-sample weights [N, S], depths [N, S] and normals [N, S, 3], and the finishing rules of
sculptmate_amd/tsr/passes.py.

  sums32   fp32, one sample after the other, each operation rounded on its own -- the order the kernels use:
               depth_sum += w * z;   normal_sum[k] += w * n[k]
  sums64   the same sums with every operation in fp64
"""
import numpy as np


def sums32(weights, z_vals, normals):
    f = np.float32
    w, z, n = np.asarray(weights, f), np.asarray(z_vals, f), np.asarray(normals, f)
    N, S = w.shape
    depth, nsum = np.zeros(N, f), np.zeros((N, 3), f)
    for i in range(S):
        depth = depth + w[:, i] * z[:, i]
        nsum = nsum + w[:, i, None] * n[:, i]
    assert depth.dtype == f and nsum.dtype == f
    return {"depth_sum": depth, "normal_sum": nsum}


def sums64(weights, z_vals, normals):
    w, z, n = (np.asarray(a, np.float64) for a in (weights, z_vals, normals))
    return {"depth_sum": (w * z).sum(-1), "normal_sum": (w[..., None] * n).sum(-2)}


def depth_of(depth_sum, opacity):
    d, o = np.asarray(depth_sum), np.asarray(opacity)
    return np.divide(d, o, out=np.zeros_like(d), where=o > 0)


def normal_of(normal_sum):
    n = np.asarray(normal_sum, np.float64)
    length = np.sqrt((n * n).sum(-1, keepdims=True))
    return np.divide(n, length, out=np.zeros_like(n), where=length > 0)


def rgba_of(premul, opacity):
    return np.concatenate([np.asarray(premul), np.asarray(opacity)[..., None]], axis=-1)
