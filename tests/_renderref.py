"""The sample placement and the alpha composite of the volume renderer, restated in numpy (TripoSR/tsr/models/nerf_renderer.py
:109-149) for tests/test_render_host.py and tests/test_gpu_render.py.  Two forms, both fed with per-sample density_act [N, S] and
color [N, S, 3]:

  composite64   every operation in fp64
  composite32   fp32, one sample after the other, each operation rounded on its own -- the order csrc/render.hip uses:
                    alpha = 1 - exp(-delta * density_act);  w = alpha * T;  sum_w += w;  sum_c += w * color;
                    T = T * ((1 - alpha) + 1e-10)
                and rgb = sum_c + (1 - sum_w) at the end.

delta is the step of the unit interval t_vals (the reference's choice), not a length along the ray.  An invalid ray has zero
weights and opacity and is white.
"""
import numpy as np


def sample_z(t_near, t_far, t_vals):
    """z [N, S] = t_near (1 - t_mid) + t_far t_mid with t_mid the interval midpoints, in the dtype of the arguments."""
    t_vals = np.asarray(t_vals)
    one, two = t_vals.dtype.type(1), t_vals.dtype.type(2)
    t_mid = (t_vals[:-1] + t_vals[1:]) / two
    tn, tf = np.asarray(t_near).reshape(-1, 1), np.asarray(t_far).reshape(-1, 1)
    return tn * (one - t_mid[None]) + tf * t_mid[None]


def composite64(density_act, color, t_vals, valid):
    d, c, t = np.asarray(density_act, np.float64), np.asarray(color, np.float64), np.asarray(t_vals, np.float64)
    valid = np.asarray(valid, bool)
    alpha = 1.0 - np.exp(-(t[1:] - t[:-1])[None] * d)
    trans = np.concatenate([np.ones_like(alpha[:, :1]), np.cumprod(1.0 - alpha[:, :-1] + 1e-10, axis=-1)], axis=-1)
    w = alpha * trans * valid[:, None]
    opacity = w.sum(-1)
    rgb = (w[..., None] * c).sum(-2) + (1.0 - opacity)[:, None]
    return {"weights": w, "opacity": opacity, "comp_rgb": rgb}


def composite32(density_act, color, t_vals, valid):
    f = np.float32
    d, c, t = np.asarray(density_act, f), np.asarray(color, f), np.asarray(t_vals, f)
    valid = np.asarray(valid, bool)
    N, S = d.shape
    T, sw, sc = np.ones(N, f), np.zeros(N, f), np.zeros((N, 3), f)
    w_all = np.zeros((N, S), f)
    for i in range(S):
        delta = f(t[i + 1] - t[i])
        alpha = f(1) - np.exp(-delta * d[:, i], dtype=f)
        w = alpha * T
        sw = sw + w
        sc = sc + w[:, None] * c[:, i]
        T = T * ((f(1) - alpha) + f(1e-10))
        w_all[:, i] = w
    w_all[~valid], sw[~valid], sc[~valid] = 0, 0, 0
    rgb = sc + (f(1) - sw)[:, None]
    assert w_all.dtype == f and rgb.dtype == f
    return {"weights": w_all, "opacity": sw, "comp_rgb": rgb}
