"""Constant tables of the no-reference scorers, built on the host with numpy (no torch, no device): ``bem.ops`` uploads each once per
device and hands it to the kernels.

NIQE (basicsr/metrics/niqe.py as Enhancement/eval.py:248-254 calls it): the AGGD shape grid of estimate_aggd_param (niqe.py:24-26) with
its closed-form gamma ratios, and per input length the weights and symmetric-padded source indices of MATLAB's antialiased bicubic x0.5
resize (matlab_functions.py:16-81).  UIQM / UCIQE (basicsr/metrics/uciqe_uiqm.py as Enhancement/eval.py:255-260 calls them): per (source
length, target length) Pillow's fixed-point BICUBIC coefficients (Resample.c), and OpenCV 4.x's 8-bit RGB -> Lab tables (color_lab.cpp,
RGB2Lab_b)."""
import math

import numpy as np

UIQM_WIDTH = 256


def niqe_gamma_table():
    """(4, 9801) f64: gam = arange(0.2, 10.001, 0.001), r_gam = G(2/a)^2 / (G(1/a) G(3/a)), sqrt(G(1/a) / G(3/a)), G(2/a) / G(1/a)."""
    gam = np.arange(0.2, 10.001, 0.001)
    rec = np.reciprocal(gam)
    tab = np.empty((4, gam.size))
    tab[0] = gam
    for i, (a, r) in enumerate(zip(gam.tolist(), rec.tolist())):
        tab[1, i] = math.gamma(r * 2) ** 2 / (math.gamma(r) * math.gamma(r * 3))
        tab[2, i] = math.sqrt(math.gamma(1 / a) / math.gamma(3 / a))
        tab[3, i] = math.gamma(2 / a) / math.gamma(1 / a)
    return tab


def niqe_resize_table(n, scale=0.5):
    """MATLAB imresize (bicubic, antialiased) along one axis of length n, in float32 like the reference: weights (out, K) f32 and the
    0-based source index of every tap (out, K) int32 with the symmetric padding folded in; all-zero end columns trimmed."""
    f32 = np.float32
    out = math.ceil(n * scale)
    width = 4.0 / scale if scale < 1 else 4.0
    x = np.arange(1, out + 1, dtype=f32)
    u = x / f32(scale) + f32(0.5 * (1 - 1 / scale))
    left = np.floor(u - f32(width / 2))
    taps = math.ceil(width) + 2
    idx = left[:, None] + np.arange(taps, dtype=f32)[None, :]
    d = np.abs((u[:, None] - idx) * f32(scale) if scale < 1 else u[:, None] - idx)
    d2, d3 = d ** 2, d ** 3
    cub = (f32(1.5) * d3 - f32(2.5) * d2 + f32(1)) * (d <= 1) + (f32(-0.5) * d3 + f32(2.5) * d2 - f32(4) * d + f32(2)) * ((d > 1) & (d <= 2))
    wt = (f32(scale) * cub if scale < 1 else cub).astype(f32)
    wt = wt / wt.sum(axis=1, keepdims=True)
    keep = np.ones(taps, bool)
    keep[0] = not (wt[:, 0] == 0).any()
    keep[-1] = not (wt[:, -1] == 0).any()
    wt, idx = wt[:, keep], idx[:, keep].astype(np.int64) - 1
    idx = np.where(idx < 0, -idx - 1, idx)
    idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    return np.ascontiguousarray(wt, dtype=f32), np.ascontiguousarray(idx, dtype=np.int32)


def _pil_bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_resize_table(n_in, n_out):
    """Pillow's BICUBIC resample of one axis, n_in -> n_out, in its 8-bit form (precompute_coeffs + normalize_coeffs_8bpc):
    bounds (n_out, 2) int32 = first source index and tap count, weights (n_out, K) int32 with 22 fractional bits, zero past the taps."""
    scale = n_in / n_out
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    K = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, K), np.int32)
    for o in range(n_out):
        center = (o + 0.5) * scale
        x0 = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - x0
        ss = 1.0 / fscale
        ws = [_pil_bicubic((x + x0 - center + 0.5) * ss) for x in range(n)]
        tot = 0.0
        for v in ws:
            tot += v
        for x, v in enumerate(ws):
            v = v / tot if tot != 0.0 else v
            kk[o, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds[o] = (x0, n)
    return bounds, kk


def lab_tables():
    """OpenCV 4.x RGB2Lab_b tables as one int32 vector: sRGB gamma x 255 x 8 (256 entries), 2^15 (x < 0.008856 ? 7.787 x + 16/116 : cbrt x)
    at x = i / (255 x 8) (3072), and the fixed-point matrix cvRound(4096 sRGB2XYZ_D65[i][j] / D65white[i]) (9, row-major, R G B order)."""
    x = np.arange(256) / 255.0
    gamma = np.rint(np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4) * 255.0 * 8)
    t = np.arange(3072) / (255.0 * 8)
    cbrt = np.rint((1 << 15) * np.where(t < 0.008856, t * 7.787 + 16.0 / 116.0, np.cbrt(t)))
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    coef = np.rint(4096 * m / np.array([0.950456, 1.0, 1.088754])[:, None])
    return np.concatenate([gamma, cbrt, coef.ravel()]).astype(np.int32)


def uiqm_resized_rows(h, w):
    """eval.py:257: the resized image is (int(256 / w * h), 256)."""
    return int(UIQM_WIDTH / w * h)
