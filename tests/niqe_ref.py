"""Float64 numpy restatement of NIQE as Enhancement/eval.py:248-254 computes it (calculate_niqe(pred * 255, crop_border=0) of
basicsr/metrics/niqe.py), written for the tests and independent of bem.ops: its own gamma tables, its own resize, plain numpy loops.

Convolution and resize sums, the fits and the MVG distance are float64.  Where the reference STORES float32 -- the Y levels, the MSCN
planes (scipy.ndimage returns the input dtype), the resized image and the paired products -- the values are rounded to float32 here too:
whether a saturated block's MSCN coefficients are exactly 0 or a one-signed 1e-5 decides which feature rows are NaN.  The four block
means of the AGGD fit are numpy's float32 means, as in the reference: near a boundary of the 0.001-step alpha grid, a float64 mean can
pick the neighbouring alpha (the device kernel sums in float64 and may sit one grid step away there).
The channel-order quirk is kept: the reference's BGR weights meet RGB data, so 24.966 multiplies R."""
import math
import warnings

import numpy as np

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def gamma_tables():
    gam = np.arange(0.2, 10.001, 0.001)
    g = np.vectorize(math.gamma)
    r_gam = g(2 / gam) ** 2 / (g(1 / gam) * g(3 / gam))
    return gam, r_gam


_TABLES = None


def _tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = gamma_tables()
    return _TABLES


def y_channel(rgb01):
    """(h,w,3) float32 in [0,1] -> (h,w) float64 of integer levels (round half to even)."""
    f = np.float32
    t = (rgb01.astype(f) * f(255)) / f(255)
    y = ((t[..., 0].astype(np.float64) * 24.966 + t[..., 1] * 128.553) + t[..., 2] * 65.481) + 16.0
    y = (y / 255.0).astype(f) * f(255)
    return np.round(y)


def _conv_nearest(img, win):
    """scipy.ndimage.convolve(img, win, mode='nearest') for a 7x7 window."""
    p = np.pad(img, 3, mode="edge")
    H, W = img.shape
    out = np.zeros_like(img)
    wf = win[::-1, ::-1]
    for a in range(7):
        for b in range(7):
            out += wf[a, b] * p[a:a + H, b:b + W]
    return out


def mscn(img, win):
    """img float32 -> float32 MSCN plane (f64 sums, f32 results and arithmetic like scipy.ndimage + numpy on float32)."""
    img = img.astype(np.float32)
    mu = _conv_nearest(img.astype(np.float64), win).astype(np.float32)
    sq = _conv_nearest(np.square(img).astype(np.float64), win).astype(np.float32)
    sigma = np.sqrt(np.abs(sq - np.square(mu)))
    return (img - mu) / (sigma + np.float32(1))


def _cubic(x):
    a = np.abs(x)
    return np.where(a <= 1, 1.5 * a ** 3 - 2.5 * a ** 2 + 1, np.where(a <= 2, -0.5 * a ** 3 + 2.5 * a ** 2 - 4 * a + 2, 0.0))


def _halve_axis0(img):
    """MATLAB imresize(., 0.5, 'bicubic', antialiasing) along axis 0: kernel cubic(x/2)/2 over 8 taps, symmetric borders."""
    n = img.shape[0]
    out = np.empty((math.ceil(n / 2),) + img.shape[1:])
    for o in range(out.shape[0]):
        u = 2 * (o + 1) - 0.5                                 # 1-based source coordinate of output o
        idx = np.floor(u - 4) + np.arange(10)                 # 1-based taps
        wt = 0.5 * _cubic((u - idx) * 0.5)
        wt /= wt.sum()
        src = idx.astype(int) - 1
        src = np.where(src < 0, -src - 1, src)
        src = np.where(src >= n, 2 * n - 1 - src, src)
        out[o] = np.tensordot(wt, img[src].astype(np.float64), axes=1)
    return out


def halve(img):
    """float32 -> float32, rounded after each pass like the reference's torch tensors."""
    return _halve_axis0(_halve_axis0(img).astype(np.float32).T).T.astype(np.float32)


def aggd(x):
    """estimate_aggd_param: (alpha index, alpha, beta_l, beta_r); alpha index 0 when the fit ratio is NaN (np.argmin of all-NaN)."""
    gam, r_gam = _tables()
    x = x.ravel().astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        ls = float(np.sqrt(np.mean(x[x < 0] ** 2))) if (x < 0).any() else np.nan
        rs = float(np.sqrt(np.mean(x[x > 0] ** 2))) if (x > 0).any() else np.nan
        g = ls / rs if rs == rs and rs != 0 else np.nan
        rhat = float(np.mean(np.abs(x))) ** 2 / float(np.mean(x ** 2)) if (x != 0).any() else np.nan
        rn = (rhat * (g ** 3 + 1) * (g + 1)) / ((g ** 2 + 1) ** 2)
    k = 0 if np.isnan(rn) else int(np.argmin((r_gam - rn) ** 2))
    a = gam[k]
    f = math.sqrt(math.gamma(1 / a) / math.gamma(3 / a))
    return k, a, ls * f, rs * f


def block_features(block):
    _, a, bl, br = aggd(block)
    feat = [a, (bl + br) / 2]
    for s in SHIFTS:
        _, a, bl, br = aggd(block * np.roll(block, s, axis=(0, 1)))       # float32 products
        feat += [a, (br - bl) * (math.gamma(2 / a) / math.gamma(1 / a)), bl, br]
    return feat


def features(y, win):
    """(nblocks, 36) feature rows, blocks idx_w-major like niqe.py."""
    nbh, nbw = y.shape[0] // BLOCK, y.shape[1] // BLOCK
    img = y[:nbh * BLOCK, :nbw * BLOCK]
    cols = []
    for scale in (1, 2):
        n = mscn(img, win)
        bs = BLOCK // scale
        cols.append(np.array([block_features(n[bh * bs:(bh + 1) * bs, bw * bs:(bw + 1) * bs]) for bw in range(nbw) for bh in range(nbh)]))
        if scale == 1:
            img = halve(img / np.float32(255)) * np.float32(255)
    return np.concatenate(cols, axis=1)


def mvg(feat, mu_pris, cov_pris):
    """-> (score, mu_d, cov_d); NaN when fewer than 2 rows are NaN-free."""
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # all-NaN columns: nanmean gives NaN, as in the reference
        mu_d = np.nanmean(feat, axis=0)
    clean = feat[~np.isnan(feat).any(axis=1)]
    if clean.shape[0] < 2:
        return float("nan"), mu_d, None
    cov_d = np.cov(clean, rowvar=False)
    d = np.ravel(mu_pris) - mu_d
    return float(np.sqrt(d @ np.linalg.pinv((cov_pris + cov_d) / 2) @ d)), mu_d, cov_d


def niqe(rgb01, params):
    """rgb01: (h,w,3) or (3,h,w) float32 in [0,1]; params: dict-like with mu_pris_param, cov_pris_param, gaussian_window."""
    rgb01 = np.asarray(rgb01, dtype=np.float32)
    if rgb01.shape[0] == 3 and rgb01.shape[-1] != 3:
        rgb01 = rgb01.transpose(1, 2, 0)
    feat = features(y_channel(rgb01), np.asarray(params["gaussian_window"], dtype=np.float64))
    return mvg(feat, np.asarray(params["mu_pris_param"], np.float64), np.asarray(params["cov_pris_param"], np.float64))[0]


# ---- the fixture tests/golden/g13_niqe.npz (written by tests/golden/make_golden_niqe.py) ----
def variant(u8, g, k):
    """uint8 -> uint8: clip(k * (u8 / 255) ** g, 0, 1) * 255, rounded (make_golden_niqe.variant)."""
    return np.rint(np.clip(k * (u8.astype(np.float64) / 255.0) ** g, 0, 1) * 255).astype(np.uint8)


def fixture_inputs(z):
    """{name: uint8 (h,w,3)} of the fixture's per-input cases; the saturated one is rebuilt from its box."""
    out = {}
    for k in (str(n) for n in z["names"]):
        if k == "saturated":
            r0, r1, c0, c1 = (int(v) for v in z["sat_box"])
            img = z["in_crop400x600"].copy()
            img[r0:r1, c0:c1] = 255
        else:
            img = z[f"in_{k}"]
        out[k] = img
    return out


def fixture_candidates(z):
    """(6, h, w, 3) uint8: the candidate set's gamma / gain variants of its source crop."""
    return np.stack([variant(z["cand_src"], g, k) for g, k in z["cand_gk"]])


def as_pred(u8):
    """uint8 HWC -> the float32 candidate the reference sees (u8 / 255)."""
    return u8.astype(np.float32) / np.float32(255)


ALPHA_COLS = [c for c in range(36) if c % 18 in (0, 2, 6, 10, 14)]
