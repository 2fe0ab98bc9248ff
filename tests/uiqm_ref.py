"""Numpy restatement of the UIQM / UCIQE selection scores as Enhancement/eval.py:255-260 computes them (getUIQM and getUCIQE of
basicsr/metrics/uciqe_uiqm.py), written for the tests and independent of bem.ops: plain numpy and Python loops.

Pieces and the reference lines they restate:
  quantise    img_as_ubyte(pred): rint(255 x) in float32, half to even (eval.py:257,260)
  pil_resize  Image.fromarray(u8).resize((256, int(256 / w * h))): Pillow's BICUBIC in its 8-bit fixed-point form (Resample.c:
              precompute_coeffs, normalize_coeffs_8bpc, 22 fractional bits), horizontal pass first, uint8 in between
  uicm        _uicm :328 with mu_a :302 (float32 sum in sorted order, one element short of its divisor) and s_a :322
  uism        _uism :431 with sobel :343 (scipy.ndimage.sobel, mode 'reflect') and eme :377 (last block absorbs the remainder,
              float32 sum of float32 terms in row-major block order)
  uiconm      _uiconm :488 (crop to whole 10 x 10 blocks, column-major block order, float64 sum)
  uiqm        getUIQM :525; under NumPy 2 (NEP 50) the c2 * uism term and everything added to it are float32
  rgb2lab_u8  cv2.cvtColor(u8, COLOR_RGB2LAB): OpenCV 4.x RGB2Lab_b (color_lab.cpp), integer tables and shifts
  uciqe       getUCIQE :42 on the Lab image (np.histogram with 65536 bins for the luminance contrast)
"""
import math

import numpy as np

F32 = np.float32
PREC = 22                      # Pillow Resample.c PRECISION_BITS (32 - 8 - 2)
WIN = 10


# ------------------------------------------------------------------------------------------------------------ quantise / resize
def quantise(pred):
    """(h,w,3) float32 in [0,1] -> uint8, skimage.img_as_ubyte: rint(x * 255) in float32."""
    return np.clip(np.rint(pred.astype(F32) * F32(255)), 0, 255).astype(np.uint8)


def resized_size(h, w):
    """eval.py:257: PIL size (256, int(256 / w * h)) -> (rows, cols)."""
    return int(256 / w * h), 256


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_coeffs(n_in, n_out):
    """Pillow's BICUBIC coefficients for one axis: bounds (n_out, 2) int32 (first source index, tap count) and the fixed-point
    weights (n_out, ksize) int32, zero beyond each row's tap count."""
    scale = n_in / n_out
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        ss = 1.0 / fscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        for x, v in enumerate(k):
            v = v / ww if ww != 0.0 else v
            kk[xx, x] = int(-0.5 + v * (1 << PREC)) if v < 0 else int(0.5 + v * (1 << PREC))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass(u8, bounds, kk, axis):
    """One fixed-point pass along `axis` of an (h,w,c) uint8 image."""
    src = np.moveaxis(u8.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    for o, (x0, n) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (PREC - 1), np.int64)
        for t in range(n):
            acc += src[x0 + t] * int(kk[o, t])
        out[o] = np.clip(acc >> PREC, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_resize(u8, rows, cols):
    """Image.fromarray(u8).resize((cols, rows)) for an RGB uint8 image, BICUBIC (Pillow's default for RGB)."""
    tmp = _pass(u8, *pil_coeffs(u8.shape[1], cols), axis=1)
    return _pass(tmp, *pil_coeffs(u8.shape[0], rows), axis=0)


# ------------------------------------------------------------------------------------------------------------------------ UIQM
def mu_a(x):
    """mu_a :302: float32 sum of sorted[T_L + 1 : K - T_R] (sequential, as Python's sum over np.float32), times float32(1 / (K - T_L - T_R))."""
    x = np.sort(x.astype(F32))
    K = x.size
    tl, tr = math.ceil(0.1 * K), math.floor(0.1 * K)
    weight = 1 / (K - tl - tr)
    part = x[tl + 1:K - tr]
    val = np.add.accumulate(part, dtype=F32)[-1] if part.size else F32(0)
    return F32(F32(weight) * val)


def s_a(x, mu):
    d = (x.astype(F32) - F32(mu)).astype(np.float64)
    return float(np.sum(d * d)) / x.size


def uicm(x):
    R, G, B = (x[..., c].ravel() for c in range(3))
    rg = R - G
    yb = ((R + G) / F32(2)) - B
    mrg, myb = mu_a(rg), mu_a(yb)
    l = math.sqrt(float(mrg) ** 2 + float(myb) ** 2)
    r = math.sqrt(s_a(rg, mrg) + s_a(yb, myb))
    return (-0.0268 * l) + (0.1586 * r)


def _sobel_axis(x, axis):
    """scipy.ndimage.sobel(x, axis) for float32 integer-valued input: [-1,0,1] along axis, [1,2,1] across, mode 'reflect'."""
    p = np.pad(x.astype(np.float64), 1, mode="symmetric")
    H, W = x.shape
    s = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    if axis == 0:
        d = lambda dx: s(1, dx) - s(-1, dx)
        return (d(-1) + 2 * d(0) + d(1)).astype(F32)
    d = lambda dy: s(dy, 1) - s(dy, -1)
    return (d(-1) + 2 * d(0) + d(1)).astype(F32)


def sobel(x):
    """sobel :343, float32 throughout; a plane without edges gives NaN (255 / 0 = inf, 0 * inf)."""
    mag = np.hypot(_sobel_axis(x, 0), _sobel_axis(x, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        mag *= F32(255.0) / np.max(mag)
    return mag


def eme(ch):
    """eme :377: block min / max, the last block of each axis absorbs the remainder, float32 terms summed in float32."""
    nx, ny = ch.shape[0] // WIN, ch.shape[1] // WIN
    w = F32(2.0 / (nx * ny))
    val = F32(0)
    for i in range(nx):
        x0, x1 = i * WIN, ((i + 1) * WIN if i < nx - 1 else ch.shape[0])
        for j in range(ny):
            y0, y1 = j * WIN, ((j + 1) * WIN if j < ny - 1 else ch.shape[1])
            blk = ch[x0:x1, y0:y1]
            mn, mx = blk.min(), blk.max()
            if mn == 0 or mx == 0:
                continue
            with np.errstate(invalid="ignore"):
                val = F32(val + F32(w * np.log(F32(mx / mn))))
    return val


def uism(x):
    e = [eme(np.multiply(sobel(x[..., c]), x[..., c])) for c in range(3)]
    return F32(F32(F32(0.299) * e[0] + F32(0.587) * e[1]) + F32(0.144) * e[2])


def uiconm(x):
    """_uiconm :488, window 10: the image cropped to whole blocks, blocks visited column-major, float64 sum of (t/b) log(t/b)."""
    k1, k2 = x.shape[1] // WIN, x.shape[0] // WIN
    val = 0.0
    for l in range(k1):
        for k in range(k2):
            blk = x[k * WIN:(k + 1) * WIN, l * WIN:(l + 1) * WIN, :]
            mx, mn = blk.max(), blk.min()
            top, bot = F32(mx - mn), F32(mx + mn)
            if math.isnan(top) or math.isnan(bot) or bot == 0.0 or top == 0.0:
                continue
            q = float(F32(top / bot))
            val += q * math.log(q)
    return (-1.0 / (k1 * k2)) * val


def uiqm_parts(u8_resized):
    """getUIQM :525 on the resized uint8 image -> (uicm, uism, uiconm, uiqm); uiqm as NumPy 2 rounds it (float32 after the c2 term)."""
    x = u8_resized.astype(F32)
    a, b, c = uicm(x), uism(x), uiconm(x)
    q = F32(F32(0.0282 * a) + F32(F32(0.2953) * b))
    q = F32(q + F32(3.5753 * c))
    return a, float(b), c, float(q)


# ------------------------------------------------------------------------------------------------------------------ Lab / UCIQE
_LAB = None


def lab_tables():
    """OpenCV 4.x RGB2Lab_b tables: sRGB gamma x 255 x 8 (256), 2^15 f(x) at x = i / (255 * 8) (3072), the 3 x 3 fixed-point matrix
    cvRound(4096 * sRGB2XYZ_D65 / D65white)."""
    global _LAB
    if _LAB is None:
        x = np.arange(256) / 255.0
        g = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
        gamma = np.rint(g * 255.0 * 8).astype(np.int64)
        t = np.arange(3072) / (255.0 * 8)
        cbrt = np.rint((1 << 15) * np.where(t < 0.008856, t * 7.787 + 16.0 / 116.0, np.cbrt(t))).astype(np.int64)
        m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
        white = np.array([0.950456, 1.0, 1.088754])
        coef = np.rint(4096 * m / white[:, None]).astype(np.int64)
        _LAB = gamma, cbrt, coef
    return _LAB


def rgb2lab_u8(u8):
    """cv2.cvtColor(u8, cv2.COLOR_RGB2LAB) for uint8 RGB (..., 3) -> uint8 (..., 3)."""
    gamma, cbrt, C = lab_tables()
    rgb = gamma[u8.astype(np.int64)]
    d = lambda v, n: (v + (1 << (n - 1))) >> n
    f = [cbrt[d(rgb @ C[i], 12)] for i in range(3)]
    L = d(296 * f[1] - 1336935, 15)
    a = d(500 * (f[0] - f[1]) + (128 << 15), 15)
    b = d(200 * (f[1] - f[2]) + (128 << 15), 15)
    return np.clip(np.stack([L, a, b], -1), 0, 255).astype(np.uint8)


def uciqe_parts(lab):
    """getUCIQE :42 after the colour conversion -> (var_chr, con_lum, aver_sat, uciqe)."""
    lum, a, b = (lab[..., c] / 255 for c in range(3))
    chr_ = np.sqrt(np.square(a) + np.square(b))
    sat = chr_ / np.sqrt(np.square(chr_) + np.square(lum))
    aver_sat = np.mean(sat)
    with np.errstate(divide="ignore", invalid="ignore"):
        var_chr = np.sqrt(np.mean(abs(1 - np.square(np.mean(chr_) / chr_))))
    hist, _ = np.histogram(lum, 65536)
    cdf = np.cumsum(hist) / np.sum(hist)
    ilow, ihigh = np.where(cdf > 0.0100)[0][0], np.where(cdf >= 0.9900)[0][0]
    con_lum = (ihigh - 1) / 65535 - (ilow - 1) / 65535
    return float(var_chr), float(con_lum), float(aver_sat), float(0.4680 * var_chr + 0.2745 * con_lum + 0.2576 * aver_sat)


def con_lum_levels(counts):
    """con_lum from a 256-level count histogram of L (the device's route): numpy's histogram bin of each present level by its own
    rule (linspace edges, then the +-1 edge correction of _histograms_impl), then the first cumulative fractions > 0.01, >= 0.99."""
    lv = np.nonzero(counts)[0]
    first, last = lv[0] / 255, lv[-1] / 255
    if first == last:
        first, last = first - 0.5, last + 0.5
    step = (last - first) / 65536
    edge = lambda i: last if i == 65536 else i * step + first
    n, c, ilow, ihigh = int(counts.sum()), 0, None, None
    for v in lv:
        x = v / 255
        i = int((x - first) / (last - first) * 65536)
        i -= i == 65536
        if x < edge(i):
            i -= 1
        if x >= edge(i + 1) and i != 65535:
            i += 1
        c += int(counts[v])
        if ilow is None and c / n > 0.01:
            ilow = i
        if ihigh is None and c / n >= 0.99:
            ihigh = i
    return (ihigh - 1) / 65535 - (ilow - 1) / 65535


def scores(pred):
    """(h,w,3) float32 candidate -> dict of every part, as eval.py:256-260 computes them."""
    u8 = quantise(pred)
    rs = pil_resize(u8, *resized_size(*u8.shape[:2]))
    uicm_, uism_, uiconm_, uiqm_ = uiqm_parts(rs)
    var_chr, con_lum, aver_sat, uciqe_ = uciqe_parts(rgb2lab_u8(u8))
    return dict(uicm=uicm_, uism=uism_, uiconm=uiconm_, uiqm=uiqm_, var_chr=var_chr, con_lum=con_lum, aver_sat=aver_sat, uciqe=uciqe_)


def select(uiqm, uciqe, w):
    """eval.py:277-278: index of the first maximum of w uiqm / max(uiqm) + (1 - w) uciqe / max(uciqe)."""
    s = (w * np.array(uiqm, F32) / max(uiqm) + (1 - w) * np.array(uciqe) / max(uciqe)).tolist()
    return s.index(max(s))


PART_NAMES = ("uicm", "uism", "uiconm", "uiqm", "var_chr", "con_lum", "aver_sat", "uciqe")
