"""Plain-torch references of the eval step's entry and exit kernels in csrc/layout.hip and csrc/selection.hip (not collected by pytest), one function per
entry point, written from that file's comments and the restatements in oracle/bem_oracle.py (which carry the file:line citations).  Nothing
here imports bem.

Every function is dtype-generic: on float64 CPU tensors it is the yardstick, on the same values in float32 it is the "f32 reference" whose
own distance from float64 sets the per-pixel bounds of tests/test_selection_gpu.py.  The selection rules work on Python lists, like the
reference's.  Below the references: the shape tables and the seeded input builders of the GPU tests, here so that
tests/test_selection_cpu.py can check the conditions the GPU tests rely on (selection gaps, SSIM inputs on integer levels).

Where a candidate channel's clamped sum is 0 the references follow numpy / torch: x * (t / 0) is NaN and survives the clamp.  The kernels
leave such a channel at 0 ("Selection tail: edges"); the tests state that difference explicitly where they reach it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

ULP = 2.0 ** -23
MARGIN = 4.0            # reductions: the project's margin over the measured f32 term (tests/test_attn_blocks_gpu.py)
GAP = 100.0             # selection cases: best and runner-up differ by GAP x the largest score error the bounds admit


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ulp32(v):
    """Spacing of float32 at |v| (elementwise, float64 tensor)."""
    v = torch.as_tensor(v, dtype=torch.float64)
    return torch.from_numpy(np.spacing(np.abs(v.numpy()).astype(np.float32)).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ entry
def reflect_index(n_out, n):
    """numpy 'reflect' at the far end: i for i < n, else 2 (n - 1) - i (the edge sample is not repeated); needs n_out - n < n."""
    i = torch.arange(n_out)
    return torch.where(i < n, i, 2 * (n - 1) - i)


def pad_reflect(x, Hp, Wp):
    """(..., H, W) -> (..., Hp, Wp), padded at the bottom and the right."""
    H, W = x.shape[-2:]
    assert 0 <= Hp - H < H and 0 <= Wp - W < W
    return x[..., reflect_index(Hp, H), :][..., :, reflect_index(Wp, W)]


def resize_down(x, s):
    """INTER_LINEAR by 1/s for even s dividing H and W: the mean of the 2x2 pixels at (s i + s/2 - 1 .. s i + s/2) in both axes."""
    a = s // 2 - 1
    return 0.25 * (x[..., a::s, a::s] + x[..., a + 1::s, a::s] + x[..., a::s, a + 1::s] + x[..., a + 1::s, a + 1::s])


def _taps(n_out, n, s, dtype):
    src = ((torch.arange(n_out, dtype=dtype) + 0.5) / s - 0.5).clamp_min(0)
    i0 = src.floor().long()
    i1 = torch.where(i0 < n - 1, i0 + 1, i0)
    return i0, i1, src - i0.to(dtype)


def bilinear_up(x, s):
    """upsample_bilinear2d, align_corners=False, scale s: hy (hx p00 + lx p01) + ly (hx p10 + lx p11), source (o + 0.5) / s - 0.5 >= 0."""
    H, W = x.shape[-2:]
    y0, y1, ly = _taps(H * s, H, s, x.dtype)
    x0, x1, lx = _taps(W * s, W, s, x.dtype)
    ly, hy = ly[:, None], 1 - ly[:, None]
    hx = 1 - lx
    top = hx * x[..., y0, :][..., :, x0] + lx * x[..., y0, :][..., :, x1]
    bot = hx * x[..., y1, :][..., :, x0] + lx * x[..., y1, :][..., :, x1]
    return hy * top + ly * bot


def plane_mean(x, h=None, w=None):
    """Mean over the top-left (h, w) window of every plane: (B,C,Hs,Ws) -> (B,C)."""
    h, w = h or x.shape[2], w or x.shape[3]
    return x[:, :, :h, :w].mean((2, 3))


def _zero_for_nan(x, zero_sum):
    """zero_sum 'nan': numpy's and torch's result, NaN where a channel's clamped sum is 0; 'zero': that channel stays 0, as the kernels
    leave it (the NaN of 0 * (t / 0) ends in fmaxf(NaN, 0) = 0)."""
    assert zero_sum in ("nan", "zero")
    return x if zero_sum == "nan" else torch.where(torch.isnan(x), torch.zeros_like(x), x)


def cond_postproc(pred, target_mean, noise, spi, noise_level, zero_sum="nan"):
    """clamp(pred, 0, 1); with target_mean (B,3): times target_mean / plane mean, clamped again; then + noise * noise_level."""
    c = pred.clamp(0, 1)
    if target_mean is not None:
        ratio = target_mean.repeat_interleave(spi, 0)[:, :, None, None] / c.mean((2, 3), keepdim=True)
        c = _zero_for_nan((c * ratio).clamp(0, 1), zero_sum)
    if noise is not None:
        c = c + noise * noise_level
    return c


# ------------------------------------------------------------------------------------------------------------------ exit
def psnr(target, final):
    """10 log10(1 / mean((target - final)^2)) over (3,h,w) per candidate, 100 where the error is 0: (Bn,3,h,w) x 2 -> (Bn)."""
    mse = ((target - final) ** 2).mean((1, 2, 3))
    return torch.where(mse == 0, torch.full_like(mse, 100.0), 10.0 * torch.log10(1.0 / mse))


def candidate_finalize(pred, target, spi, h, w, gt_mean, zero_sum="nan"):
    """pred (Bn,3,Hp,Wp), target (B,3,h,w)|None -> final (Bn,3,h,w), per-channel ratio (Bn,3), PSNR (Bn) (0 without a target)."""
    q = pred[:, :, :h, :w].clamp(0, 1)
    t = None if target is None else target.repeat_interleave(spi, 0)
    ratio = torch.ones(q.shape[:2], dtype=q.dtype)
    if gt_mean:
        ratio = t.mean((2, 3)) / q.mean((2, 3))
        q = _zero_for_nan((q * ratio[:, :, None, None]).clamp(0, 1), zero_sum)
    return q, ratio, (torch.zeros(q.shape[0], dtype=q.dtype) if t is None else psnr(t, q))


def to_levels(x):
    """img_as_ubyte's values: rint(255 clamp(x, 0, 1)), half to even, in x's dtype."""
    return torch.round(x.clamp(0, 1) * 255.0)


def ssim(final, target, spi):
    """calculate_ssim(img_as_ubyte(target), img_as_ubyte(final)) per candidate: 11x11 Gaussian (sigma 1.5) over the valid region, per
    channel, mean over region and channels.  final (Bn,3,h,w), target (B,3,h,w) -> (Bn)."""
    Bn, _, h, w = final.shape
    dt = final.dtype
    g = torch.exp(-((torch.arange(11, dtype=dt) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    a = to_levels(target).repeat_interleave(spi, 0).reshape(Bn * 3, 1, h, w)
    b = to_levels(final).reshape(Bn * 3, 1, h, w)
    f = lambda z: F.conv2d(F.conv2d(z, g.reshape(1, 1, 11, 1)), g.reshape(1, 1, 1, 11))      # the window is the outer product g g^T
    mu1, mu2 = f(a), f(b)
    s1, s2, s12 = f(a * a) - mu1 * mu1, f(b * b) - mu2 * mu2, f(a * b) - mu1 * mu2
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return m.reshape(Bn, -1).mean(1)


GRAY = (0.114, 0.587, 0.299)        # COLOR_BGR2GRAY on the channel order as stored


def mc_mean(raw, target, spi, h, w, gt_mean):
    """clamp(mean_n clamp(raw_n[:h,:w])); with gt_mean the image times mean(gray(target)) / mean(gray(mc)), clamped.  The N candidates
    are added one after the other, as numpy's mean over a leading axis does: in float32 that is the reference's own rounding."""
    Bn = raw.shape[0]
    c = raw[:, :, :h, :w].clamp(0, 1).reshape(Bn // spi, spi, 3, h, w)
    acc = torch.zeros_like(c[:, 0])
    for n in range(spi):
        acc = acc + c[:, n]
    mc = (acc / spi).clamp(0, 1)
    if gt_mean:
        wts = torch.tensor(GRAY, dtype=raw.dtype).reshape(1, 3, 1, 1)
        ratio = (target * wts).sum(1).mean((1, 2)) / (mc * wts).sum(1).mean((1, 2))
        mc = (mc * ratio[:, None, None, None]).clamp(0, 1)
    return mc


def _scores(s1, s2, weight):
    """The reference's list arithmetic: weight s1 / max(s1) + (1 - weight) s2 / max(s2), Python's max, numpy's division."""
    with np.errstate(all="ignore"):
        if s2 is None:
            return (np.array(s1, dtype=np.float64) / max(s1)).tolist()
        return (weight * np.array(s1, dtype=np.float64) / max(s1) + (1 - weight) * np.array(s2, dtype=np.float64) / max(s2)).tolist()


def select_best(psnr_row):
    """Index of the first maximum of psnr / max(psnr), with Python-list semantics (also for NaN: max keeps its first argument when no
    later one compares greater, and list.index finds that very object)."""
    sc = _scores([float(v) for v in psnr_row], None, 1.0)
    return sc.index(max(sc))


def select_scores(s1_row, s2_row=None, weight=1.0, rule="weighted"):
    s1 = [float(v) for v in s1_row]
    if rule == "max":
        return s1.index(max(s1))
    if rule == "min":
        return s1.index(min(s1))
    sc = _scores(s1, None if s2_row is None else [float(v) for v in s2_row], weight)
    return sc.index(max(sc))


def ranked(s1_row, s2_row=None, weight=1.0, rule="weighted"):
    """The scores the rule compares, larger = better, as a float64 tensor (for the gap conditions)."""
    s1 = [float(v) for v in s1_row]
    if rule == "max":
        return torch.tensor(s1, dtype=torch.float64)
    if rule == "min":
        return -torch.tensor(s1, dtype=torch.float64)
    return torch.tensor(_scores(s1, None if s2_row is None else [float(v) for v in s2_row], weight), dtype=torch.float64)


def gap(scores):
    """Best minus runner-up."""
    top = torch.sort(scores, descending=True)[0]
    return float(top[0] - top[1])


def weighted_score_error(s1_row, e1, s2_row=None, e2=0.0, weight=1.0):
    """Largest change of weight s1/max(s1) + (1-weight) s2/max(s2) when every s1 moves by at most e1 and every s2 by e2:
    |d(s/m)| <= e/|m| + |s| e/m^2 <= 2 e/|m| for |s| <= |m| (positive scores)."""
    m1 = max(abs(float(v)) for v in s1_row)
    if s2_row is None:
        return 2 * e1 / m1
    m2 = max(abs(float(v)) for v in s2_row)
    return weight * 2 * e1 / m1 + (1 - weight) * 2 * e2 / m2


# ------------------------------------------------------------------------------------------------------------------ shape tables
# (h, w, Hp, Wp, B, N); CF_CHUNK = 4096 pixels per workgroup
FINALIZE = {
    "one-chunk": (64, 64, 64, 64, 1, 2),
    "4097": (17, 241, 32, 256, 2, 3),
    "ragged-n64": (61, 203, 64, 256, 2, 64),
    "sub-wave": (5, 7, 16, 16, 1, 64),
    "degenerate": (1, 1, 16, 16, 2, 2),
}
FINALIZE_SEED = {"one-chunk": 101, "4097": 102, "ragged-n64": 110, "sub-wave": 104, "degenerate": 105}
COMPOSITE = "ragged-n64"

# (h, w, Hp, Wp, B, N); the grid is min(cdiv(hw, 256), 256) workgroups per (image, channel)
MC_MEAN = {
    "256-groups": (256, 256, 256, 256, 1, 2),
    "second-pass": (259, 254, 272, 256, 2, 3),
    "n64": (21, 27, 24, 32, 2, 64),
    "degenerate": (1, 1, 8, 8, 1, 1),
}

COND_PLANES = [(4, 5), (16, 16), (1, 257), (28, 40)]          # hw = 20, 256, 257, 1120
COND_BN = [(1, 1), (2, 64)]

# (B, N, h, w)
SSIM = {
    "1x2-tiles": (1, 2, 26, 42),
    "one-pixel": (1, 1, 11, 11),
    "one-wide": (1, 2, 75, 11),
    "n64": (2, 64, 12, 12),
}

PADS = [(33, 17, 64, 32), (5, 9, 8, 16), (64, 50, 64, 64), (100, 150, 128, 192)]
RESIZE = [(64, 128, 2), (64, 128, 4), (64, 128, 16), (32, 16, 16)]
BILINEAR = [(1, 1), (1, 5), (5, 1), (28, 40)]


# ------------------------------------------------------------------------------------------------------------------ input builders
def two_targets(g, B, h, w):
    """Targets in [0,1] whose means differ by 0.55 from image to image: a candidate scored against the other image's target is far off."""
    return torch.stack([0.05 + 0.55 * (b % 2) + 0.35 * torch.rand(3, h, w, generator=g) for b in range(B)])


def finalize_inputs(name, exact_candidate=None):
    """pred (B N,3,Hp,Wp) = 0.4 N(0,1) + 0.5 (both clamps act), target (B,3,h,w).  exact_candidate: that candidate's crop is its target."""
    h, w, Hp, Wp, B, N = FINALIZE[name]
    g = gen(FINALIZE_SEED[name])
    pred = 0.4 * torch.randn(B * N, 3, Hp, Wp, generator=g) + 0.5
    target = two_targets(g, B, h, w)
    if exact_candidate is not None:
        pred[exact_candidate, :, :h, :w] = target[exact_candidate // N]
    return pred, target


def psnr_f32_term(pred, target, spi, h, w, gt_mean):
    """Worst |PSNR(float32 evaluation) - PSNR(float64)| over the candidates of a case: what rounding the final image to float32 pixels and
    its ratio to a float32 number costs.  The float32 evaluation is the oracle's numpy path (float32 arrays, as eval.py holds them)."""
    from oracle import bem_oracle as O
    p64 = candidate_finalize(pred.double(), target.double(), spi, h, w, gt_mean)[2]
    worst = 0.0
    for i in range(pred.shape[0]):
        q = np.clip(pred[i, :, :h, :w].permute(1, 2, 0).numpy(), 0, 1)
        t = target[i // spi].permute(1, 2, 0).numpy()
        if gt_mean:
            q = np.clip(q * (t.mean(axis=(0, 1), keepdims=True) / q.mean(axis=(0, 1), keepdims=True)), 0, 1)
        worst = max(worst, abs(O.psnr_ref(t, q) - float(p64[i])))
    return worst


def psnr_bound(p64, f32_term):
    """Admitted |PSNR - float64| per candidate: one float32 ulp of the value, plus MARGIN x the float32 term where there is one."""
    return ulp32(p64) + MARGIN * f32_term


def composite_reference(pred, target, N, h, w):
    """float64 PSNR and SSIM of every candidate, with the error each GPU figure may carry."""
    fin64, _, p64 = candidate_finalize(pred.double(), target.double(), N, h, w, True)
    fin32 = candidate_finalize(pred, target, N, h, w, True)[0]
    s64 = ssim(fin64, target.double(), N)
    s32 = ssim(fin32.double(), target.double(), N)                  # float32 finals: what the quantisation to levels makes of their rounding
    return {"psnr": p64, "ssim": s64, "psnr_bound": psnr_bound(p64, psnr_f32_term(pred, target, N, h, w, True)),
            "ssim_bound": ulp32(s64) + MARGIN * float((s32 - s64).abs().max())}


def mc_inputs(name):
    h, w, Hp, Wp, B, N = MC_MEAN[name]
    g = gen(200 + sum(map(ord, name)))
    raw = 0.4 * torch.randn(B * N, 3, Hp, Wp, generator=g) + 0.5
    return raw, two_targets(g, B, h, w)


def ssim_inputs(name):
    """Target and candidates on the levels k / 255: 255 x is then within 1e-4 of the integer k in float32 and in float64, never near a half."""
    B, N, h, w = SSIM[name]
    g = gen(300 + sum(map(ord, name)))
    kt = torch.randint(0, 256, (B, 3, h, w), generator=g)
    kf = (kt[:, None] + torch.randint(-25, 26, (B, N, 3, h, w), generator=g)).clamp(0, 255).reshape(B * N, 3, h, w)
    return kf.float() / 255.0, kt.float() / 255.0


def select_rows(name):
    """(psnr (B,N), ssim (B,N), {row: 'tie'}) float32 score tables.  Rows marked 'tie' carry a bit-equal maximum twice, on purpose."""
    g = gen(400 + sum(map(ord, name)))
    ties = {}
    if name == "n64":
        B, N = 3, 64
    elif name == "b65":
        B, N = 65, 2
    else:
        B, N = 7, 5
    ps = torch.rand(B, N, generator=g) * 10 + 15
    ss = torch.rand(B, N, generator=g) * 0.3 + 0.6
    if name == "edges":
        ps[0] = 0.0                                            # all-zero PSNRs: 0 / 0, every score NaN, index 0
        ss[0] = ss[0, 0]
        ties[0] = "tie"
        ps[1, 2] = 100.0                                       # an exact candidate
        ps[2, 0] = ps[2, 3] = ps[2].max() + 1.0                # tie at the first index
        ss[2, 0] = ss[2, 3] = ss[2].max() + 0.05
        ties[2] = "tie"
        ps[3, 1] = ps[3, N - 1] = ps[3].max() + 1.0            # tie that ends at the last index
        ss[3, 1] = ss[3, N - 1] = ss[3].max() + 0.05
        ties[3] = "tie"
        ps[4] = -ps[4]                                         # negative PSNRs: dividing by a negative maximum reverses the order
    return ps, ss, ties


SELECT_CASES = ["n64", "b65", "edges"]
SELECT_RULES = [("weighted", 1.0), ("weighted", 0.5), ("weighted", 0.0), ("max", 1.0), ("min", 1.0)]
