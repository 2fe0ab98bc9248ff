"""torch-CPU restatement of the LPIPS loss term and of the three pieces its HIP backward is made of, in any dtype: the checker of
bem.autograd.LPIPSFn, on top of the metric's restatement tests/lpips_ref.py.  The product package never imports it.

The loss is ``weight * mean_b d(gt_b, pred_b)`` on images in [0,1] (``2 x - 1`` applied, no quantisation); its gradient is torch's
autograd of that expression.  The pieces: the closed-form gradient of one layer's head, the first-maximum gather of MaxPool2d(3, 2)
and the index map that takes the gradient of conv1's block-form operand back to the image."""
import torch
import torch.nn.functional as F

import lpips_ref as R

EPS = 1e-10


def loss_and_grad(sd, lin, pred01, gt01, weight, dtype=torch.float64):
    """(loss, d loss / d pred01) of weight * R.lpips(sd, lin, 2 gt - 1, 2 pred - 1, dtype).mean(), both in ``dtype``."""
    pred = pred01.detach().to(dtype).clone().requires_grad_(True)
    loss = weight * R.lpips(sd, lin, 2 * gt01.to(dtype) - 1, 2 * pred - 1, dtype).mean()
    (g,) = torch.autograd.grad(loss, pred)
    return loss.detach(), g


# ------------------------------------------------------------------------------ one layer's head
def safe_norm(y):
    """sqrt(sum_c y^2) over dim 1, keepdim, with derivative 0 (not NaN) where the sum is 0."""
    ss = y.pow(2).sum(1, keepdim=True)
    pos = ss > 0
    return torch.where(pos, torch.where(pos, ss, torch.ones_like(ss)).sqrt(), torch.zeros_like(ss))


def head_safe(y0, y1, w):
    """R.head with the safe norm: the same value everywhere, and a finite gradient at pixels whose features are all zero."""
    n0, n1 = y0 / (safe_norm(y0) + EPS), y1 / (safe_norm(y1) + EPS)
    return ((n0 - n1).pow(2) * w.to(y0.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def head_grad(y0, y1, w):
    """d head(y0, y1, w).sum() / d y1 in closed form: with n = |y|, r = 1 / (n + eps), a = y0 r0, b = y1 r1, D = -2 w (a - b):
    g_k = r1 D_k - y1_k (r1 / n1) sum_c b_c D_c, the second term 0 where n1 = 0; divided by the number of pixels."""
    n0, n1 = y0.pow(2).sum(1, keepdim=True).sqrt(), y1.pow(2).sum(1, keepdim=True).sqrt()
    r0, r1 = 1 / (n0 + EPS), 1 / (n1 + EPS)
    b = y1 * r1
    D = -2 * w.to(y0.dtype).view(1, -1, 1, 1) * (y0 * r0 - b)
    q = torch.where(n1 > 0, r1 / torch.where(n1 > 0, n1, torch.ones_like(n1)), torch.zeros_like(n1))
    return (r1 * D - y1 * q * (b * D).sum(1, keepdim=True)) / (y0.shape[2] * y0.shape[3])


def head_bwd(feat, w, gin=None, factor=1.0):
    """What bem_lpips_layer_bwd_f32 returns for feat (2B,C,h,w): (y_pred > 0) ? gin + factor * head_grad : 0, in the dtype of feat."""
    B = feat.shape[0] // 2
    g = factor * head_grad(feat[:B], feat[B:], w)
    if gin is not None:
        g = g + gin.to(feat.dtype)
    return torch.where(feat[B:] > 0, g, torch.zeros_like(g))


# ------------------------------------------------------------------------------ MaxPool2d(3, 2)
def pool_bwd(y, dpool):
    """Gradient of F.max_pool2d(y, 3, 2) by gathering: every window gives its dpool to its first maximum in row-major order."""
    Bn, C, H, W = y.shape
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    win = y.unfold(2, 3, 2).unfold(3, 3, 2).reshape(Bn, C, Ho, Wo, 9)
    eq = win == win.max(-1, keepdim=True).values
    first = eq & (eq.cumsum(-1) == 1)
    cols = (first.to(y.dtype) * dpool.to(y.dtype).unsqueeze(-1)).permute(0, 1, 4, 2, 3).reshape(Bn, C * 9, Ho * Wo)
    hc, wc = 2 * (Ho - 1) + 3, 2 * (Wo - 1) + 3
    out = torch.zeros_like(y)
    out[:, :, :hc, :wc] = F.fold(cols, (hc, wc), 3, stride=2)
    return out


# ------------------------------------------------------------------------------ conv1's block form
def block_hw(H, W):
    """(Hb, Wb) of the block grid conv1 reads: its output size plus 2, the width rounded up to even."""
    Ho, Wo = R.sizes(H)[0], R.sizes(W)[0]
    return Ho + 2, (Wo + 3) // 2 * 2


def unblock_grad(gxs, H, W, k=1.0, scale=None):
    """dpred[b,c,y,x] = k * gxs[b, 16 c + 4 ((y+2) % 4) + (x+2) % 4, (y+2) // 4, (x+2) // 4] / scale_c by index arithmetic."""
    y, x = torch.arange(H).view(1, H, 1) + 2, torch.arange(W).view(1, 1, W) + 2
    ch = 16 * torch.arange(3).view(3, 1, 1) + 4 * (y % 4) + x % 4
    g = k * gxs[:, ch, (y // 4).expand(3, H, W), (x // 4).expand(3, H, W)]
    return g if scale is None else g / scale.view(1, 3, 1, 1)


POOL_SIZES = [(3, 3), (7, 7), (8, 12), (9, 10), (15, 15)]


def tied_pool_case(H, W, planes=(2, 3)):
    """(y, dpool) full of ties: y in multiples of 0.25 from five values (a ReLU output: many zeros), dpool small integers, so every
    sum of the backward is exact in f32 and implementations compare with torch.equal."""
    g = torch.Generator().manual_seed(H * 100 + W)
    y = torch.randint(0, 5, planes + (H, W), generator=g).float() * 0.25
    dpool = torch.randint(-8, 9, planes + ((H - 3) // 2 + 1, (W - 3) // 2 + 1), generator=g).float()
    return y, dpool
