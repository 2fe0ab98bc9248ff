"""torch-CPU restatement of the four per-pixel statistics of CombinedLoss (basicsr/losses/my_loss.py:51-74) and of their weighted sum,
in any dtype, written from the formulas: the checker of csrc/pixstat_loss.hip.  With d = pred - gt, n elements, B samples:
    smooth_l1 = mean(0.5 d^2 where |d| < 1, |d| - 0.5 elsewhere)
    mse = mean d^2,   psnr = 40 - 20 log10(1 / sqrt(mse))
    color = mean_b |mean(gt_b) - mean(pred_b)|
    hist = mean_k |h_gt[k] / sum h_gt - h_pred[k] / sum h_pred|,   h = torch.histc(x, 256, 0, 1)   (no gradient)
    loss = a1 smooth_l1 + a3 hist + a5 psnr + a6 color, a term with a zero alpha left out
and the ``l2`` perceptual term (sum over layers of layer_weight * mean (f(x) - f(gt))^2, times perceptual_weight) over tests/vgg_ref.py's
feature extractor.  The product package never imports it."""
import torch

import vgg_ref

VALUES = ("loss", "smooth_l1", "mse", "psnr", "color", "hist")
ALPHAS = (1.00, 0.05, 0.0083, 0.25)                      # alpha1, alpha3, alpha5, alpha6 of my_loss.py:55-60
BINS = 256


def pair(shape, seed):
    """(pred, gt) f32: gt uniform in [0,1], pred = gt + 0.1 randn (unclamped, as a network's output is), and where the tensors are large
    enough a planted set of values at fixed flat positions: exact 0 and 1, bin edges k/256 and the float just below them, values below 0
    and above 1, and pairs with |d| > 1 (pred 2.3, -1.2 against gt 0.1, 0.9: the linear branch of smooth-L1)."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    pred = gt + 0.1 * torch.randn(shape, generator=g)
    n = gt.numel()
    edges = torch.tensor([1, 2, 77, 128, 200, 255], dtype=torch.float32) / BINS
    special = torch.cat([torch.tensor([0.0, 1.0, -0.0]), edges, torch.nextafter(edges, torch.zeros(())), torch.tensor([-0.25, -1e-9, 1.0 + 2 ** -23, 1.7])])
    if n >= 4 * special.numel():
        at = torch.arange(special.numel()) * (n // special.numel())
        pred.view(-1)[at] = special
        gt.view(-1)[at + 1] = special.clamp(0, 1)
        pred.view(-1)[at[:2] + 2] = torch.tensor([2.3, -1.2])
        gt.view(-1)[at[:2] + 2] = torch.tensor([0.1, 0.9])
    return pred, gt


def counts(x):
    """torch.histc(x, 256, 0, 1) of an f32 tensor as int64 counts."""
    return torch.histc(x.detach().float().cpu(), bins=BINS, min=0.0, max=1.0).to(torch.int64)


def values(pred, gt, alphas=ALPHAS, dtype=torch.float64):
    """{name: 0-d tensor in dtype} for VALUES; differentiable in pred."""
    pred, gt = pred.to(dtype), gt.to(dtype)
    a1, a3, a5, a6 = alphas
    d = pred - gt
    ad = d.abs()
    sl1 = torch.where(ad < 1, 0.5 * d * d, ad - 0.5).mean()
    mse = (d * d).mean()
    psnr = 40.0 - 20.0 * torch.log10(1.0 / torch.sqrt(mse))
    color = (gt.mean(dim=(1, 2, 3)) - pred.mean(dim=(1, 2, 3))).abs().mean()
    hp, hg = (torch.histc(t.detach(), bins=BINS, min=0.0, max=1.0) for t in (pred, gt))
    hist = (hg / hg.sum() - hp / hp.sum()).abs().mean()
    loss = sum(a * v for a, v in ((a1, sl1), (a3, hist), (a5, psnr), (a6, color)) if a != 0)
    return dict(loss=loss, smooth_l1=sl1, mse=mse, psnr=psnr, color=color, hist=hist)


def loss_and_grad(pred, gt, alphas=ALPHAS, dtype=torch.float64):
    """(values as a (6,) tensor in VALUES' order, d loss / d pred), computed in ``dtype`` on the CPU."""
    x = pred.detach().to(dtype).requires_grad_(True)
    v = values(x, gt.detach(), alphas, dtype)
    (g,) = torch.autograd.grad(v["loss"], x) if v["loss"].requires_grad else (torch.zeros_like(x),)
    return torch.stack([v[k].detach() for k in VALUES]), g


def perceptual_l2(sd, x, gt, layer_weights, perceptual_weight=1.0, **norm):
    fx, fg = vgg_ref.features(sd, x, layer_weights, **norm), vgg_ref.features(sd, gt, layer_weights, **norm)
    total = 0
    for k, w in layer_weights.items():
        total = total + ((fx[k] - fg[k]) ** 2).mean() * w
    return total * perceptual_weight


def perceptual_l2_loss_and_grad(sd, x, gt, layer_weights, perceptual_weight=1.0, dtype=torch.float64, **norm):
    x = x.detach().to(dtype).requires_grad_(True)
    sd = {k: v.to(dtype) for k, v in sd.items()}
    loss = perceptual_l2(sd, x, gt.detach().to(dtype), layer_weights, perceptual_weight, **norm)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g
