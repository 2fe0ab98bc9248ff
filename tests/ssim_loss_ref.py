"""The SSIM loss of Stage-II training restated in torch on the CPU, parametrised by dtype: the yardstick of test_ssim_loss_cpu.py and
test_ssim_loss_gpu.py (float64) and the f32 form whose own error sets their tolerance.

Definition (basicsr/losses/my_loss.py:37-38, 1 - pytorch_msssim.ssim(y_true, y_pred, data_range=1.0, size_average=True)): every (b,c)
plane on its own, the normalised 11-tap Gaussian g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) applied separably, rows then columns, over the
valid region only, C1 = 0.01^2, C2 = 0.03^2, mean over all B * C * (H - 10) * (W - 10) positions.  ``loss`` goes through autograd;
``grad_formula`` is the hand-written gradient the HIP backward implements."""
import torch
import torch.nn.functional as F

WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype):
    """The taps in float64, rounded to dtype (the kernel's table is the float32 rounding of the same values)."""
    i = torch.arange(WIN, dtype=torch.float64) - WIN // 2
    g = torch.exp(-i * i / (2 * SIGMA * SIGMA))
    return (g / g.sum()).to(dtype)


def _filt(x, g):
    """Valid-region separable filter of (B,C,H,W): along the rows (W) first, then along the columns (H)."""
    C = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, 1, WIN).expand(C, 1, 1, WIN), groups=C)
    return F.conv2d(x, g.view(1, 1, WIN, 1).expand(C, 1, WIN, 1), groups=C)


def _filt_t(a, g):
    """The transposed (full) correlation: a valid-region map back to H x W."""
    C = a.shape[1]
    a = F.conv_transpose2d(a, g.view(1, 1, WIN, 1).expand(C, 1, WIN, 1), groups=C)
    return F.conv_transpose2d(a, g.view(1, 1, 1, WIN).expand(C, 1, 1, WIN), groups=C)


def _maps(x, y, g):
    m1, my = _filt(x, g), _filt(y, g)
    m2, my2, m12 = _filt(x * x, g), _filt(y * y, g), _filt(x * y, g)
    A1, A2 = 2 * m1 * my + C1, 2 * (m12 - m1 * my) + C2
    B1, B2 = m1 * m1 + my * my + C1, (m2 - m1 * m1) + (my2 - my * my) + C2
    return m1, my, A1, A2, B1, B2


def ssim_map(pred, gt, dtype=torch.float64):
    """S on the valid region, (B,C,H-10,W-10) of dtype: the values the loss averages."""
    _, _, A1, A2, B1, B2 = _maps(pred.to(dtype), gt.to(dtype), window(dtype))
    return A1 * A2 / (B1 * B2)


def loss(pred, gt, weight=1.0, dtype=torch.float64):
    """weight * (1 - mean S) as a 0-dim tensor of dtype; differentiable in pred."""
    return weight * (1 - ssim_map(pred, gt, dtype).mean())


def loss_and_grad(pred, gt, weight=1.0, dtype=torch.float64):
    """(loss, dloss/dpred) through autograd, both of dtype."""
    x = pred.detach().to(dtype).requires_grad_(True)
    l = loss(x, gt, weight, dtype)
    l.backward()
    return l.detach(), x.grad


def grad_formula(pred, gt, weight=1.0, dtype=torch.float64):
    """dloss/dpred = -(weight / Npos) (G^T a + 2 x G^T b + y G^T c) with the three coefficient maps on the valid region."""
    x, y, g = pred.detach().to(dtype), gt.to(dtype), window(dtype)
    m1, my, A1, A2, B1, B2 = _maps(x, y, g)
    S = A1 * A2 / (B1 * B2)
    b = -S / B2
    c = 2 * A1 / (B1 * B2)
    a = 2 * my * (A2 - A1) / (B1 * B2) - 2 * m1 * S * (1 / B1 - 1 / B2)
    return -(weight / S.numel()) * (_filt_t(a, g) + 2 * x * _filt_t(b, g) + y * _filt_t(c, g))


def pair(shape, seed):
    """The inputs of the tests: gt = rand, pred = clamp(gt + 0.1 randn, 0, 1), seeded."""
    gen = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=gen)
    return (gt + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1), gt
