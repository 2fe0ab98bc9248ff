"""The N-state SS2D scan in the operand layout of bem_ss2d_scan_n_f32, restated in torch for any dtype (float64 for the error yardstick,
float32 for the oracle's own rounding) and differentiable (the backward tests take autograd through it).

  x0, x1 (B,C,L)        activations, row-major / transposed pixel order
  xd0, xd1 (B,2,R+2N,L) x_dbl rows [dt | B_0..B_{N-1} | C_0..C_{N-1}] of directions {0,2} / {1,3}
  dtw (4,C,R), dtb (4,C), A_logs (4C,N), Ds (4C)
  returns y0, y1 (B,C,L): y(dir 0) + y(dir 2), y(dir 1) + y(dir 3)
Per direction: dl = softplus(dt_row . dtw + dtb), h_n = exp(dl A_n) h_n + dl B_n x, y = sum_n C_n h_n + D x, the reverse directions
scanning from the last position (vmamba.py:657-684 with the cross scan / merge folded into the layout)."""
import torch
import torch.nn.functional as F


def _scan(x, rows, w, b, A, D, rev):
    R = w.shape[1]
    N = A.shape[1]
    dts, Bs, Cs = rows[:, :R], rows[:, R:R + N], rows[:, R + N:]
    if rev:
        x, dts, Bs, Cs = x.flip(-1), dts.flip(-1), Bs.flip(-1), Cs.flip(-1)
    dl = F.softplus(torch.einsum("brl,cr->bcl", dts, w) + b[None, :, None])
    dA = torch.exp(dl[:, :, None, :] * A[None, :, :, None])          # (B,C,N,L)
    dBu = (dl * x)[:, :, None, :] * Bs[:, None, :, :]
    h = torch.zeros(x.shape[0], x.shape[1], N, dtype=x.dtype)
    ys = []
    for t in range(x.shape[-1]):
        h = dA[..., t] * h + dBu[..., t]
        ys.append((h * Cs[:, None, :, t]).sum(-1))
    y = torch.stack(ys, -1) + D[None, :, None] * x
    return y.flip(-1) if rev else y


def ss2d_scan_n_ref(x0, x1, xd0, xd1, dtw, dtb, A_logs, Ds, dtype=torch.float64):
    cv = lambda t: t.detach().cpu().to(dtype) if not t.requires_grad else t.cpu().to(dtype)
    x0, x1, xd0, xd1, dtw, dtb, A_logs, Ds = map(cv, (x0, x1, xd0, xd1, dtw, dtb, A_logs, Ds))
    C = x0.shape[1]
    A = -torch.exp(A_logs)
    out = []
    for o, (x, xd) in enumerate(((x0, xd0), (x1, xd1))):
        y = 0
        for d in (0, 1):
            k = o + 2 * d
            y = y + _scan(x, xd[:, d], dtw[k], dtb[k], A[k * C:(k + 1) * C], Ds[k * C:(k + 1) * C], d == 1)
        out.append(y)
    return out[0], out[1]


def make_operands(B, C, H, W, N, seed, dev="cpu"):
    """x (B,C,H,W) and SS2D parameters drawn so that the state term carries the output: dl in (0.05, 1), Ds ~ 0.1 N(0,1), B / C rows
    of order 1 (the trivial init would leave C h at the f32 rounding floor of D x, see tests/stage2_yardstick.py)."""
    g = torch.Generator().manual_seed(seed)
    R = max(1, -(-C // 16))
    M = R + 2 * N
    x = torch.randn(B, C, H, W, generator=g)
    xw = 0.3 * torch.randn(4, M, C, generator=g)
    dtw = 0.2 * torch.randn(4, C, R, generator=g)
    dt = 0.05 + 0.95 * torch.rand(4, C, generator=g)
    dtb = dt + torch.log(-torch.expm1(-dt))
    A_logs = torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(4 * C, 1) + 0.1 * torch.randn(4 * C, N, generator=g)
    Ds = 0.1 * torch.randn(4 * C, generator=g)
    return x, xw, dtw, dtb, A_logs, Ds


def x_dbl(x, xw):
    """(x0, x1, xd0, xd1) of the kernel layout from x (B,C,H,W) and x_proj_weight (4, R+2N, C), in float32."""
    B, C, H, W = x.shape
    x0 = x.reshape(B, C, H * W).contiguous()
    x1 = x.transpose(2, 3).reshape(B, C, H * W).contiguous()
    xd0 = torch.stack([torch.einsum("bcl,jc->bjl", x0, xw[0]), torch.einsum("bcl,jc->bjl", x0, xw[2])], 1).contiguous()
    xd1 = torch.stack([torch.einsum("bcl,jc->bjl", x1, xw[1]), torch.einsum("bcl,jc->bjl", x1, xw[3])], 1).contiguous()
    return x0, x1, xd0, xd1


def merge(y0, y1, H, W):
    """y0 (row-major) + y1 (transposed order) -> (B,C,H,W)."""
    B, C, _ = y0.shape
    return y0.reshape(B, C, H, W) + y1.reshape(B, C, W, H).transpose(2, 3)
