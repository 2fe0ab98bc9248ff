"""Plain-torch references of the kernels in csrc/attn_blocks.hip (not collected by pytest), one function per entry point, written from the
formulas in that file's header comments and basicsr/archs/DecompModel_arch.py:57-99.  Nothing here imports bem.

Every function is dtype-generic: called on float64 CPU tensors it is the yardstick, called on the same values in float32 it is the "f32
reference" whose own distance from float64 sets the bounds of tests/test_attn_blocks_gpu.py.  The backwards are torch autograd through
these forwards.  Reductions also return the sum of the absolute values of their terms, the scale their rounding error is measured on.
"""
import torch
import torch.nn.functional as F

# (B, C, Cr, H, W): the shape grid of the GPU tests
SHAPES = {
    "shipped-train": (2, 160, 10, 32, 32),        # Options/DecompDualBranch_4.yml: n_feat 40, gt_size 128, plane / 4
    "shipped-eval-256": (1, 160, 10, 64, 64),
    "config5-eval": (1, 160, 10, 112, 160),       # 400x600 padded to 448x640, / 4
    "fixture-width": (3, 64, 4, 9, 7),
    "ragged": (2, 5, 3, 3, 11),                   # Cr % 4 != 0, C < 64
    "thread-loop": (1, 300, 18, 4, 5),            # C > 256: two thread passes, five lane passes
    "degenerate": (1, 16, 1, 1, 1),
    "narrow-h": (2, 8, 2, 2, 50),                 # narrower than the 7x7 radius in one dimension
    "narrow-w": (2, 8, 2, 50, 2),
    "over-256-pixels": (3, 24, 6, 17, 19),
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0):
    """float32 values (what the kernels are given); .double() of them is what the float64 reference is given."""
    return torch.randn(*shape, generator=g) * scale


def quantised(g, *shape, levels=3):
    """Multiples of 1/4 in [-1/4 * (levels // 2), ...]: exact in f32 and f64, and tied along any axis of a few entries."""
    return (torch.randint(0, levels, shape, generator=g).float() - levels // 2) * 0.25


def tie_fraction(x):
    """Fraction of the (b, y, x) pixels whose channel maximum is reached by more than one channel."""
    return float(((x == x.max(1, keepdim=True)[0]).sum(1) > 1).double().mean())


# ------------------------------------------------------------------------------------------------------------------ forwards
def plane_mean(x):
    """(B,C,H,W) -> (B,C); also sum |x| / HW."""
    return x.mean((2, 3)), x.abs().mean((2, 3))


def se_gate(mean, w1, w2):
    """sigmoid(W2 relu(W1 mean)): mean (B,C), w1 (Cr,C), w2 (C,Cr) -> (B,C)."""
    return torch.sigmoid(torch.relu(mean @ w1.t()) @ w2.t())


def spatial_attention(x, w, chan_scale=None, parts=False):
    """xs * sigmoid(conv_kxk([mean_c xs, max_c xs], zero padding k // 2)) with xs = x * chan_scale[b][c]; w (1,2,k,k).
    parts: also the (B,2,H,W) map and the pre-sigmoid plane (B,1,H,W)."""
    xs = x if chan_scale is None else x * chan_scale[:, :, None, None]
    amap = torch.cat([xs.mean(1, keepdim=True), xs.max(1, keepdim=True)[0]], 1)
    pre = F.conv2d(amap, w, padding=w.shape[-1] // 2)
    out = xs * torch.sigmoid(pre)
    return (out, amap, pre) if parts else out


def row_scale(w, scale):
    """w (M, ...) * scale (M) along the first axis."""
    return w * scale.reshape(-1, *([1] * (w.dim() - 1)))


def chan_scale(x, scale, add=None, add_bc=None, add_bc_scale=1.0):
    """scale[(b,) c] * x (+ add) (+ add_bc[b][c] * add_bc_scale); scale with C elements (a parameter) or (B,C) (per image)."""
    B, C = x.shape[:2]
    s = scale.reshape(B, C, 1, 1) if tuple(scale.shape) == (B, C) else scale.reshape(1, C, 1, 1)
    out = s * x
    if add is not None:
        out = out + add
    if add_bc is not None:
        out = out + (add_bc * add_bc_scale)[:, :, None, None]
    return out


def chan_dot(a, b, per_image=True):
    """per_image: (B,C) = sum_p a b; otherwise (C) = sum_{b,p} a b (what the kernel adds to a parameter's gradient).  Also sum |a b|."""
    dims = (2, 3) if per_image else (0, 2, 3)
    t = a * b
    return t.sum(dims), t.abs().sum(dims)


# ------------------------------------------------------------------------------------------------------------------ backwards
def se_gate_bwd(mean, w1, w2, dy):
    """Autograd of se_gate: returns {dmean, dw1, dw2} and, under the same keys + '_abs', the sums of absolute terms of each one's last
    reduction (dmean[b][c] = sum_r W1[r][c] dz1[b][r]; dW1[r][c] = sum_b dz1[b][r] m[b][c]; dW2[c][r] = sum_b dz2[b][c] h[b][r])."""
    mean, w1, w2 = (t.detach().clone().requires_grad_() for t in (mean, w1, w2))
    z1 = mean @ w1.t()
    h = torch.relu(z1)
    z2 = h @ w2.t()
    y = torch.sigmoid(z2)
    dmean, dw1, dw2, dz1, dz2 = torch.autograd.grad(y, [mean, w1, w2, z1, z2], dy)
    with torch.no_grad():
        return {"y": y.detach(), "dmean": dmean, "dw1": dw1, "dw2": dw2,
                "dmean_abs": dz1.abs() @ w1.abs(), "dw1_abs": dz1.abs().t() @ mean.abs(), "dw2_abs": dz2.abs().t() @ h.abs()}


def spatial_attention_bwd(x, w, dout):
    """Autograd of spatial_attention(x, w): {out, dx, dw, dw_abs}; dw[ch][dy][dx] = sum_{b,p} map[b][ch][p + tap] dpre[b][p], dw_abs the
    same sum over absolute values.  The max branch's gradient goes where torch.max(dim) points: the first maximal channel."""
    x, w = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    out, amap, pre = spatial_attention(x, w, parts=True)
    dx, dw, dpre = torch.autograd.grad(out, [x, w, pre], dout)
    k = w.shape[-1]
    with torch.no_grad():
        B = x.shape[0]
        cols = F.unfold(amap.abs(), k, padding=k // 2)                         # (B, 2 k k, HW)
        dw_abs = (cols * dpre.abs().reshape(B, 1, -1)).sum((0, 2)).reshape(1, 2, k, k)
    return {"out": out.detach(), "dx": dx, "dw": dw, "dw_abs": dw_abs}


def saturating_weight(x, w, target=100.0, chan_scale=None):
    """w rescaled (in float64, returned as float32) so that the pre-sigmoid plane of spatial_attention(x, w) reaches about +-target."""
    _, _, pre = spatial_attention(x.double(), w.double(), None if chan_scale is None else chan_scale.double(), parts=True)
    return (w.double() * (target / float(pre.abs().max()))).float()
