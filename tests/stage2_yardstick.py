"""Helpers for the Stage-II parity tests that must see the selective-scan recurrence (not collected by pytest).

* `recurrence_dominated(sd, seed)` re-draws a Stage-II state dict in place so that every block reaches the output: at
  initialisation (Ds = 1, dt ~ 0.001 .. 0.1) each scan returns almost exactly D*u and its state term C*h sits at the f32
  rounding floor of the net's output.
* `ss2d_core64` / `iwt64` evaluate the oracle's algorithm in float64 (patched over `ss2d_core_ref` / `iwt_ref`): the yardstick.
* `ARCHS` names the six Stage-II archs with their shipped decomposition model and their oracle function.
"""
import torch
import torch.nn.functional as F

from oracle import bem_oracle as O

# (arch class, decomp model of its Options/*.yml, oracle function)
ARCHS = {
    "DecompDualBranchDDWavelet": ("model4", O.ddwavelet_ref),
    "DecompDualBranch2DD": ("model4", O.dualbranch2dd_ref),
    "DecompDualBranch2": ("model1", O.dualbranch2_ref),
    "DecompSingleBranch": ("model1", O.singlebranch_ref),
    "DecompSingleBranchDD": ("model1", O.singlebranchdd_ref),
    "DecompDualBranch": ("model4", O.dualbranch_ref),
}
SIBLINGS = ["DecompDualBranch2DD", "DecompDualBranch2", "DecompSingleBranch", "DecompSingleBranchDD", "DecompDualBranch"]


def build_arch(name, n_feat=40, num_blocks=(2, 2, 2), seed=100):
    import bem.archs as A
    torch.manual_seed(seed)
    return getattr(A, name)(in_channels=6, out_channels=3, n_feat=n_feat, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp",
                            use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=list(num_blocks),
                            decomp_model=ARCHS[name][0])


def oracle(name, sd, x, scan):
    """The arch's oracle forward (final_out)."""
    return ARCHS[name][1](sd, x, scan)


DS_SCALE = 0.1          # Ds ~ DS_SCALE * N(0, 1): D*u no larger than the state term C*h
DT_RANGE = (0.05, 1.0)  # dt = softplus(dt_proj + dt_projs_bias) about a uniform draw from this range
BC_GAIN = 3.0           # gain on the B and C rows of x_proj_weight: C*h grows as BC_GAIN**2


def recurrence_dominated(sd, seed):
    """Re-draw, in place and seeded, the parameters that decide how much of each scan's state term C*h reaches the output: Ds ~ 0.1 N(0,1),
    dt_projs_bias the inverse softplus of U[0.05, 1], and the B / C rows of x_proj_weight scaled by 3.  out_norm cancels a channel-uniform
    scale of the scan output, so what reaches the output is the state term against D*u: it is seen best with the two of one size.
    The frozen decomposition (decomp.*) is not touched.  Returns sd."""
    g = torch.Generator().manual_seed(seed)
    for k in sorted(sd):
        v = sd[k]
        if k.startswith("decomp."):
            continue
        if k.endswith(".Ds"):
            v.copy_(DS_SCALE * torch.randn(v.shape, generator=g))
        elif k.endswith(".dt_projs_bias"):
            dt = DT_RANGE[0] + (DT_RANGE[1] - DT_RANGE[0]) * torch.rand(v.shape, generator=g, dtype=torch.float64)
            v.copy_(torch.log(torch.expm1(dt)))
        elif k.endswith(".x_proj_weight"):
            v[:, -2:].mul_(BC_GAIN)                 # (K, R + 2, Cd): dt rows, then B, then C (d_state 1)
    return sd


def scan64(u, delta, A, Bm, Cm, D, delta_bias, blk=32):
    """The d_state-1 selective scan h_t = exp(dt_t A) h_{t-1} + dt_t B_t u_t, y_t = C_t h_t + D u_t in float64: u / delta (B, K*Cd, L),
    A (K*Cd, 1), Bm / Cm (B, K, 1, L).  Closed form inside blocks of `blk` steps, h_t = exp(cl_t) (h_in + sum_{s<=t} exp(-cl_s) b_s) with
    cl the running sum of dt*A from the block's start (every block at once), then one pass over the blocks for the carries h_in.
    Returns (C*h, D*u) separately."""
    Bt, KC, L = u.shape
    K = Bm.shape[1]
    dt = F.softplus(delta + delta_bias[None, :, None])
    la = dt * A.reshape(1, KC, 1)
    bu = dt * u * Bm[:, :, 0].repeat_interleave(KC // K, dim=1)
    nb = -(-L // blk)
    pad = lambda t: F.pad(t, (0, nb * blk - L)).view(Bt, KC, nb, blk)
    cl = torch.cumsum(pad(la), -1)
    assert float(cl.min()) > -600, "a block's decay leaves the float64 range: use a smaller blk"
    hl = torch.exp(cl) * torch.cumsum(torch.exp(-cl) * pad(bu), -1)            # block-local states (h_in = 0)
    h, hin = torch.zeros(Bt, KC, dtype=u.dtype), []
    for j in range(nb):
        hin.append(h)
        h = torch.exp(cl[:, :, j, -1]) * h + hl[:, :, j, -1]
    hs = (hl + torch.exp(cl) * torch.stack(hin, 2)[..., None]).reshape(Bt, KC, nb * blk)[:, :, :L]
    return hs * Cm[:, :, 0].repeat_interleave(KC // K, dim=1), D[None, :, None] * u


def ss2d_core64(sd, pre, x, scan=None, state_gain=1.0):
    """ss2d_core_ref with nothing cast down (the reference casts to f32); `state_gain` scales the scan's state term C*h."""
    B, Cd, H, W = x.shape
    xw, dtw = sd[pre + "x_proj_weight"], sd[pre + "dt_projs_weight"]
    K, _, R = dtw.shape
    N = sd[pre + "A_logs"].shape[1]
    assert N == 1
    xs = O.cross_scan_ref(x)
    x_dbl = torch.einsum("bkcl,kjc->bkjl", xs, xw)
    dts, Bs, Cs = torch.split(x_dbl, [R, N, N], dim=2)
    dts = torch.einsum("bkrl,kcr->bkcl", dts, dtw)
    ch, du = scan64(xs.reshape(B, K * Cd, H * W), dts.reshape(B, K * Cd, H * W), -torch.exp(sd[pre + "A_logs"]), Bs, Cs, sd[pre + "Ds"],
                    sd[pre + "dt_projs_bias"].reshape(-1))
    y = O.cross_merge_ref((state_gain * ch + du).reshape(B, K, Cd, H, W)).reshape(B, Cd, H, W)
    return O.layernorm2d_ref(y, sd[pre + "out_norm.weight"], sd[pre + "out_norm.bias"])


def iwt64(x):
    """iwt_ref without its f32 cast."""
    B, C4, H, W = x.shape
    C = C4 // 4
    ll, hl, lh, hh = (x[:, i * C:(i + 1) * C] / 2 for i in range(4))
    out = torch.zeros(B, C, 2 * H, 2 * W, dtype=x.dtype)
    out[:, :, 0::2, 0::2], out[:, :, 1::2, 0::2] = ll - hl - lh + hh, ll - hl + lh - hh
    out[:, :, 0::2, 1::2], out[:, :, 1::2, 1::2] = ll + hl - lh - hh, ll + hl + lh + hh
    return out


def float64_ref(name, sd, x, core=ss2d_core64):
    """The arch's oracle evaluated in float64: the yardstick."""
    from unittest import mock
    with mock.patch.object(O, "ss2d_core_ref", core), mock.patch.object(O, "iwt_ref", iwt64):
        r = oracle(name, {k: v.double() for k, v in sd.items()}, x.double(), None)
    assert r.dtype == torch.float64
    return r


def errors(a, ref):
    """(mean, max) of |a - ref| in float64."""
    e = (a.double() - ref).abs()
    return float(e.mean()), float(e.max())
