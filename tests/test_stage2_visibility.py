"""Can the Stage-II float64 parity tests see what they guard?  CPU only, oracle only.

tests/test_modules_gpu.py::test_stage2_shipped_size_vs_float64, test_stage2_config5_vs_float64 and test_config5_monte_carlo_vs_oracle
hold the HIP output to 2x the f32 oracle's distance from the float64 evaluation (mean and max), under the recurrence-dominated operating
point of tests/stage2_yardstick.py.  Here each block of the oracle is scaled by (1 + 1e-3) in turn -- the scan's state term C*h, every SS2D branch,
every gdMlp branch, and each arch-specific block -- and the output must move by at least 5x that bound.  A kernel that is off by 0.1 % in
any of them therefore fails the GPU test."""
import contextlib
import functools
from unittest import mock

import pytest
import torch

import stage2_yardstick as Y
from oracle import bem_oracle as O

EPS = 1e-3
MARGIN = 5.0


def _scaled(f):
    return lambda *a, **k: (1 + EPS) * f(*a, **k)


def _cross_fusion_scaled(sd, pre, x_src, x_tgt, _f=O.cross_fusion_ref):
    """Cross-fusion with its gated branch (not the residual it is added to) scaled."""
    return x_tgt + (1 + EPS) * (_f(sd, pre, x_src, x_tgt) - x_tgt)


def _perturbations(name):
    p = {"scan state term C*h": ({}, functools.partial(Y.ss2d_core64, state_gain=1 + EPS)),
         "SS2D branches": ({"ss2d_ref": _scaled(O.ss2d_ref)}, Y.ss2d_core64),
         "gdMlp branches": ({"gdmlp_ref": _scaled(O.gdmlp_ref)}, Y.ss2d_core64),
         "Hamilton product": ({"hamilton_ref": _scaled(O.hamilton_ref)}, Y.ss2d_core64)}
    if name == "DecompDualBranch":
        p["cross-fusion branches"] = ({"cross_fusion_ref": _cross_fusion_scaled}, Y.ss2d_core64)
        p["SE gates"] = ({"se_block_ref": _scaled(O.se_block_ref)}, Y.ss2d_core64)
        p["spatial attention"] = ({"spatial_attention_ref": _scaled(O.spatial_attention_ref)}, Y.ss2d_core64)
    return p


@pytest.mark.parametrize("name", list(Y.ARCHS))
def test_float64_bound_sees_every_block(name):
    sd = Y.recurrence_dominated({k: v.detach().clone() for k, v in Y.build_arch(name).state_dict().items()}, 7)
    g = torch.Generator().manual_seed(11)
    x = torch.cat([0.25 * torch.rand(1, 3, 64, 64, generator=g), torch.rand(1, 3, 64, 64, generator=g)], 1)
    r64 = Y.float64_ref(name, sd, x)
    em, eM = Y.errors(Y.oracle(name, sd, x, O.selective_scan_c), r64)
    bm, bM = 2 * em, 2 * eM                                          # what the GPU tests allow HIP
    print(f"\n{name} 64x64: f32 oracle vs float64 mean {em:.2e} max {eM:.2e}; GPU bound mean {bm:.2e} max {bM:.2e}")
    weak = []
    for what, (patches, core) in _perturbations(name).items():
        with mock.patch.multiple(O, **patches) if patches else contextlib.nullcontext():
            dm, dM = Y.errors(Y.float64_ref(name, sd, x, core=core), r64)
        print(f"  {what:22s} x(1+1e-3): |dout| mean {dm:.2e} ({dm / bm:6.1f}x bound)  max {dM:.2e} ({dM / bM:6.1f}x bound)")
        if dm < MARGIN * bm or dM < MARGIN * bM:
            weak.append((what, dm / bm, dM / bM))
    assert not weak, f"blocks the float64 bound cannot see at {MARGIN}x: {weak}"


def _scan_steps64(u, delta, A, Bm, Cm, D, delta_bias):
    """The selective-scan recurrence one step at a time in float64 (selective_scan_ref without its f32 casts)."""
    Bt, KC, L = u.shape
    Cd = KC // Bm.shape[1]
    dt = torch.nn.functional.softplus(delta + delta_bias[None, :, None])
    Bx, Cx = Bm.repeat_interleave(Cd, dim=1), Cm.repeat_interleave(Cd, dim=1)
    dA, dBu = torch.exp(dt.unsqueeze(2) * A[None, :, :, None]), (dt * u).unsqueeze(2) * Bx
    h, ys = torch.zeros(Bt, KC, A.shape[1], dtype=u.dtype), []
    for t in range(L):
        h = dA[..., t] * h + dBu[..., t]
        ys.append((h * Cx[..., t]).sum(-1))
    return torch.stack(ys, dim=2) + u * D[None, :, None]


@pytest.mark.parametrize("L,blk", [(1000, 32), (77, 32), (64, 16), (300, 256)])
def test_blocked_float64_scan_is_the_step_loop(L, blk):
    """The yardstick's scan (closed form per block, then the carries) against the per-step loop: ragged and whole blocks, strong decay."""
    g = torch.Generator().manual_seed(L)
    Bt, K, Cd = 2, 4, 3
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u, delta, A = r(Bt, K * Cd, L), r(Bt, K * Cd, L), -torch.exp(r(K * Cd, 1))
    Bm, Cm, D, bias = r(Bt, K, 1, L), r(Bt, K, 1, L), r(K * Cd), r(K * Cd)
    ch, du = Y.scan64(u, delta, A, Bm, Cm, D, bias, blk=blk)
    ref = _scan_steps64(u, delta, A, Bm, Cm, D, bias)
    assert float((ch + du - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert torch.equal(du, D[None, :, None] * u)
