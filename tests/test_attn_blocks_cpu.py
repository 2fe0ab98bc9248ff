"""The float64 references of tests/attn_blocks_ref.py pinned without a GPU: against the oracle's restatements of the three blocks
(oracle/bem_oracle.py, dtype-generic, run in float64), against the tensors the reference project's own modules saw and produced
(tests/golden/g12_dualbranch.npz), and -- for the backwards -- against the formulas of csrc/attn_blocks.hip's comments written out by hand,
with the max branch routed to the first maximal channel.  Also: the tie inputs the GPU tests use do carry ties on every shape of the grid,
and the float64 path of tests/stage2_yardstick.py carries autograd (the module-path GPU test differentiates through it)."""
import pytest
import torch
import torch.nn.functional as F

import attn_blocks_ref as R
from conftest import load_golden
from oracle import bem_oracle as O


def close(a, b, rtol, atol, what=""):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max())
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {err:.3e} (ref max {float(b.abs().max()):.3e})"


def _case(name, seed):
    B, C, Cr, H, W = R.SHAPES[name]
    g = R.gen(seed)
    return g, (B, C, Cr, H, W), R.randn(g, B, C, H, W).double()


SMALL = [n for n in R.SHAPES if n != "config5-eval"]


@pytest.mark.parametrize("name", SMALL)
def test_forwards_equal_the_oracle_in_float64(name):
    g, (B, C, Cr, H, W), x = _case(name, 1)
    w1, w2 = R.randn(g, Cr, C, scale=0.5).double(), R.randn(g, C, Cr, scale=0.5).double()
    sd = {"se.fc.0.weight": w1, "se.fc.2.weight": w2}
    y = R.se_gate(R.plane_mean(x)[0], w1, w2)
    close(R.chan_scale(x, y), O.se_block_ref(sd, "se.", x), 1e-13, 1e-14, "SE block")
    for k in (3, 7):
        w = R.randn(g, 1, 2, k, k, scale=0.3).double()
        close(R.spatial_attention(x, w), O.spatial_attention_ref({"sa.conv.weight": w}, "sa.", x), 1e-13, 1e-14, f"attention {k}")
        close(R.spatial_attention(x, w, y), O.spatial_attention_ref({"sa.conv.weight": w}, "sa.", O.se_block_ref(sd, "se.", x)), 1e-13, 1e-14,
              f"SE + attention {k}")
    # cross-fusion, both as the training form (gate * t + x_tgt) and as the inference form (gate folded into the rows of W and b)
    Wt, b, gate = R.randn(g, C, C, 1, 1, scale=0.2).double(), R.randn(g, C).double(), (1 + 0.3 * R.randn(g, 1, C, 1, 1)).double()
    xt = R.randn(g, B, C, H, W).double()
    sd = {"cf.transform.weight": Wt, "cf.transform.bias": b, "cf.gate": gate}
    want = O.cross_fusion_ref(sd, "cf.", x, xt)
    close(R.chan_scale(F.conv2d(x, Wt, b), gate.reshape(-1), add=xt), want, 1e-12, 1e-13, "cross-fusion, training form")
    close(F.conv2d(x, R.row_scale(Wt, gate.reshape(-1)), R.row_scale(b, gate.reshape(-1))) + xt, want, 1e-12, 1e-13, "cross-fusion, folded gate")


@pytest.mark.parametrize("name", SMALL)
def test_backwards_equal_oracle_autograd_and_the_written_out_formulas(name):
    g, (B, C, Cr, H, W), x = _case(name, 2)
    HW = H * W
    # ---- SE block: autograd through the oracle against chan_dot -> se_gate_bwd -> chan_scale(add_bc), the chain bem/autograd.py runs
    w1, w2 = R.randn(g, Cr, C, scale=0.5).double(), R.randn(g, C, Cr, scale=0.5).double()
    dout = R.randn(g, B, C, H, W).double()
    leaves = [t.clone().requires_grad_() for t in (x, w1, w2)]
    want = torch.autograd.grad(O.se_block_ref({"se.fc.0.weight": leaves[1], "se.fc.2.weight": leaves[2]}, "se.", leaves[0]), leaves, dout)
    mean = R.plane_mean(x)[0]
    dy = R.chan_dot(dout, x)[0]
    r = R.se_gate_bwd(mean, w1, w2, dy)
    close(R.chan_scale(dout, r["y"], add_bc=r["dmean"], add_bc_scale=1.0 / HW), want[0], 1e-11, 1e-13, "SE dx")
    close(r["dw1"], want[1], 1e-11, 1e-13, "SE dW1")
    close(r["dw2"], want[2], 1e-11, 1e-13, "SE dW2")
    # the same by hand (csrc/attn_blocks.hip: dz2 = dy y (1 - y); dW2 = dz2 h^T; dh = W2^T dz2; dz1 = dh [h > 0]; dW1 = dz1 m^T; dm = W1^T dz1)
    h = torch.relu(mean @ w1.t())
    dz2 = dy * r["y"] * (1 - r["y"])
    dz1 = (dz2 @ w2) * (h > 0)
    close(r["dw2"], dz2.t() @ h, 1e-11, 1e-13, "SE dW2 by hand")
    close(r["dw1"], dz1.t() @ mean, 1e-11, 1e-13, "SE dW1 by hand")
    close(r["dmean"], dz1 @ w1, 1e-11, 1e-13, "SE dmean by hand")
    assert (r["dw1_abs"] >= r["dw1"].abs() * (1 - 1e-12)).all() and (r["dw2_abs"] >= r["dw2"].abs() * (1 - 1e-12)).all()
    assert (r["dmean_abs"] >= r["dmean"].abs() * (1 - 1e-12)).all()
    # ---- spatial attention, random and tied inputs
    for k in (3, 7):
        for xin in (x, R.quantised(g, B, C, H, W).double()):
            w = R.randn(g, 1, 2, k, k, scale=0.3).double()
            leaves = [xin.clone().requires_grad_(), w.clone().requires_grad_()]
            want = torch.autograd.grad(O.spatial_attention_ref({"sa.conv.weight": leaves[1]}, "sa.", leaves[0]), leaves, dout)
            r = R.spatial_attention_bwd(xin, w, dout)
            close(r["dx"], want[0], 1e-11, 1e-13, f"attention {k} dx")
            close(r["dw"], want[1], 1e-11, 1e-13, f"attention {k} dw")
            # by hand: dpre = (sum_c dout x) a (1 - a); dmap = conv^T(dpre); dx = dout a + dmap_mean / C + [c == first argmax] dmap_max
            _, amap, pre = R.spatial_attention(xin, w, parts=True)
            a = torch.sigmoid(pre)
            dpre = (dout * xin).sum(1, keepdim=True) * a * (1 - a)
            dmap = F.conv_transpose2d(dpre, w, padding=k // 2)
            eq = xin == xin.max(1, keepdim=True)[0]
            first = eq & (eq.cumsum(1) == 1)
            close(r["dx"], dout * a + dmap[:, 0:1] / C + first * dmap[:, 1:2], 1e-11, 1e-13, f"attention {k} dx by hand, first maximum")
            assert (r["dw_abs"] >= r["dw"].abs() * (1 - 1e-12)).all()
    # ---- cross-fusion's gate gradient is chan_dot in parameter mode
    gate = (1 + 0.3 * R.randn(g, 1, C, 1, 1)).double().requires_grad_()
    t, xt = R.randn(g, B, C, H, W).double(), R.randn(g, B, C, H, W).double()
    (dg,) = torch.autograd.grad(xt + gate * t, [gate], dout)
    close(R.chan_dot(dout, t, per_image=False)[0], dg.reshape(-1), 1e-11, 1e-13, "gate gradient")


def test_references_reproduce_the_recorded_taps():
    """g12: the inputs and outputs of the reference project's own CrossFusionBlock / SEBlock / SpatialAttention modules (f32 run)."""
    g = load_golden("g12_dualbranch")
    sd = {k: torch.as_tensor(v).double() for k, v in g["sd"].items()}
    t = {k: torch.as_tensor(v).double() for k, v in g["taps"].items()}
    for s_ in ("", "2"):
        x = t[f"bottleneck_se{s_}.in0"]
        y = R.se_gate(R.plane_mean(x)[0], sd[f"bottleneck_se{s_}.fc.0.weight"], sd[f"bottleneck_se{s_}.fc.2.weight"])
        close(R.chan_scale(x, y), t[f"bottleneck_se{s_}.out"], 1e-5, 1e-6, "SE" + s_)
        w = sd[f"spatial_attention{s_}.conv.weight"]
        close(R.spatial_attention(x, w, y), t[f"spatial_attention{s_}.out"], 1e-5, 1e-6, "SE + attention" + s_)
        close(R.spatial_attention(t[f"spatial_attention{s_}.in0"], w), t[f"spatial_attention{s_}.out"], 1e-5, 1e-6, "attention" + s_)
    for name in ("cross_fusion_12", "cross_fusion_21"):
        gate = sd[name + ".gate"].reshape(-1)
        tr = F.conv2d(t[name + ".in0"], sd[name + ".transform.weight"], sd[name + ".transform.bias"])
        close(R.chan_scale(tr, gate, add=t[name + ".in1"]), t[name + ".out"], 1e-5, 2e-6, name)
        folded = F.conv2d(t[name + ".in0"], R.row_scale(sd[name + ".transform.weight"], gate), R.row_scale(sd[name + ".transform.bias"], gate))
        close(folded + t[name + ".in1"], t[name + ".out"], 1e-5, 2e-6, name + ", folded gate")


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_tie_inputs_carry_ties_on_every_shape(name):
    B, C, Cr, H, W = R.SHAPES[name]
    x = R.quantised(R.gen(5), B, C, H, W)
    assert torch.equal(x.double().float(), x) and torch.equal(x * 4, (x * 4).round())
    assert R.tie_fraction(x) >= 0.5, (name, R.tie_fraction(x))


def test_chan_scale_and_chan_dot_modes():
    g = R.gen(3)
    B, C, H, W = 2, 5, 3, 4
    x, add = R.randn(g, B, C, H, W).double(), R.randn(g, B, C, H, W).double()
    sp, sb, bc = R.randn(g, C).double(), R.randn(g, B, C).double(), R.randn(g, B, C).double()
    for b in range(B):
        for c in range(C):
            close(R.chan_scale(x, sp, add, bc, 0.25)[b, c], sp[c] * x[b, c] + add[b, c] + 0.25 * bc[b, c], 1e-14, 1e-15)
            close(R.chan_scale(x, sb)[b, c], sb[b, c] * x[b, c], 1e-14, 1e-15)
            close(R.chan_scale(x, sp.reshape(1, C, 1, 1), add_bc=bc)[b, c], sp[c] * x[b, c] + bc[b, c], 1e-14, 1e-15)
    d, dabs = R.chan_dot(x, add)
    assert d.shape == (B, C) and float((d[1, 2] - (x[1, 2] * add[1, 2]).sum()).abs()) < 1e-13
    assert torch.allclose(R.chan_dot(x, add, per_image=False)[0], d.sum(0), rtol=1e-13) and (dabs >= d.abs()).all()
    close(R.row_scale(x, R.randn(R.gen(4), B).double())[1], x[1] * R.randn(R.gen(4), B).double()[1], 1e-14, 1e-15)


def test_float64_oracle_path_carries_autograd():
    """The module-path GPU test takes float64 gradients through O.dualbranch_ref with the float64 scan of tests/stage2_yardstick.py."""
    import stage2_yardstick as Y
    net = Y.build_arch("DecompDualBranch", n_feat=8, num_blocks=(1, 1, 1))
    sd = {k: v.detach().double() for k, v in net.state_dict().items()}
    keys = [k for k in sd if k.startswith(("cross_fusion_", "bottleneck_se", "spatial_attention"))]
    assert len(keys) == 12
    for k in keys:
        sd[k].requires_grad_()
    x = torch.rand(1, 6, 16, 16, generator=R.gen(6)).double().requires_grad_()
    out = Y.float64_ref("DecompDualBranch", sd, x)
    grads = torch.autograd.grad(out, [x] + [sd[k] for k in keys], torch.ones_like(out))
    assert all(v.dtype == torch.float64 and torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in grads)
