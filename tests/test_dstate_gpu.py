"""GPU: SS2D with d_state N > 1 -- the N-state scan kernels (bem_ss2d_scan_n_f32 / _bwd_f32) against the oracle and a float64
restatement (tests/dstate_ref.py), the VSSBlock against the reference (g14_dstate.npz), and the archs, training steps and the
Monte-Carlo pipeline built with d_state > 1 against the oracle."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dstate_ref as D
from conftest import PKG, load_golden, qd_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    from bem import native
    native.lib()
    return torch.device("cuda", 0)


def close(a, b, rtol, atol=0.0, what=""):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    bound = atol + rtol * b.abs()
    assert bool((err <= bound).all()), f"{what}: max|diff| {float(err.max()):.3e}, worst excess {float((err - bound).max()):.3e}"


def _run_kernel(x, xw, dtw, dtb, A_logs, Ds, dev):
    from bem import ops
    x0, x1, xd0, xd1 = D.x_dbl(x, xw)
    c = lambda t: t.to(dev).contiguous()
    A = (-torch.exp(A_logs)).contiguous()
    y0, y1 = ops.ss2d_scan_n(c(x0), c(x1), c(xd0), c(xd1), c(dtw), c(dtb), c(A), c(Ds))
    torch.cuda.synchronize()
    return (x0, x1, xd0, xd1), y0.cpu(), y1.cpu()


@pytest.mark.parametrize("N", [2, 4, 8, 16])
@pytest.mark.parametrize("B,C,H,W", [(2, 12, 16, 12), (2, 12, 17, 23), (1, 8, 56, 80), (1, 8, 128, 128)])
def test_scan_n_kernel_vs_oracle_and_float64(dev, N, B, C, H, W):
    """L = 192 (one 256-position tile), 391 (odd, L % 4 != 0), 4480 (18 tiles), 16384; C = 12 leaves 4 idle wavefronts in the second
    workgroup.  The HIP error to float64 must be within 2x the f32 restatement's own error (plus 1e-6 of the output scale)."""
    from oracle import bem_oracle as O
    x, xw, dtw, dtb, A_logs, Ds = D.make_operands(B, C, H, W, N, seed=1000 + N + H)
    ops_in, y0, y1 = _run_kernel(x, xw, dtw, dtb, A_logs, Ds, dev)
    r0, r1 = D.ss2d_scan_n_ref(*ops_in, dtw, dtb, A_logs, Ds)
    f0, f1 = D.ss2d_scan_n_ref(*ops_in, dtw, dtb, A_logs, Ds, dtype=torch.float32)
    scale = float(torch.cat([r0, r1]).abs().max())
    for got, f32, ref, what in ((y0, f0, r0, "y0"), (y1, f1, r1, "y1")):
        e_hip = (got.double() - ref).abs()
        e_f32 = (f32.double() - ref).abs()
        assert float(e_hip.max()) <= 2 * float(e_f32.max()) + 1e-6 * scale, (what, float(e_hip.max()), float(e_f32.max()), scale)
        assert float(e_hip.mean()) <= 2 * float(e_f32.mean()) + 1e-7 * scale, (what, float(e_hip.mean()), float(e_f32.mean()))
    # the oracle's SS2D core (cross scan, x_proj, selective scan, cross merge, out_norm) on the same operands
    sd = {"x_proj_weight": xw, "dt_projs_weight": dtw, "dt_projs_bias": dtb, "A_logs": A_logs, "Ds": Ds,
          "out_norm.weight": torch.ones(C), "out_norm.bias": torch.zeros(C)}
    ref = O.ss2d_core_ref(sd, "", x, O.selective_scan_c)
    close(O.layernorm2d_ref(D.merge(y0, y1, H, W), torch.ones(C), torch.zeros(C)), ref, 1e-4, 2e-5, "ss2d_core_ref")


@pytest.mark.parametrize("N", [4, 16])
@pytest.mark.parametrize("H,W", [(16, 12), (17, 23)])
def test_scan_n_backward_vs_autograd(dev, N, H, W):
    """bem_ss2d_scan_n_bwd_f32 against torch.autograd through the float64 restatement: dx0 / dx1, the x_dbl gradients (R + 2N rows),
    dA_logs (4C, N), dDs, ddtw, ddtb."""
    from bem import ops
    B, C = 2, 12
    x, xw, dtw, dtb, A_logs, Ds = D.make_operands(B, C, H, W, N, seed=77 + N)
    x0, x1, xd0, xd1 = D.x_dbl(x, xw)
    g = torch.Generator().manual_seed(5)
    dy0, dy1 = torch.randn(x0.shape, generator=g), torch.randn(x0.shape, generator=g)
    leaves = [t.double().requires_grad_() for t in (x0, x1, xd0, xd1, dtw, dtb, A_logs, Ds)]
    r0, r1 = D.ss2d_scan_n_ref(*leaves)
    grads = torch.autograd.grad([r0, r1], leaves, [dy0.double(), dy1.double()])
    c = lambda t: t.to(dev).contiguous()
    dAlog, dDs = torch.zeros(4 * C, N, device=dev), torch.zeros(4 * C, device=dev)
    ddtw, ddtb = torch.zeros(4, C, dtw.shape[2], device=dev), torch.zeros(4, C, device=dev)
    dx0, dx1, dxd0, dxd1 = ops.ss2d_scan_n_bwd(c(x0), c(x1), c(xd0), c(xd1), c(dy0), c(dy1), c(dtw), c(dtb), c(-torch.exp(A_logs)), c(Ds),
                                               dAlog, dDs, ddtw, ddtb)
    torch.cuda.synchronize()
    for got, ref, what in ((dx0, grads[0], "dx0"), (dx1, grads[1], "dx1"), (dxd0, grads[2], "dxd0"), (dxd1, grads[3], "dxd1"),
                           (ddtw, grads[4], "ddtw"), (ddtb, grads[5], "ddtb"), (dAlog, grads[6], "dA_logs"), (dDs, grads[7], "dDs")):
        s = float(ref.abs().max())
        close(got, ref.float(), 2e-4, 2e-5 * s + 1e-6, what)


def _vss(N):
    from bem.modules import VSSBlock
    return VSSBlock(hidden_dim=40, ssm_d_state=N, ssm_ratio=1, ssm_conv_bias=False, forward_type="v05_noz", mlp_ratio=4, mlp_type="gdmlp")


@pytest.mark.parametrize("N", [4, 16])
def test_vssblock_forward_golden(dev, N):
    g = load_golden("g14_dstate")
    blk = _vss(N)
    blk.load_state_dict(g[f"sd_n{N}"], strict=True)
    blk.to(dev).eval()
    with torch.no_grad():
        y = blk(g[f"x_n{N}"].to(dev))
    close(y, g[f"y_n{N}"], 1e-3, 3e-5, f"VSSBlock N={N}")


@pytest.mark.parametrize("N", [4, 16])
def test_vssblock_backward_golden(dev, N):
    """dx and the x_proj / A_logs (4C, N) / dt bias / Ds / in_proj gradients recorded from the reference's autograd."""
    g = load_golden("g14_dstate")
    blk = _vss(N).to(dev)
    blk.load_state_dict(g[f"sd_n{N}"], strict=True)
    blk.train()
    x = g[f"x_n{N}"].to(dev).requires_grad_()
    y = blk(x)
    close(y, g[f"y_n{N}"], 2e-5, 1e-5, "forward")
    y.backward(g[f"dout_n{N}"].to(dev))
    close(x.grad, g[f"dx_n{N}"], 1e-3, 1e-5, "dx")
    params = dict(blk.named_parameters())
    for k, ref in g[f"grads_n{N}"].items():
        close(params[k].grad, ref, 2e-3, 1e-5 * float(ref.abs().max()) + 1e-7, k)


def _kw(d_state, n_feat=16, nb=(1, 1, 1)):
    return dict(n_feat=n_feat, d_state=list(d_state), ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0,
                sam=False, stage=1, num_blocks=list(nb))


def _visible(net, seed):
    """Ds / dt biases / B-C rows away from their init, so that the scans' state terms reach the outputs (tests/stage2_yardstick.py)."""
    from bem.modules import SS2D
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, SS2D):
                m.Ds.copy_(0.1 * torch.randn(m.Ds.shape, generator=g))
                dt = 0.05 + 0.95 * torch.rand(m.dt_projs_bias.shape, generator=g)
                m.dt_projs_bias.copy_(dt + torch.log(-torch.expm1(-dt)))
                m.x_proj_weight[:, m.dt_rank:].mul_(3.0)


def test_stage2_mixed_d_state_forward_vs_oracle(dev):
    """DecompDualBranchDDWavelet with d_state = [1, 4, 2] (the N = 1 kernels at level 0, the N-state kernel elsewhere), 64x64."""
    import bem.archs as A
    from bem.pipeline import synthetic_pair
    from oracle import bem_oracle as O
    torch.manual_seed(3)
    net = A.DecompDualBranchDDWavelet(in_channels=6, out_channels=3, decomp_model="model4", **_kw([1, 4, 2], nb=(1, 1, 1)))
    _visible(net, 4)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    lq, gt = synthetic_pair((2, 3, 64, 64), seed=9)
    x = torch.cat([lq, gt], 1)
    ref = O.ddwavelet_ref(sd, x, O.selective_scan_c)
    with torch.no_grad():
        out = net.to(dev).eval()(x.to(dev))[-1]
    close(out, ref, 2e-3, 1e-4, "DDWavelet d_state [1,4,2]")


def _train_opt(d_state):
    return dict(model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, condition=dict(type="mean", scale_down=16, noise_level=0.0),
                network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, decomp_model="model4", **_kw(d_state, nb=(2, 1, 1))),
                path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None),
                train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                           scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                           optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                           pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))


def _train_inputs():
    from bem.pipeline import synthetic_pair
    lq, gt = synthetic_pair((1, 3, 32, 32), seed=21)
    g = torch.Generator().manual_seed(33)
    gt_down = F.interpolate(gt, scale_factor=1 / 16, mode="bilinear") + 0.1 * torch.randn(1, 3, 2, 2, generator=g)
    return lq, gt, gt_down


def _train_run(sd0, steps=2):
    from basicsr.models import build_model
    model = build_model(_train_opt([4, 4, 4]))
    model.net_g.load_state_dict(sd0, strict=False)
    lq, gt, gt_down = _train_inputs()
    out = []
    for it in range(steps):
        model.feed_train_data(dict(lq=lq, gt=gt, gt_down=gt_down))
        tn = model.optimize_parameters(it + 1)
        out.append((float(model.log_dict["l_pix"]), float(tn)))
    return model, out


def _train_sd():
    import bem.archs as A
    torch.manual_seed(11)
    net = A.DecompDualBranchDDWavelet(in_channels=6, out_channels=3, decomp_model="model4", **_kw([4, 4, 4], nb=(2, 1, 1)))
    _visible(net, 12)
    return {k: v.detach().clone() for k, v in net.state_dict().items() if not k.startswith("decomp.")}


def test_stage2_training_step_d_state_4_vs_oracle(dev):
    """Config-4 shape (DecompDualBranchDDWavelet + model4, L1, clip 1, AdamW) at d_state = [4, 4, 4]: two steps against
    oracle.train_step_ref, the tolerances of the existing Stage-II training tests."""
    from oracle import bem_oracle as O
    sd0 = _train_sd()
    sd = {**sd0, **qd_state_dict("model4")}
    lq, gt, gt_down = _train_inputs()
    ref = O.train_step_ref(sd, lq, gt, gt_down, steps=2, lr=2e-4, weight_decay=1e-4, max_grad_norm=1.0)
    model, got = _train_run(sd0)
    for it in range(2):
        assert abs(got[it][0] - ref["loss"][it]) < 3e-6, (it, got[it][0], ref["loss"][it])
        assert abs(got[it][1] - ref["grad_norm"][it]) < 5e-4 * ref["grad_norm"][it], (it, got[it][1], ref["grad_norm"][it])
    named = dict(model.net_g.named_parameters())
    bad = tot = 0
    for k, v in ref["params"].items():
        u_ref, u_dev = (v - sd[k]).double(), (named[k].detach().cpu() - sd[k]).double()
        assert float((u_dev - u_ref).abs().max()) <= 2 * 2 * 2e-4 * 1.05, k
        bad += int(((u_dev - u_ref).abs() > 0.05 * u_ref.abs() + 2e-6).sum())
        tot += v.numel()
    assert bad <= 0.01 * tot, f"{bad} of {tot} parameter updates differ from the oracle's"
    assert any(k.endswith("A_logs") and v.shape[1] == 4 for k, v in ref["params"].items())


def test_stage2_training_step_d_state_4_reproducible(dev):
    sd0 = _train_sd()
    ma, a = _train_run(sd0)
    mb, b = _train_run(sd0)
    for (la, na), (lb, nb) in zip(a, b):
        assert abs(la - lb) <= 1e-6 and abs(na - nb) <= 1e-5 * max(1.0, na)
    pa, pb = dict(ma.net_g.named_parameters()), dict(mb.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    assert worst <= 4e-5, worst


def test_stage1_captured_step_d_state_2(dev, tmp_path, monkeypatch):
    """Stage-I training at d_state = [2, 2, 2]: the step replayed from a HIP graph equals the launched one (the equality of
    test_train_gpu.py::test_stage1_captured_step_equals_the_launched_one)."""
    from basicsr.train import train_pipeline

    def run(root):
        argv = ["--opt", os.path.join(PKG, "Options", "CG_UNet_LOLv1.yml"), "--synthetic", "4",
                "--force_yml", "network_g:n_feat=16", "network_g:num_blocks=[1,1,1]", "network_g:d_state=[2,2,2]", "train:total_iter=6",
                "logger:save_checkpoint_freq=100", "logger:print_freq=1", "datasets:train:batch_size_per_gpu=2", "datasets:train:gt_size=64",
                "train:scheduler:periods=[4,4,4]"]
        torch.manual_seed(100)
        return train_pipeline(str(root), argv=argv)[0]
    monkeypatch.setenv("BEM_STAGE1_GRAPH", "0")
    a = run(tmp_path / "A")
    monkeypatch.setenv("BEM_STAGE1_GRAPH", "1")
    b = run(tmp_path / "B")
    assert [g for g in b._graphs.values() if isinstance(g, dict)], "no captured step"
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    assert all(v.shape[1] == 2 for k, v in pa.items() if k.endswith("A_logs"))
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    assert worst <= 4e-5, worst
    assert abs(float(a.log_dict["l_pix"]) - float(b.log_dict["l_pix"])) <= 1e-4


def test_pipeline_eval_d_state_4_vs_oracle(dev):
    """BEMPipeline, N = 2 Bayesian samples at 64x64, d_state = [4, 4, 4] in both stages, injected eps / noise, against oracle.eval_mc_ref."""
    from basicsr.bayesian import convert2bnn_selective
    import bem.archs as A
    from bem.pipeline import BEMPipeline, synthetic_pair
    from oracle import bem_oracle as O
    torch.manual_seed(100)
    kw = _kw([4, 4, 4])
    net1 = A.Network(in_channels=3, out_channels=3, **kw)
    convert2bnn_selective(net1, {"sigma_init": 0.05, "decay": 0.998, "pretrain": False})
    net2 = A.DecompDualBranchDDWavelet(in_channels=6, out_channels=3, decomp_model="model4", **kw)
    _visible(net2, 8)
    sd1 = {k: v.detach().clone() for k, v in net1.state_dict().items()}
    sd2 = {k: v.detach().clone() for k, v in net2.state_dict().items()}
    lq, gt = synthetic_pair((1, 3, 64, 64))
    N = 2
    g = torch.Generator().manual_seed(7)
    eps_cpu = [{k[:-len("mu_weight")] + "weight" if k.endswith("mu_weight") else k[:-len("mu_bias")] + "bias": torch.randn(v.shape, generator=g)
                for k, v in sd1.items() if k.endswith(("mu_weight", "mu_bias"))} for _ in range(N)]
    noise = torch.randn(N, 3, 4, 4, generator=g)
    ref = O.eval_mc_ref(sd1, sd2, lq, gt, N, eps_list=eps_cpu, noise_list=[noise[i:i + 1] for i in range(N)], scan=O.selective_scan_c)
    net1.to(dev).eval(); net2.to(dev).eval()
    eps_dev = {k: torch.stack([e[k] for e in eps_cpu]).to(dev) for k in eps_cpu[0]}
    out = BEMPipeline(net1, net2).enhance(lq.to(dev), gt.to(dev), N, gt_mean=True, eps=eps_dev, noise=noise.to(dev))
    fin = out["final"].cpu()
    err = max(float((fin[i].permute(1, 2, 0) - torch.from_numpy(np.asarray(ref["finals"][i]))).abs().max()) for i in range(N))
    assert err < 5e-4, err
    assert float(np.abs(np.array(ref["psnr"]) - out["psnr"].cpu().numpy()).max()) < 1e-3
    assert out["best"][0] == ref["best"]
