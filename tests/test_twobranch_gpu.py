"""GPU: the Stage-II archs without a decomposition.  The fused output head (bem_fusion_head_f32 / _bwd_f32) against a float64 torch head and
torch autograd, the four archs against the reference's recorded outputs (g15) and, at shipped width, against their float64 restatement;
two ImageEnhancer training steps of TunedModel / FusedTunedModel against oracle.train_step_ref; the Monte-Carlo pipeline with a
FusedTunedModel Stage II against oracle.eval_mc_ref; Enhancement/eval.py and basicsr/train.py with the new option files."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import twobranch_ref as T
from conftest import PKG, load_golden
from oracle import bem_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def G(seed):
    return torch.Generator().manual_seed(seed)


def _weights(seed, w1_scale=0.3, b1=(-2.0, 2.0, 0.1)):
    g = G(seed)
    w1 = w1_scale * torch.randn(3, 6, 3, 3, generator=g)
    w2 = 0.3 * torch.randn(3, 3, 3, 3, generator=g)
    return w1, torch.tensor(b1), w2, 0.1 * torch.randn(3, generator=g)


def _head64(x6, w1, b1, w2, b2):
    h = torch.relu(F.conv2d(x6.double(), w1.double(), b1.double(), padding=1))
    return F.conv2d(h, w2.double(), b2.double(), padding=1)


def _inputs(B, H, W, seed, dev, wide=6):
    """Two (B,3,H,W) branch outputs as channel slices of one (B,wide,H,W) tensor (batch stride wide*H*W); a spatial ramp makes the
    pre-activation change sign inside the image."""
    g = G(seed)
    big = torch.randn(B, wide, H, W, generator=g)
    ramp = torch.linspace(-3, 3, W)[None, None, None, :] + torch.linspace(-1, 1, H)[None, None, :, None]
    big[:, :6] += ramp
    big = big.to(dev)
    return big, big[:, 0:3], big[:, wide - 3:wide]


SHAPES = [(1, 1, 1), (5, 1, 1), (64, 1, 1), (1, 5, 7), (5, 5, 7), (64, 5, 7), (1, 33, 70), (5, 33, 70), (64, 33, 70), (1, 256, 256),
          (5, 256, 256), (64, 256, 256), (1, 448, 640), (5, 448, 640)]


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_head_forward_vs_float64(dev, B, H, W):
    big, o1, o2 = _inputs(B, H, W, B * 1000 + H + W, dev, wide=9)
    assert o1.stride(0) == o2.stride(0) == 9 * H * W
    w1, b1, w2, b2 = _weights(H * W)
    from bem import ops
    out = ops.fusion_head(o1, o2, *(t.to(dev) for t in (w1, b1, w2, b2)))
    ref = _head64(torch.cat([o1, o2], 1), *(t.to(dev) for t in (w1, b1, w2, b2)))
    err = float((out.double() - ref).abs().max())
    assert err <= 2e-5 * max(1.0, float(ref.abs().max())), err
    # the border matters: the head with relu(conv1) evaluated in the halo instead of zero padding differs (b1[1] = +2)
    if H * W > 1:
        h = torch.relu(F.conv2d(F.pad(torch.cat([o1, o2], 1).double(), (2, 2, 2, 2)), w1.double().to(dev), b1.double().to(dev)))
        wrong = F.conv2d(h, w2.double().to(dev), b2.double().to(dev))
        assert float((wrong - ref).abs().max()) > 1e-2


def test_head_forward_contiguous_and_mean(dev):
    from bem import ops
    g = G(3)
    o1, o2 = torch.randn(4, 3, 37, 91, generator=g).to(dev), torch.randn(4, 3, 37, 91, generator=g).to(dev)
    w = [t.to(dev) for t in _weights(5)]
    out = ops.fusion_head(o1, o2, *w)
    ref = _head64(torch.cat([o1, o2], 1), *w)
    assert float((out.double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    assert torch.equal(ops.fusion_head(o1, o2, mean=True), (o1 + o2) / 2.0)
    dout = torch.randn(4, 3, 37, 91, generator=g).to(dev)
    d1, d2 = ops.fusion_head_bwd_(None, None, dout, mean=True)
    assert torch.equal(d1, dout / 2) and torch.equal(d2, dout / 2)


def _bwd_case(dev, B, H, W, seed, zero_first=False):
    from bem import ops
    big, o1, o2 = _inputs(B, H, W, seed, dev)
    w1, b1, w2, b2 = (t.to(dev) for t in _weights(seed + 1))
    if zero_first:
        w1, b1 = torch.zeros_like(w1), torch.zeros_like(b1)
    dout = torch.randn(B, 3, H, W, generator=G(seed + 2)).to(dev)
    g = G(seed + 3)
    acc0 = [torch.randn(t.shape, generator=g).to(dev) for t in (w1, b1, w2, b2)]
    acc = [a.clone() for a in acc0]
    do1, do2 = ops.fusion_head_bwd_(o1, o2, dout, w1, b1, w2, *acc)
    leaves = [t.double().requires_grad_() for t in (o1, o2, w1, b1, w2, b2)]
    ref = _head64(torch.cat(leaves[:2], 1), *leaves[2:])
    grads = torch.autograd.grad(ref, leaves, dout.double())
    return (o1, o2, dout, w1, b1, w2, acc0), (do1, do2, acc), grads


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 5, 7), (3, 33, 70), (2, 256, 256), (16, 128, 128), (1, 448, 640)])
def test_head_backward_vs_autograd(dev, B, H, W):
    (_, _, _, _, _, _, acc0), (do1, do2, acc), grads = _bwd_case(dev, B, H, W, 17 + H)
    for name, got, want in (("do1", do1, grads[0]), ("do2", do2, grads[1])):
        err = float((got.double() - want).abs().max())
        assert err <= 2e-5 * max(1.0, float(want.abs().max())), (name, err)
    for name, a0, got, want in zip(("dw1", "db1", "dw2", "db2"), acc0, acc, grads[2:]):
        d = got.double() - a0.double()                     # accumulated onto the existing values
        err = float((d - want).abs().max())
        assert err <= 1e-5 * max(1.0, float(want.abs().max())), (name, err, float(want.abs().max()))


def test_head_backward_zero_preactivation(dev):
    """w1 = 0, b1 = 0: pre is exactly 0 everywhere; threshold_backward passes no gradient there, so do1 / do2 / dw1 / db1 are 0 and h = 0
    makes dw2 0 too; db2 is the sum of dout."""
    (_, _, dout, _, _, _, acc0), (do1, do2, acc), grads = _bwd_case(dev, 2, 33, 70, 5, zero_first=True)
    assert float(do1.abs().max()) == 0 and float(do2.abs().max()) == 0
    for a0, got in zip(acc0[:3], acc[:3]):
        assert torch.equal(got, a0)
    want = dout.double().sum((0, 2, 3))
    assert float((acc[3].double() - acc0[3].double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert float(grads[0].abs().max()) == 0 and float(grads[2].abs().max()) == 0


def test_head_backward_bitwise_reproducible(dev):
    from bem import ops
    (o1, o2, dout, w1, b1, w2, acc0), first, _ = _bwd_case(dev, 8, 128, 128, 77)
    acc = [a.clone() for a in acc0]
    second = ops.fusion_head_bwd_(o1, o2, dout, w1, b1, w2, *acc)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert all(torch.equal(a, b) for a, b in zip(first[2], acc))


# ------------------------------------------------------------------------------------------------------------------
# the archs
# ------------------------------------------------------------------------------------------------------------------
def _g15(tag):
    g = load_golden(f"g15_twobranch_{tag}")
    return {k: v.float() for k, v in g["sd"].items()}, g


@pytest.mark.parametrize("name,tag,d_state", [(n, T.TAGS[n], (1, 1, 1)) for n in T.REFS] + [("TunedModel", "tuned_n1_4_16", (1, 4, 16))])
def test_arch_vs_reference_golden(dev, name, tag, d_state):
    sd, g = _g15(tag)
    net = T.build(name, n_feat=16, num_blocks=(1, 1, 1), d_state=d_state)
    net.load_state_dict(sd, strict=True)
    net.to(dev).eval()
    x = g["x"].to(dev)
    outs = net(x)
    assert outs[0].data_ptr() == x.data_ptr()
    y = outs[-1].cpu()
    err = (y.double() - g["y"].double()).abs()
    assert float(err.max()) <= 2e-4 and float(err.mean()) <= 2e-5, (float(err.max()), float(err.mean()))
    if "fusion_out" in g:   # the head alone on the reference's operands
        from bem import ops
        fin = g["fusion_in"].to(dev)
        f = net.fusion
        h = ops.fusion_head(fin[:, :3], fin[:, 3:], f[0].weight.detach(), f[0].bias.detach(), f[2].weight.detach(), f[2].bias.detach())
        assert float((h.cpu() - g["fusion_out"]).abs().max()) <= 2e-6


@pytest.mark.parametrize("name", list(T.REFS))
def test_arch_shipped_size_vs_float64(dev, name):
    """n_feat 40, [2,2,2], 256x256, at the recurrence-dominated operating point of tests/stage2_yardstick.py: the HIP output within 2x the f32
    restatement's distance from the float64 evaluation (mean and max), the bound of the existing Stage-II parity tests."""
    import stage2_yardstick as Y
    net = T.build(name)
    sd = Y.recurrence_dominated({k: v.detach().clone() for k, v in net.state_dict().items()}, 7)
    net.load_state_dict(sd)
    g = G(11)
    x = torch.cat([0.25 * torch.rand(1, 3, 256, 256, generator=g), torch.rand(1, 3, 256, 256, generator=g)], 1)
    r64 = T.float64_ref(name, sd, x)
    em, eM = Y.errors(T.REFS[name](sd, x, O.selective_scan_c), r64)
    out = net.to(dev).eval()(x.to(dev))[-1].cpu()
    hm, hM = Y.errors(out, r64)
    assert hm <= 2 * em and hM <= 2 * eM, (hm, em, hM, eM)


def _enhancer(arch):
    from basicsr.models import build_model
    opt = dict(model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, condition=dict(type="mean", scale_down=16, noise_level=0.0),
               network_g=dict(type=arch, in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                              mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1]),
               path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None),
               train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                          scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                          optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                          pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))
    return build_model(opt)


@pytest.mark.parametrize("name", ["TunedModel", "FusedTunedModel"])
def test_train_step_matches_oracle(dev, name):
    """Two ImageEnhancer.optimize_parameters steps on the g15 weights against oracle.train_step_ref around the restatement: losses, gradient
    norms, every first-step gradient and the parameters after the second step."""
    sd, g = _g15(T.TAGS[name])
    x = g["x"][:1]
    lq = x[:, :3].contiguous()
    gen = G(34)
    gt = (2.5 * lq + 0.05 * torch.randn(lq.shape, generator=gen)).clamp(0, 1)
    gt_down = F.interpolate(gt, scale_factor=1 / 16, mode="bilinear") + 0.1 * torch.randn(1, 3, 2, 2, generator=gen)
    ref = O.train_step_ref(sd, lq, gt, gt_down, steps=2, lr=2e-4, weight_decay=1e-4, max_grad_norm=1.0, stage2=T.REFS[name])
    model = _enhancer(name)
    model.net_g.load_state_dict(sd, strict=True)
    named = dict(model.net_g.named_parameters())
    assert set(ref["params"]) == set(named)
    for it in range(2):
        model.feed_train_data(dict(lq=lq, gt=gt, gt_down=gt_down))
        tn = model.optimize_parameters(it + 1)
        assert abs(float(model.log_dict["l_pix"]) - ref["loss"][it]) < 3e-6, (it, float(model.log_dict["l_pix"]), ref["loss"][it])
        assert abs(float(tn) - ref["grad_norm"][it]) < 5e-4 * ref["grad_norm"][it], (it, float(tn), ref["grad_norm"][it])
    bad = tot = 0
    for k, v in ref["params"].items():
        u_ref, u_dev = (v - sd[k]).double(), (named[k].detach().cpu() - sd[k]).double()
        assert float((u_dev - u_ref).abs().max()) <= 2 * 2 * 2e-4 * 1.05, k
        bad += int(((u_dev - u_ref).abs() > 0.05 * u_ref.abs() + 2e-6).sum())
        tot += v.numel()
    assert bad <= 0.01 * tot, f"{bad} of {tot} parameter updates differ from the oracle's"
    for k in ("fusion.0.weight", "fusion.0.bias", "fusion.2.weight", "fusion.2.bias"):
        assert float((named[k].detach().cpu() - sd[k]).abs().max()) > 0, k


@pytest.mark.parametrize("name", ["TunedModel", "FusedTunedModel", "NaiveVMUNetTwoBranch", "VMUNet"])
def test_gradients_vs_oracle(dev, name):
    """Every parameter gradient of one training forward / backward (L1 loss) against torch autograd through the restatement."""
    from bem import autograd as ag
    sd, g = _g15(T.TAGS[name])
    net = T.build(name, n_feat=16, num_blocks=(1, 1, 1))
    net.load_state_dict(sd, strict=True)
    net.to(dev).train()
    x = g["x"]
    gt = torch.rand(2, 3, 32, 32, generator=G(9))
    loss = ag.l1_loss(net(x.to(dev))[-1], gt.to(dev))
    loss.backward()
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    rl = (T.REFS[name](leaves, x, O.selective_scan_ref) - gt).abs().mean()
    rl.backward()
    assert abs(float(loss.detach()) - float(rl.detach())) < 3e-6
    for k, p in net.named_parameters():
        want = leaves[k].grad
        got = p.grad.cpu()
        scale = max(float(want.abs().max()), 1e-6)
        assert float((got - want).abs().max()) <= 2e-3 * scale + 1e-7, (k, float((got - want).abs().max()), scale)


def test_pipeline_candidates_fused_tuned_vs_oracle(dev):
    """BEMPipeline with a FusedTunedModel Stage II (seeded initialisation, the pipeline sends it cat(img, cond) on the B*N rows), N = 3
    samples, injected eps / noise, against oracle.eval_mc_ref with the restatement: candidates, PSNR within 1e-3 dB, the same selection."""
    from basicsr.bayesian import convert2bnn_selective
    import bem.archs as A
    from bem.pipeline import BEMPipeline, synthetic_pair
    torch.manual_seed(100)
    kw = dict(n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1,
              num_blocks=[1, 1, 1])
    net1 = A.Network(in_channels=3, out_channels=3, **kw)
    convert2bnn_selective(net1, {"sigma_init": 0.05, "decay": 0.998, "pretrain": False})
    net2 = A.FusedTunedModel(in_channels=6, out_channels=3, **kw)
    sd2, _ = _g15("fused")                 # the g15 weights: at initialisation the head's output clamps to 0
    net2.load_state_dict(sd2, strict=True)
    sd1 = {k: v.detach().clone() for k, v in net1.state_dict().items()}
    lq, gt = synthetic_pair((1, 3, 60, 52))
    N = 3
    g = G(7)
    eps_cpu = [{k[:-len("mu_weight")] + "weight" if k.endswith("mu_weight") else k[:-len("mu_bias")] + "bias": torch.randn(v.shape, generator=g)
                for k, v in sd1.items() if k.endswith(("mu_weight", "mu_bias"))} for _ in range(N)]
    noise = torch.randn(N, 3, 4, 4, generator=g)
    ref = O.eval_mc_ref(sd1, sd2, lq, gt, N, eps_list=eps_cpu, noise_list=[noise[i:i + 1] for i in range(N)], scan=O.selective_scan_c,
                        stage2=T.fusedtunedmodel_ref)
    net1.to(dev).eval(); net2.to(dev).eval()
    eps_dev = {k: torch.stack([e[k] for e in eps_cpu]).to(dev) for k in eps_cpu[0]}
    out = BEMPipeline(net1, net2).enhance(lq.to(dev), gt.to(dev), N, gt_mean=True, eps=eps_dev, noise=noise.to(dev))
    fin = out["final"].cpu()
    # GT-mean scales each candidate by mean(target) / mean(candidate) per channel: the bound of the other pipeline tests, 5e-4, grows by it
    gain = max(1.0, max(float((gt[0].mean((1, 2)) / p[0].mean((1, 2))).max()) for p in ref["preds"]))
    err = max(float((fin[i].permute(1, 2, 0) - torch.from_numpy(np.asarray(ref["finals"][i]))).abs().max()) for i in range(N))
    assert err < 5e-4 * gain, (err, gain)
    assert float(np.abs(np.array(ref["psnr"]) - out["psnr"].cpu().numpy()).max()) < 1e-3
    assert out["best"][0] == ref["best"]


def test_eval_driver_with_tunedmodel(dev, tmp_path):
    """Enhancement/eval.py --cond_opt Options/TwoBranch_1.yml on two synthetic PNG pairs with seeded random checkpoints."""
    import importlib.util
    from PIL import Image
    from bem.pipeline import build_nets, synthetic_pair
    spec = importlib.util.spec_from_file_location("bem_eval_driver_tb", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    net1, net2 = build_nets(device="cpu", stage2="TunedModel")
    torch.save({"params": net1.state_dict()}, tmp_path / "cg.pth")
    torch.save({"params": net2.state_dict()}, tmp_path / "s2.pth")
    (tmp_path / "in").mkdir(); (tmp_path / "gt").mkdir()
    lq, gt = synthetic_pair((2, 3, 64, 64))
    for i in range(2):
        for d, t in (("in", lq), ("gt", gt)):
            Image.fromarray(np.rint(t[i].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(tmp_path / d / f"{i}.png")
    out = drv.main(["--opt", os.path.join(PKG, "Options", "CG_UNet_LOLv1.yml"), "--cond_opt", os.path.join(PKG, "Options", "TwoBranch_1.yml"),
                    "--weights", str(tmp_path / "cg.pth"), "--cond_weights", str(tmp_path / "s2.pth"), "--input_dir", str(tmp_path / "in"),
                    "--target_dir", str(tmp_path / "gt"), "--result_dir", str(tmp_path / "res"), "--dataset", "synthetic", "--GT_mean",
                    "--num_samples", "3", "--Monte_Carlo", "--seed", "11"])
    assert sorted(os.listdir(out["result_dir"])) == ["0.png", "1.png", "result.txt"]
    assert len(out["psnr"]) == 2 and all(5 < p < 100 for p in out["psnr"])


def test_training_driver_fused_tuned_resume(dev, tmp_path):
    """basicsr/train.py --opt Options/TwoBranch_3.yml --synthetic: a run broken after 3 iterations and resumed with --auto_resume ends where
    the uninterrupted run ends."""
    from basicsr.train import train_pipeline

    def run(root, total, resume=False):
        argv = ["--opt", os.path.join(PKG, "Options", "TwoBranch_3.yml"), "--synthetic", "4",
                "--force_yml", "network_g:n_feat=16", "network_g:num_blocks=[1,1,1]", f"train:total_iter={total}", "logger:save_checkpoint_freq=3",
                "logger:print_freq=1", "datasets:train:batch_size_per_gpu=2", "datasets:train:gt_size=64", "train:scheduler:periods=[4,4,4]"]
        if resume:
            argv.append("--auto_resume")
        torch.manual_seed(100)
        return train_pipeline(str(root), argv=argv)
    a, ia = run(tmp_path / "A", 6)
    run(tmp_path / "B", 3)
    assert (tmp_path / "B" / "experiments" / "FusedTwoBranch_3" / "training_states" / "3.state").is_file()
    b, ib = run(tmp_path / "B", 6, resume=True)
    assert ia["iter"] == ib["iter"] == 6
    assert type(a.net_g).__name__ == "FusedTunedModel"
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    assert worst <= 4e-5, worst
