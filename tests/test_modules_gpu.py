"""GPU parity of the module mirrors (VSSBlock, Decomp, Stage-I / Stage-II nets) against golden vectors
produced by the reference itself, and against the CPU oracle at the BASELINE sizes."""
import numpy as np
import pytest
import torch

import os

import stage2_yardstick as Y
from conftest import PKG, load_golden, qd_state_dict
from oracle import bem_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def close(a, b, rtol, atol, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite"
    err = (a - b).abs().max().item()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})"


def psnr(a, b):
    return 10 * np.log10(1.0 / float(((a.double() - b.double()) ** 2).mean()))


def test_vssblock_golden():
    from bem.modules import VSSBlock
    g = load_golden("g4_vssblock")
    blk = VSSBlock(hidden_dim=40, ssm_d_state=1, ssm_ratio=1, ssm_conv_bias=False, forward_type="v05_noz", mlp_ratio=4, mlp_type="gdmlp")
    blk.load_state_dict(g["sd"], strict=True)
    blk.cuda().eval()
    x = g["x"].cuda()
    y1 = blk.op.forward_fused(x, blk.norm)
    close(y1 - x, g["y_ss2d"], 1e-3, 2e-5, "SS2D branch")
    close(blk(x), g["y"], 1e-3, 3e-5, "VSSBlock")


def test_decomp_golden():
    from bem.archs import Decomp
    g = load_golden("g5_decomp")
    img = g["img"].cuda()
    x6 = torch.cat([torch.zeros_like(img), img], 1).contiguous()          # decompose the slice at c0 = 3
    d = Decomp.from_shipped("model4", True).cuda()
    out = d(x6, 3)
    close(out[:, :16], g["q1w_model4"], 1e-3, 2e-5, "Q1_w")
    close(out[:, 16:], g["q2w_model4"], 1e-3, 2e-5, "Q2_w")
    for m in ("model1", "model4"):
        q = Decomp.from_shipped(m, False).cuda()(img.contiguous(), 0)
        close(q[:, :4], g[f"q1_{m}"], 1e-3, 2e-5, f"Q1 {m}")
        close(q[:, 4:], g[f"q2_{m}"], 1e-3, 2e-5, f"Q2 {m}")


@pytest.mark.parametrize("tag,cls,dm", [("ddw", "DecompDualBranchDDWavelet", "model4"), ("single", "DecompSingleBranch", "model1")])
def test_stage2_golden(tag, cls, dm):
    import bem.archs as A
    g = load_golden(f"g6_{tag}")
    net = getattr(A, cls)(in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp",
                          use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[2, 1, 1], decomp_model=dm)
    assert list(net.state_dict().keys()) and set(net.state_dict().keys()) == set(g["keys"].tolist())
    sd = dict(g["sd"]); sd.update({k: v for k, v in qd_state_dict(dm).items() if k in net.state_dict()})
    net.load_state_dict(sd, strict=True)
    net.cuda().eval()
    out = net(g["x"].cuda())[-1]
    close(out, g["out"], 2e-3, 1e-4, cls)
    assert abs(psnr(out.cpu(), g["gt"]) - psnr(g["out"], g["gt"])) < 1e-3          # north-star parity bar (dB)


def _stage1(n_feat, blocks):
    from basicsr.archs import build_network
    from basicsr.bayesian import convert2bnn_selective
    net = build_network(dict(type="Network", in_channels=3, out_channels=3, n_feat=n_feat, stage=1, num_blocks=blocks, d_state=[1, 1, 1],
                             ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=True))
    convert2bnn_selective(net, {"sigma_init": 0.05, "decay": 0.998, "pretrain": False})
    return net


def test_stage1_golden_det_and_injected_eps():
    from basicsr.bayesian import set_prediction_type
    from bem.modules import SampleCtx, sampling
    g = load_golden("g7_network")
    net = _stage1(16, [2, 1, 1])
    assert set(net.state_dict().keys()) == set(g["keys"].tolist())
    net.load_state_dict(g["sd"], strict=True)
    net.cuda().eval()
    x = g["x"].cuda()
    set_prediction_type(net, True)
    close(net(x)[-1], g["y_det"], 2e-3, 5e-5, "Stage-I deterministic")
    set_prediction_type(net, False)
    # the reference shares ONE weight sample across the batch: nsets = 1 with the recorded epsilons
    eps = {k: v[None].cuda() for k, v in g["eps"].items()}
    with sampling(SampleCtx(1, eps)):
        close(net(x)[-1], g["y_sto"], 2e-3, 5e-5, "Stage-I sampled (injected eps)")
    # per-batch-element samples: row i with eps set i must equal a B=1 run with that set
    B = x.shape[0]
    gen = torch.Generator().manual_seed(3)
    eps2 = {k: torch.randn((B,) + tuple(v.shape), generator=gen).cuda() for k, v in g["eps"].items()}
    with sampling(SampleCtx(B, eps2)):
        yb = net(x)[-1]
    for i in range(B):
        with sampling(SampleCtx(1, {k: v[i:i + 1].contiguous() for k, v in eps2.items()})):
            close(net(x[i:i + 1].contiguous())[-1], yb[i:i + 1], 1e-4, 1e-5, f"per-sample weights row {i}")
    # Philox path runs and differs between calls / rows
    y1, y2 = net(x)[-1], net(x)[-1]
    assert torch.isfinite(y1).all() and not torch.equal(y1, y2)


def test_stage2_full_width_vs_oracle_256():
    """BASELINE config-2 geometry (n_feat 40, [2,2,2], 256x256), batch 2, seeded random weights:
    HIP vs the CPU oracle (C scan).  PSNR(candidate, gt) must agree within 1e-3 dB."""
    import bem.archs as A
    torch.manual_seed(100)
    net = A.DecompDualBranchDDWavelet(in_channels=6, out_channels=3, n_feat=40, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                                      mlp_type="gdmlp", use_pixelshuffle=True, num_blocks=[2, 2, 2], decomp_model="model4")
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(287128)
    lq = 0.25 * torch.rand(2, 3, 256, 256, generator=g)
    gt = (3.5 * lq + 0.05 * torch.randn(2, 3, 256, 256, generator=g)).clamp(0, 1)
    cond = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(gt, 16) + 0.1 * torch.randn(2, 3, 16, 16, generator=g),
                                           scale_factor=16, mode="bilinear", align_corners=False)
    x = torch.cat([lq, cond], 1)
    ref = O.ddwavelet_ref(sd, x, O.selective_scan_c)
    out = net.cuda().eval()(x.cuda())[-1].cpu()
    close(out, ref, 5e-3, 2e-4, "Stage-II 256x256")
    for i in range(2):
        assert abs(psnr(out[i].clamp(0, 1), gt[i]) - psnr(ref[i].clamp(0, 1), gt[i])) < 1e-3


def test_operator_seam_modules():
    """basicsr.vmamba.models.{csms6s,csm_triton} drop-ins, called like forward_corev2 calls them."""
    from basicsr.vmamba.models.csm_triton import cross_merge_fn, cross_scan_fn
    from basicsr.vmamba.models.csms6s import selective_scan_fn
    g = load_golden("g1_scan_a")
    y = selective_scan_fn(g["u"].cuda(), g["delta"].cuda(), g["A"].cuda(), g["B"].cuda(), g["C"].cuda(), g["D"].cuda(), g["delta_bias"].cuda(), True, True)
    close(y, g["y"], 1e-4, 1e-4, "selective_scan_fn")
    c = load_golden("g2_cross")
    assert torch.equal(cross_scan_fn(c["x"].cuda()).cpu(), c["xs"])
    close(cross_merge_fn(c["ys"].cuda()), c["y"], 0, 1e-6, "cross_merge_fn")
    with pytest.raises(NotImplementedError):
        cross_scan_fn(c["x"].cuda(), scans=1)


def test_eval_loop_golden_g8():
    """The whole MC loop (Stage-I samples with the recorded eps/noise -> upsample -> Stage-II -> GT-mean ->
    PSNR -> selection) against the run of the reference nets recorded in g8_eval.npz."""
    from basicsr.bayesian import convert2bnn_selective
    import bem.archs as A
    from bem.pipeline import BEMPipeline
    g = load_golden("g8_eval")
    kw = dict(n_feat=8, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=True, num_blocks=[1, 1, 1])
    net1 = A.Network(in_channels=3, out_channels=3, stage=1, **kw)
    convert2bnn_selective(net1, {"sigma_init": 0.05, "decay": 0.998, "pretrain": False})
    net1.load_state_dict(g["sd1"], strict=True)
    net2 = A.DecompDualBranchDDWavelet(in_channels=6, out_channels=3, decomp_model="model4", **kw)
    sd2 = dict(g["sd2"]); sd2.update({k: v for k, v in qd_state_dict("model4").items() if k in net2.state_dict()})
    net2.load_state_dict(sd2, strict=True)
    net1.cuda().eval(); net2.cuda().eval()
    n = g["conds"].shape[0]
    eps = {k: torch.stack([g[f"eps{i}"][k] for i in range(n)]).cuda() for k in g["eps0"]}
    pipe = BEMPipeline(net1, net2, 16, 0.1)
    r = pipe.enhance(g["lq"].cuda(), g["gt"].cuda(), n, gt_mean=True, eps=eps, noise=g["noises"].cuda(), img_down=g["img_down"].cuda())
    close(r["conds"], g["conds"], 2e-3, 1e-4, "conditions")
    close(r["raw"][:, :, :60, :52].clamp(0, 1), g["preds"], 2e-3, 2e-4, "candidates")
    close(r["final"].permute(0, 2, 3, 1), g["finals"], 2e-3, 2e-4, "GT-mean candidates")
    assert np.abs(r["psnr"].cpu().numpy() - np.asarray(g["psnr"])).max() < 1e-3        # dB
    assert r["best"][0] == int(g["best"])


def test_smoke_entry():
    import __graft_entry__ as ge
    ge.smoke()


def test_stage2_config5_geometry_400x600():
    """BASELINE config-5 geometry: a 400x600 image is reflect-padded to 448x640 (L = 71680 at level 0: multi-chunk scan
    with the global read-modify-write path, non-square maps, 28x40 condition).  One (image, sample) pair, seeded weights,
    deterministic Stage-I: HIP pipeline vs the CPU oracle; PSNR of the candidate must agree within 1e-3 dB, the final image within
    1.5e-2 max / 5e-6 mean (measured on the MI355X: max 4.2e-3, mean 1.2e-6)."""
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, net2 = build_nets(device="cuda")
    sd1 = {k: v.detach().cpu() for k, v in net1.state_dict().items()}
    sd2 = {k: v.detach().cpu() for k, v in net2.state_dict().items()}
    lq, gt = synthetic_pair((1, 3, 400, 600), seed=5)
    noise = torch.randn(1, 3, 28, 40, generator=torch.Generator().manual_seed(9))
    ref = O.eval_mc_ref(sd1, sd2, lq, gt, 1, deterministic=True, gt_mean=True, noise_list=[noise], scan=O.selective_scan_c)
    out = BEMPipeline(net1, net2).enhance(lq.cuda(), gt.cuda(), 1, gt_mean=True, deterministic=True, noise=noise.cuda())
    assert out["raw"].shape == (1, 3, 448, 640) and out["final"].shape == (1, 3, 400, 600)
    # Stage I: the condition carries the GT-mean rescale (x ~20 on these random-init nets) of the Stage-I rounding error
    close(out["conds"], ref["conds"][0], 0, 1e-4, "config-5 geometry condition")
    # Stage II at this geometry in isolation: the oracle evaluated on the condition the HIP Stage I produced (fed with the
    # oracle's own condition instead, Stage II's sensitivity to its input -- ~200x here -- would be measuring Stage I again)
    pad = torch.from_numpy(np.ascontiguousarray(O.pad_reflect_ref(lq[0].permute(1, 2, 0).numpy(), 64))).permute(2, 0, 1)[None]
    up = torch.nn.functional.interpolate(out["conds"].cpu(), scale_factor=16, mode="bilinear", align_corners=False)
    ref2 = O.ddwavelet_ref(sd2, torch.cat([pad, up], 1), O.selective_scan_c)
    close(out["raw"], ref2, 1e-4, 5e-6, "config-5 geometry Stage II")
    # end to end: the north-star criterion (PSNR of the selected candidate within 1e-3 dB) and a sanity bound on the image
    d = (out["final"][0].permute(1, 2, 0).cpu() - torch.from_numpy(ref["finals"][0])).abs()
    print(f"final image: mean|d| {d.mean():.2e} max|d| {d.max():.2e}")
    assert d.max() < 1.5e-2 and d.mean() < 5e-6, (d.max(), d.mean())
    assert abs(float(out["psnr"][0]) - ref["psnr"][0]) < 1e-3


@pytest.mark.parametrize("tag,cls,dm", [("dualdd", "DecompDualBranch2DD", "model4"), ("dual2", "DecompDualBranch2", "model1"),
                                        ("singledd", "DecompSingleBranchDD", "model1")])
def test_sibling_archs_golden(tag, cls, dm):
    """The three sibling Stage-II archs against the reference's own outputs (g9 fixtures); same kernels, other wiring."""
    import bem.archs as A
    g = load_golden(f"g9_{tag}")
    net = getattr(A, cls)(in_channels=6, out_channels=3, n_feat=8, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp",
                          use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model=dm)
    assert set(net.state_dict().keys()) == set(g["keys"].tolist())
    sd = dict(g["sd"]); sd.update({k: v for k, v in qd_state_dict(dm).items() if k in net.state_dict()})
    net.load_state_dict(sd, strict=True)
    net.cuda().eval()
    res = net(g["x"].cuda())
    close(res[-1], g["out"], 2e-3, 1e-4, cls)
    close(res[0], g["first"], 0, 0, cls + " passthrough")


def test_dualbranch_se_attention_golden():
    """DecompDualBranch (DecompModel_arch.py:101-366) against the reference's own run (g12): the three blocks it adds on the tensors the
    reference's modules saw (forward hooks: cross-fusion as a gated GEMM with residual, SE gate + 7x7 spatial attention in one pass),
    then the whole net (the backward side: tests/test_train_gpu.py::test_dualbranch_*)."""
    import bem.archs as A
    from bem import ops
    g = load_golden("g12_dualbranch")
    net = A.DecompDualBranch(in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp",
                             use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model="model4")
    assert set(net.state_dict().keys()) == set(g["keys"].tolist())
    sd = dict(g["sd"]); sd.update({k: v for k, v in qd_state_dict("model4").items() if k in net.state_dict()})
    net.load_state_dict(sd, strict=True)
    net.cuda().eval()
    t = {k: torch.as_tensor(v).cuda() for k, v in g["taps"].items()}
    for s_ in ("", "2"):
        se, sa = getattr(net, "bottleneck_se" + s_), getattr(net, "spatial_attention" + s_)
        x = t[f"bottleneck_se{s_}.in0"]
        y = se.gate(x)
        close(x * y[:, :, None, None], t[f"bottleneck_se{s_}.out"], 1e-5, 1e-6, "SE" + s_)
        close(sa(x, chan_scale=y), t[f"spatial_attention{s_}.out"], 1e-5, 1e-6, "SE + attention" + s_)
        close(sa(t[f"spatial_attention{s_}.in0"]), t[f"spatial_attention{s_}.out"], 1e-5, 1e-6, "attention alone" + s_)
    for name in ("cross_fusion_12", "cross_fusion_21"):
        close(getattr(net, name)(t[name + ".in0"], t[name + ".in1"]), t[name + ".out"], 1e-5, 2e-6, name)
    # 3x3 attention kernel (the class accepts 3 or 7) against torch on a ragged plane
    gen = torch.Generator().manual_seed(5)
    x3, w3 = torch.randn(2, 5, 7, 9, generator=gen).cuda(), torch.randn(1, 2, 3, 3, generator=gen).cuda()
    m3 = torch.cat([x3.mean(1, keepdim=True), x3.max(1, keepdim=True)[0]], 1)
    close(ops.spatial_attention(x3, w3), x3 * torch.sigmoid(torch.nn.functional.conv2d(m3.cpu(), w3.cpu(), padding=1)).cuda(), 1e-5, 1e-6, "3x3")
    res = net(g["x"].cuda())
    close(res[-1], g["out"], 2e-3, 1e-4, "DecompDualBranch")
    close(res[0], g["first"], 0, 0, "passthrough")
    net.train()                                   # the recording (training) forward computes the same function
    close(net(g["x"].cuda())[-1].detach(), res[-1], 1e-5, 1e-6, "train-mode forward")


def test_mc_pipeline_with_dualbranch_stage2_vs_oracle():
    """The Monte-Carlo loop of eval.py:199-297 with DecompDualBranch (Options/DecompDualBranch_4.yml) as the Stage-II net -- an arch whose
    decomposition cannot be hoisted out of the sample loop: N = 3 candidates of one 48x40 image (padded to 64x64) with injected weight
    epsilons and condition noise against oracle.eval_mc_ref(stage2=dualbranch_ref); PSNR within the north star's 1e-3 dB, same selection."""
    import bem.archs as A
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, _ = build_nets(n_feat=16, num_blocks=(1, 1, 1), device="cuda")
    torch.manual_seed(5)
    net2 = A.DecompDualBranch(in_channels=6, n_feat=16, d_state=[1, 1, 1], mlp_type="gdmlp", num_blocks=[1, 1, 1], decomp_model="model4").cuda().eval()
    sd1 = {k: v.detach().cpu() for k, v in net1.state_dict().items()}
    sd2 = {k: v.detach().cpu() for k, v in net2.state_dict().items()}
    lq, gt = synthetic_pair((1, 3, 48, 40), seed=12)
    N = 3
    g = torch.Generator().manual_seed(22)
    eps_cpu = [{(k[:-len("mu_weight")] + "weight" if k.endswith("mu_weight") else k[:-len("mu_bias")] + "bias"): torch.randn(v.shape, generator=g)
                for k, v in sd1.items() if k.endswith(("mu_weight", "mu_bias"))} for _ in range(N)]
    noise = [torch.randn(1, 3, 4, 4, generator=g) for _ in range(N)]
    ref = O.eval_mc_ref(sd1, sd2, lq, gt, N, eps_list=eps_cpu, noise_list=noise, gt_mean=True, scan=O.selective_scan_c, stage2=O.dualbranch_ref)
    pipe = BEMPipeline(net1, net2, 16, 0.1)
    eps = {k: torch.stack([e[k] for e in eps_cpu]).cuda() for k in eps_cpu[0]}
    out = pipe.enhance(lq.cuda(), gt.cuda(), N, gt_mean=True, eps=eps, noise=torch.cat(noise).cuda())
    for i in range(N):
        assert abs(float(out["psnr"][i]) - ref["psnr"][i]) < 1e-3, (i, float(out["psnr"][i]), ref["psnr"][i])
        close(out["final"][i].permute(1, 2, 0), ref["finals"][i], 0, 5e-4, f"candidate {i}")
    assert int(out["best"][0]) == ref["best"]


# ----------------------------------------------------------------------------- float64 yardstick --
# the oracle's algorithm with nothing cast down (tests/stage2_yardstick.py; its scan is checked against the per-step loop in
# tests/test_stage2_visibility.py)
_ss2d_core64, _iwt64 = Y.ss2d_core64, Y.iwt64


def test_stage2_within_f32_rounding_of_float64():
    """Who is closer to the exact result?  The oracle's algorithm is evaluated once more in float64 (same functions, the
    two f32 casts of the reference patched out) and used as the yardstick: the HIP Stage-II output must be no further from
    it than 2x the distance of the reference's own f32 CPU evaluation (full width, 128x128, seeded weights).  The x6
    GEMMs are individually closer to float64 than torch's f32 GEMM is (scripts/x6_acc.py, test_pw_gemm_x6_accuracy);
    this checks that nothing else on the path gives that away."""
    from unittest import mock
    import bem.archs as A
    torch.manual_seed(100)
    net = A.DecompDualBranchDDWavelet(in_channels=6, out_channels=3, n_feat=40, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                                      mlp_type="gdmlp", use_pixelshuffle=True, num_blocks=[2, 2, 2], decomp_model="model4")
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    x = torch.cat([0.25 * torch.rand(1, 3, 128, 128, generator=g), torch.rand(1, 3, 128, 128, generator=g)], 1)
    r32 = O.ddwavelet_ref(sd, x, O.selective_scan_c)
    with mock.patch.object(O, "ss2d_core_ref", _ss2d_core64), mock.patch.object(O, "iwt_ref", _iwt64):
        r64 = O.ddwavelet_ref({k: v.double() for k, v in sd.items()}, x.double(), None)
    assert r64.dtype == torch.float64
    out = net.cuda().eval()(x.cuda())[-1].cpu().double()
    e_ref, e_hip = (r32.double() - r64).abs(), (out - r64).abs()
    print(f"vs float64: reference f32 mean {e_ref.mean():.3e} max {e_ref.max():.3e} | HIP mean {e_hip.mean():.3e} max {e_hip.max():.3e}")
    assert e_hip.mean() <= 2 * e_ref.mean() + 1e-7 and e_hip.max() <= 2 * e_ref.max() + 1e-6


def test_pipeline_scorers_and_monte_carlo():
    """enhance() with the pluggable scorers: PSNR/SSIM-weighted full-reference rule and the CLIP stand-in (no-reference, index(max))
    choose what eval.py's list arithmetic chooses from the same score vectors; the Monte-Carlo mean comes with its PSNR / SSIM."""
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    from bem.scorers import ClipStandIn, FullReference
    net1, net2 = build_nets(n_feat=8, num_blocks=(1, 1, 1), seed=100, device="cuda")
    lq, gt = synthetic_pair((2, 3, 64, 64))
    pipe = BEMPipeline(net1, net2)
    N = 4
    r = pipe.enhance(lq.cuda(), gt.cuda(), N, gt_mean=True, seed=3, scorer=FullReference(0.4), monte_carlo=True)
    ps, ss = r["scores"].cpu().view(2, N), r["scores2"].cpu().view(2, N)
    assert r["best"] == [O.select_ref(ps[b].double().tolist(), ss[b].double().tolist(), 0.4) for b in range(2)]
    fin = r["final"].cpu()
    for bn in (0, 5):
        ref = O.ssim_ref(O.img_as_ubyte_ref(gt[bn // N].permute(1, 2, 0).numpy()), O.img_as_ubyte_ref(fin[bn].permute(1, 2, 0).numpy()))
        assert abs(float(ss.view(-1)[bn]) - ref) < 1e-6
    assert r["mc"].shape == (2, 3, 64, 64) and r["mc_psnr"].shape == (2,) and r["mc_ssim"].shape == (2,)
    pr = r["raw"].cpu()[:N, :, :64, :64].permute(0, 2, 3, 1).numpy()
    close(r["mc"][0].permute(1, 2, 0), torch.from_numpy(O.mc_mean_ref(pr, gt[0].permute(1, 2, 0).numpy(), True)), 2e-6, 2e-6, "mc")
    r2 = pipe.enhance(lq.cuda(), None, N, gt_mean=False, seed=3, scorer=ClipStandIn())
    s = r2["scores"].cpu().view(2, N)
    assert r2["best"] == [O.select_ref(no_ref_list=s[b].tolist(), no_ref="clip") for b in range(2)]


def test_eval_driver_cli(tmp_path):
    """Enhancement/eval.py with the reference's command line on two synthetic PNG pairs and seeded random checkpoints: runs, writes
    one PNG per input and result.txt, and its Best_PSNR equals the pipeline's own selection on the same inputs and seed."""
    import importlib.util
    from PIL import Image
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    spec = importlib.util.spec_from_file_location("bem_eval_driver", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    net1, net2 = build_nets(device="cpu")
    torch.save({"params": net1.state_dict()}, tmp_path / "cg.pth")
    torch.save({"params": {k: v for k, v in net2.state_dict().items()}}, tmp_path / "s2.pth")
    (tmp_path / "in").mkdir(); (tmp_path / "gt").mkdir()
    lq, gt = synthetic_pair((2, 3, 64, 64))
    for i in range(2):
        for d, t in (("in", lq), ("gt", gt)):
            Image.fromarray(np.rint(t[i].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(tmp_path / d / f"{i}.png")
    out = drv.main(["--opt", os.path.join(PKG, "Options", "CG_UNet_LOLv1.yml"), "--cond_opt", os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml"),
                    "--weights", str(tmp_path / "cg.pth"), "--cond_weights", str(tmp_path / "s2.pth"), "--input_dir", str(tmp_path / "in"),
                    "--target_dir", str(tmp_path / "gt"), "--result_dir", str(tmp_path / "res"), "--dataset", "synthetic", "--GT_mean",
                    "--num_samples", "3", "--psnr_weight", "0.5", "--Monte_Carlo", "--seed", "11"])
    assert sorted(os.listdir(out["result_dir"])) == ["0.png", "1.png", "result.txt"]
    txt = open(os.path.join(out["result_dir"], "result.txt")).read()
    assert "Best_PSNR" in txt and "Best_SSIM" in txt and "MC_PSNR" in txt
    assert len(out["psnr"]) == 2 and all(5 < p < 100 for p in out["psnr"]) and all(0 < s <= 1 for s in out["ssim"])


@pytest.mark.parametrize("tag", ["model2", "model3"])
def test_decomp_model2_model3_golden(tag):
    """QD model2 (dilated branch convolutions) / model3 (mini U-Net, eval mode) with the shipped weights against the outputs recorded
    from the reference (g5_decomp23.npz): the wavelet-domain maps the DDWavelet arch consumes and the full-resolution Q1 / Q2."""
    import bem.archs as A
    g = load_golden("g5_decomp23")
    img = g["img"].cuda()
    dw = A.Decomp.from_shipped(tag, wavelet_out=True).cuda()
    out = dw(img).cpu()
    close(out[:, :16], g[f"q1w_{tag}"], 2e-4, 2e-5, tag + " Q1_w"); close(out[:, 16:], g[f"q2w_{tag}"], 2e-4, 2e-5, tag + " Q2_w")
    df = A.Decomp.from_shipped(tag, wavelet_out=False).cuda()
    q = df(img).cpu()
    close(q[:, :4], g[f"q1_{tag}"], 2e-4, 2e-5, tag + " Q1"); close(q[:, 4:], g[f"q2_{tag}"], 2e-4, 2e-5, tag + " Q2")


@pytest.mark.parametrize("yml", ["DecompDualBranch2DDWavelet_4.yml", "DecompSingleBranch_1.yml"])
@pytest.mark.parametrize("dm", ["model2", "model3"])
def test_archs_build_and_run_with_every_decomp_model(yml, dm):
    """Every shipped Decomp* option file differs only in network_g.type and decomp_model: the *_2 / *_3 variants build
    and run, and agree with the oracle evaluated with the same weights."""
    from basicsr.archs import build_network
    from basicsr.utils.options import parse
    opt = parse(os.path.join(PKG, "Options", yml), is_train=False)
    ng = dict(opt["network_g"], decomp_model=dm, n_feat=8, num_blocks=[1, 1, 1])
    torch.manual_seed(3)
    net = build_network(ng).cuda().eval()
    x = torch.rand(1, 6, 32, 32, generator=torch.Generator().manual_seed(4))
    out = net(x.cuda())[-1].cpu()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    ref = (O.ddwavelet_ref if "Wavelet" in yml else O.singlebranch_ref)(sd, x, O.selective_scan_c, **({"decomp_model": dm}))
    close(out, ref, 2e-3, 1e-4, f"{yml} {dm}")


def test_full_width_stochastic_mc_vs_oracle():
    """The headline path at FULL WIDTH with stochastic weights: n_feat 40, blocks [2,2,2], shipped QD model4 decomposition, one 64x64 image,
    N = 4 Bayesian samples with injected weight epsilons and condition noise (eval.py:199-297, image_enhancer_model.py:165-216).  Every
    candidate's PSNR must agree with oracle.eval_mc_ref within 1e-3 dB (the north star's bar), candidates to 3e-4 (measured on the MI355X:
    max|d| 9.1e-5 over the four), same selected index."""
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, net2 = build_nets(device="cuda")
    sd1 = {k: v.detach().cpu() for k, v in net1.state_dict().items()}
    sd2 = {k: v.detach().cpu() for k, v in net2.state_dict().items()}
    lq, gt = synthetic_pair((1, 3, 64, 64), seed=11)
    N = 4
    g = torch.Generator().manual_seed(21)
    eps_cpu = [{(k[:-len("mu_weight")] + "weight" if k.endswith("mu_weight") else k[:-len("mu_bias")] + "bias"): torch.randn(v.shape, generator=g)
                for k, v in sd1.items() if k.endswith(("mu_weight", "mu_bias"))} for _ in range(N)]
    noise = torch.randn(N, 3, 4, 4, generator=g)
    ref = O.eval_mc_ref(sd1, sd2, lq, gt, N, gt_mean=True, eps_list=eps_cpu, noise_list=[noise[i:i + 1] for i in range(N)], scan=O.selective_scan_c)
    r = BEMPipeline(net1, net2, 16, 0.1).enhance(lq.cuda(), gt.cuda(), N, gt_mean=True, eps={k: torch.stack([e[k] for e in eps_cpu]).cuda() for k in eps_cpu[0]},
                                                noise=noise.cuda())
    fin = r["final"].cpu()
    for i in range(N):
        d = float((fin[i].permute(1, 2, 0) - torch.from_numpy(ref["finals"][i])).abs().max())
        print(f"candidate {i}: max|d| {d:.2e}")
        assert d < 3e-4, (i, d)
    dps = np.abs(np.asarray(ref["psnr"]) - r["psnr"].cpu().numpy())
    assert dps.max() < 1e-3, dps                                     # dB
    s = sorted(ref["psnr"], reverse=True)
    if s[0] - s[1] > 1e-3:
        assert int(r["best"][0]) == int(ref["best"])
    # the samples are different draws: the candidates must not coincide
    assert float((fin[0] - fin[1]).abs().max()) > 1e-4


def test_exchange_and_select_on_rccl_world1():
    """bem.dist on the `nccl` (= RCCL) backend with one rank: the all_gather_into_tensor form of the exchange runs on the device, and
    both exchange modes return the unsharded selection (N > 1 ranks are covered on gloo in tests/test_dist_cpu.py)."""
    import torch.distributed as dist
    from bem import dist as bdist
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        g = torch.Generator().manual_seed(2)
        Bn, N = 3, 4
        final = torch.rand(Bn * N, 3, 8, 6, generator=g).cuda()
        score = torch.rand(Bn * N, generator=g).cuda()
        score[4:8] = 0.5                                              # a tie image: first index wins
        ref_best = [int(torch.argmax(score[i * N:(i + 1) * N].cpu())) for i in range(Bn)]
        ref_best[1] = 0
        for mode in ("candidates", "scores"):
            img, best = bdist.exchange_and_select(final, score, N, 1, mode)
            assert best.tolist() == ref_best
            assert torch.equal(img, final.view(Bn, N, 3, 8, 6)[torch.arange(Bn), torch.tensor(ref_best)])
        # the collective itself, in the backend's tensor form (all_gather_into_tensor over RCCL), on both payloads of the exchange
        assert dist.get_backend() == "nccl"
        assert torch.equal(bdist._all_gather_rows(final, 1), final) and torch.equal(bdist._all_gather_rows(score, 1), score)
        assert torch.equal(bdist.gather_samples(final, Bn, N, 0, 1), final)
    finally:
        dist.destroy_process_group()


def test_bench_step_reproducible_under_full_load():
    """The bench's own step (8 images x 8 samples at 256x256, full width, Philox draws from a fixed seed) run three times: every candidate of
    every run must agree to 2e-6 (the only order-dependent sums are the f64 attention statistics and score reductions).  This is the load
    under which the gfx950 stale-register hazard of DESIGN.md section 6.4 fires (several workgroups per CU in every kernel): a wrong
    output there is off by a whole bias value, not by rounding."""
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, net2 = build_nets(device="cuda")
    pipe = BEMPipeline(net1, net2, 16, 0.1)
    lq, gt = synthetic_pair((8, 3, 256, 256), seed=287128, device="cuda")
    from bem.modules import SampleCtx
    runs = []
    for _ in range(3):
        SampleCtx._epoch = 77000                      # the forward counter keys the Philox streams: rewind it, so the three runs draw the same weights
        r = pipe.enhance(lq, gt, 8, gt_mean=True, seed=4242, sync=False)
        runs.append((r["final"].clone(), r["psnr"].clone(), r["best"].clone() if torch.is_tensor(r["best"]) else r["best"]))
    torch.cuda.synchronize()
    for f, p, b in runs[1:]:
        d = float((f - runs[0][0]).abs().max())
        assert d <= 2e-6, d
        assert float((p - runs[0][1]).abs().max()) <= 1e-4
    # the first stochastic forward draws its weight sets leaf by leaf (90 launches) and records the streams; the later ones make all draws in
    # one launch (EvalSampleBank) from those same streams -- the runs above therefore compare the two forms
    from bem.modules import EvalSampleBank
    bank = EvalSampleBank.of(net1)
    assert bank is not None and bank.sig is not None and bank.nrows == sum(2 if m.bias else 1 for m in bank.leaves) == 90
    assert torch.isfinite(runs[0][0]).all()


def test_sample_major_blocks_equal_unsharded_candidates():
    """What a rank computes under sample-major sharding (bem.dist, Enhancement/eval.py under torchrun): `BEMPipeline.candidates` for a block
    [lo, hi) of the N samples with the epsilons / noise of ALL rows handed in.  The blocks of a two-rank split (N = 5: 3 + 2), put back in
    (image, sample) order exactly as `gather_samples` does, must equal the unsharded call: candidates, conditions and scores -- hence the
    same first-maximum selection (the gather itself runs on gloo in tests/test_dist_cpu.py, the collective on RCCL in the world-1 test)."""
    from bem.dist import shard_samples
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, net2 = build_nets(n_feat=16, num_blocks=(1, 1, 1), seed=100, device="cuda")
    sd1 = net1.state_dict()
    lq, gt = synthetic_pair((2, 3, 64, 64), seed=9)
    B, N, world = 2, 5, 2
    g = torch.Generator().manual_seed(3)
    eps = {(k[:-len("mu_weight")] + "weight" if k.endswith("mu_weight") else k[:-len("mu_bias")] + "bias"): torch.randn((B * N,) + tuple(v.shape), generator=g).cuda()
           for k, v in sd1.items() if k.endswith(("mu_weight", "mu_bias"))}
    noise = torch.randn(B * N, 3, 4, 4, generator=g).cuda()
    pipe = BEMPipeline(net1, net2, 16, 0.1)
    full = pipe.candidates(lq.cuda(), gt.cuda(), N, True, eps=eps, noise=noise)
    parts = []
    for rank in range(world):
        lo, hi = shard_samples(N, rank, world)
        parts.append((lo, hi, pipe.candidates(lq.cuda(), gt.cuda(), hi - lo, True, eps=eps, noise=noise, rank=rank, sample_offset=lo, total_samples=N)))
    for key in ("final", "psnr", "conds"):
        rows = []
        for b in range(B):
            for lo, hi, r in parts:
                n = hi - lo
                rows.append(r[key][b * n:(b + 1) * n])
        got = torch.cat(rows)
        close(got, full[key], 1e-5, 1e-6, f"sample-major {key}")


# ------------------------------------------------------------- shipped sizes, recurrence-dominated weights, float64 yardstick --
def _yardstick(out, r32, r64, what):
    """HIP no further from float64 than 2x the f32 oracle, mean and max (tests/test_stage2_visibility.py: every block moved by
    1e-3 moves the output by >= 5x this bound)."""
    (rm, rM), (hm, hM) = Y.errors(r32, r64), Y.errors(out, r64)
    print(f"{what} vs float64: f32 oracle mean {rm:.3e} max {rM:.3e} | HIP mean {hm:.3e} max {hM:.3e} "
          f"({hm / rm:.2f}x, {hM / rM:.2f}x) | max|out| {r64.abs().max():.3f}")
    assert torch.isfinite(out).all()
    assert hm <= 2 * rm and hM <= 2 * rM, (what, hm, rm, hM, rM)


@pytest.mark.parametrize("name,batch", [(n, 1) for n in Y.SIBLINGS] + [("DecompDualBranchDDWavelet", 2)])
def test_stage2_shipped_size_vs_float64(name, batch):
    """Each Stage-II arch as its Options/*.yml ships it (n_feat 40, [2,2,2], its decomposition model) at 256x256 -- DDWavelet at
    config 2's batch of 2 -- with the recurrence-dominated weights of tests/stage2_yardstick.py: level 0 runs the chunked scan with 32
    carries, the 3x3 tap form at W = 256, the 4x4-s2 im2col kernel at Wo = 128, SE and 7x7 attention on 64x64 bottlenecks."""
    from bem import ops
    net = Y.build_arch(name)
    sd = Y.recurrence_dominated({k: v.detach().clone() for k, v in net.state_dict().items()}, 7)
    net.load_state_dict(sd, strict=True)
    ops.bump_weight_epoch()
    g = torch.Generator().manual_seed(11)
    x = torch.cat([0.25 * torch.rand(batch, 3, 256, 256, generator=g), torch.rand(batch, 3, 256, 256, generator=g)], 1)
    out = net.cuda().eval()(x.cuda())[-1].cpu()
    _yardstick(out, Y.oracle(name, sd, x, O.selective_scan_c), Y.float64_ref(name, sd, x), f"{name} 256x256 batch {batch}")


def _config5_nets():
    """build_nets() with the Stage-II net moved to the recurrence-dominated operating point (before its first forward)."""
    from bem import ops
    from bem.pipeline import build_nets
    net1, net2 = build_nets(device="cuda")
    sd2 = Y.recurrence_dominated({k: v.detach().cpu().clone() for k, v in net2.state_dict().items()}, 7)
    net2.load_state_dict(sd2, strict=True)
    ops.bump_weight_epoch()
    return net1, net2, {k: v.detach().cpu() for k, v in net1.state_dict().items()}, sd2


def _stage2_input(lq, cond):
    """The Stage-II input of eval.py for a 400x600 image: reflect-padded to 448x640, condition bilinear x16."""
    pad = torch.from_numpy(np.ascontiguousarray(O.pad_reflect_ref(lq[0].permute(1, 2, 0).numpy(), 64))).permute(2, 0, 1)[None]
    return torch.cat([pad, torch.nn.functional.interpolate(cond, scale_factor=16, mode="bilinear", align_corners=False)], 1)


def test_stage2_config5_vs_float64():
    """Config 5, Stage II in isolation at 448x640 (level 0: L = 71680, the chunked scan with 35 carries; levels 1 / 2: 112x160 / 56x80 on
    the generic scan) with the recurrence-dominated weights, on the condition the HIP Stage I produced for a 400x600 image."""
    from bem.pipeline import BEMPipeline, synthetic_pair
    net1, net2, _, sd2 = _config5_nets()
    lq, gt = synthetic_pair((1, 3, 400, 600), seed=5)
    noise = torch.randn(1, 3, 28, 40, generator=torch.Generator().manual_seed(9))
    r = BEMPipeline(net1, net2).enhance(lq.cuda(), gt.cuda(), 1, gt_mean=True, deterministic=True, noise=noise.cuda())
    x = _stage2_input(lq, r["conds"].cpu())
    out = net2(x.cuda())[-1].cpu()
    name = "DecompDualBranchDDWavelet"
    _yardstick(out, Y.oracle(name, sd2, x, O.selective_scan_c), Y.float64_ref(name, sd2, x), "config-5 Stage II 448x640")


def test_config5_monte_carlo_vs_oracle():
    """Config 5's Monte-Carlo loop: one 400x600 image, N = 4 Bayesian samples with injected weight epsilons and condition noise, Stage II
    at the recurrence-dominated operating point.  Stage I per sample (per-sample weight sets on 28x40 .. 7x10 planes) against the oracle's
    conditions (measured max|d| 5.7e-5); Stage II on the four HIP conditions in one batch against the float64 yardstick on each; every
    candidate's PSNR within 1e-3 dB; the same selected index.  The noisy conditions make Stage II ill-conditioned here: where a pixel's
    channel maximum comes close to 0, the decomposition's q1 = RGB / (max + 1e-7) is large, and the f32 oracle itself is up to 1e-2 from
    float64 at outputs of ~1e4 -- hence the yardstick bound, not a fixed one."""
    from bem.pipeline import BEMPipeline, synthetic_pair
    net1, net2, sd1, sd2 = _config5_nets()
    lq, gt = synthetic_pair((1, 3, 400, 600), seed=13)
    N = 4
    g = torch.Generator().manual_seed(23)
    eps_cpu = [{(k[:-len("mu_weight")] + "weight" if k.endswith("mu_weight") else k[:-len("mu_bias")] + "bias"): torch.randn(v.shape, generator=g)
                for k, v in sd1.items() if k.endswith(("mu_weight", "mu_bias"))} for _ in range(N)]
    noise = torch.randn(N, 3, 28, 40, generator=g)
    ref = O.eval_mc_ref(sd1, sd2, lq, gt, N, gt_mean=True, eps_list=eps_cpu, noise_list=[noise[i:i + 1] for i in range(N)], scan=O.selective_scan_c)
    r = BEMPipeline(net1, net2, 16, 0.1).enhance(lq.cuda(), gt.cuda(), N, gt_mean=True, eps={k: torch.stack([e[k] for e in eps_cpu]).cuda() for k in eps_cpu[0]},
                                                noise=noise.cuda())
    assert r["conds"].shape == (N, 3, 28, 40) and r["raw"].shape == (N, 3, 448, 640)
    conds = r["conds"].cpu()
    xs = [_stage2_input(lq, conds[i:i + 1]) for i in range(N)]
    out = net2(torch.cat(xs).cuda())[-1].cpu()                       # the N candidates in one batch
    name = "DecompDualBranchDDWavelet"
    for i in range(N):
        close(conds[i:i + 1], ref["conds"][i], 0, 1e-4, f"condition {i}")
        _yardstick(out[i:i + 1], Y.oracle(name, sd2, xs[i], O.selective_scan_c), Y.float64_ref(name, sd2, xs[i]), f"config-5 MC sample {i}")
    dps = np.abs(np.asarray(ref["psnr"]) - r["psnr"].cpu().numpy())
    assert dps.max() < 1e-3, dps                                     # dB
    s = sorted(ref["psnr"], reverse=True)
    if s[0] - s[1] > 1e-3:
        assert int(r["best"][0]) == int(ref["best"])
    assert float((out[0] - out[1]).abs().max()) > 1e-3                # the samples are different draws
