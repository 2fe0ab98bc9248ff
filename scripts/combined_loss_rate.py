#!/usr/bin/env python3
"""Rate of the CombinedLoss term on the GPU (HIP events, warm-up), against a torch-on-GPU restatement of the same four statistics:

  1. ms of the pixstat forward (with the backward's record) and of forward + backward at (16,3,256,256): the HIP kernels
     (bem.ops.pixstat_loss / pixstat_loss_bwd) and the restatement below (torch ops + autograd), the two forms alternating in one process,
     three repeats, the spread between the repeats quoted; the achieved bytes/s of the two streaming kernels from their algorithmic
     traffic (forward 8 B per element: pred and gt read once; backward 12 B: both read, dpred written);
  2. ms of the whole CombinedLoss (pixstat + SSIM + VGG19[:16]-MSE, seeded VGG weights), forward + backward;
  3. ms of a DecompDualBranchDDWavelet training step (Options/DecompDualBranch2DDWavelet_4.yml's net, batch 16, 256x256) with its own
     losses, and with ``train.combined_opt`` (the recipe's defaults) beside them, the two alternating in one run.

  python scripts/combined_loss_rate.py [--iters 10] [--hbm_tbs 8.0] [--out profiles/combined_loss_rate.txt]
"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-enhancement-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ALPHAS = (1.00, 0.05, 0.0083, 0.25)            # alpha1, alpha3, alpha5, alpha6


def timed(fn, iters, warmup=2):
    """Median ms of fn() over ``iters`` runs, each between its own pair of events."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return sorted(ms)[len(ms) // 2]


def torch_pixstat(y_pred, y_true):
    """my_loss.py:22-49 and :70-72 without the SSIM and VGG terms, in torch's own ops (the yardstick; its code is fixed)."""
    sl1 = F.smooth_l1_loss(y_true, y_pred)
    mse = F.mse_loss(y_true, y_pred)
    psnr = 40.0 - torch.mean(20 * torch.log10(1.0 / torch.sqrt(mse)))
    color = torch.mean(torch.abs(torch.mean(y_true, dim=[1, 2, 3]) - torch.mean(y_pred, dim=[1, 2, 3])))
    ht, hp = torch.histc(y_true, bins=256, min=0.0, max=1.0), torch.histc(y_pred, bins=256, min=0.0, max=1.0)
    hist = torch.mean(torch.abs(ht / ht.sum() - hp / hp.sum()))
    return ALPHAS[0] * sl1 + ALPHAS[1] * hist + ALPHAS[2] * psnr + ALPHAS[3] * color


def spread(v):
    return f"{sorted(v)[1]:.3f} ms (repeats {', '.join(f'{x:.3f}' for x in v)})"


def seeded_vgg(upto=7, seed=5):
    """A torchvision-keyed state dict for vgg19.features[:16] with seeded weights (the rate does not depend on their values)."""
    g, sd, cin, idx = torch.Generator().manual_seed(seed), {}, 3, 0
    for width, depth in ((64, 2), (128, 2), (256, 4)):
        for _ in range(depth):
            if len(sd) // 2 < upto:
                sd[f"features.{idx}.weight"] = torch.randn(width, cin, 3, 3, generator=g) * (2.0 / (width * 9)) ** 0.5
                sd[f"features.{idx}.bias"] = torch.randn(width, generator=g) * 0.05
            cin, idx = width, idx + 2
        idx += 1
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--hbm_tbs", type=float, default=8.0, help="HBM peak in TB/s for the roofline fraction (MI355X: 8.0)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combined_loss_rate.txt"))
    a = ap.parse_args()
    from basicsr.losses import build_loss
    from bem import ops
    dev = torch.device("cuda", 0)
    lines = [f"combined_loss_rate: {torch.cuda.get_device_name(0)}, median of {a.iters} after warm-up, HIP events, HIP and torch forms alternating, 3 repeats"]

    # ---- 1. pixstat forward and forward + backward, HIP against the torch restatement ----
    shape = (16, 3, 256, 256)
    gen = torch.Generator().manual_seed(1)
    gt = torch.rand(shape, generator=gen)
    pred = (gt + 0.1 * torch.randn(shape, generator=gen)).to(dev)                  # unclamped, as a network's output is
    gt = gt.to(dev)
    one = torch.ones(1, device=dev)
    xt = pred.clone().requires_grad_(True)

    def h_fwd():
        return ops.pixstat_loss(pred, gt, ALPHAS, want_grad=True)

    def h_fb():
        ops.pixstat_loss_bwd(pred, gt, h_fwd()[1], one)

    def t_fwd():
        return torch_pixstat(xt, gt)

    def t_fb():
        xt.grad = None
        t_fwd().backward()
    _, rec = h_fwd()
    hip_l, tor_l = float(h_fwd()[0][0]), float(t_fwd().detach())
    hf, hfb, hb, tf, tfb = [], [], [], [], []
    for _ in range(3):
        hf.append(timed(h_fwd, a.iters))
        tf.append(timed(t_fwd, a.iters))
        hfb.append(timed(h_fb, a.iters))
        tfb.append(timed(t_fb, a.iters))
        hb.append(timed(lambda: ops.pixstat_loss_bwd(pred, gt, rec, one), a.iters))
    nb, nbb = ops.pixstat_loss_cost(pred)[0], ops.pixstat_loss_bwd_cost(pred)[0]
    mhf, mhfb, mhb, mtf, mtfb = (sorted(v)[1] for v in (hf, hfb, hb, tf, tfb))
    lines += [f"{shape}: pixstat loss HIP {hip_l:.6f}, torch {tor_l:.6f}",
              f"  forward            HIP {spread(hf)}   torch {spread(tf)}   torch / HIP {mtf / mhf:.2f}",
              f"  forward + backward HIP {spread(hfb)}   torch {spread(tfb)}   torch / HIP {mtfb / mhfb:.2f}",
              f"  backward alone     HIP {spread(hb)}",
              f"  forward (two launches and the 2 KiB memset): {nb / 1e6:.1f} MB algorithmic (8 B per element) -> {nb / mhf / 1e9:.3f} TB/s, "
              f"{100 * nb / mhf / 1e9 / a.hbm_tbs:.1f} % of {a.hbm_tbs} TB/s; backward: {nbb / 1e6:.1f} MB (12 B per element) -> "
              f"{nbb / mhb / 1e9:.3f} TB/s, {100 * nbb / mhb / 1e9 / a.hbm_tbs:.1f} %"]

    # ---- 2. the whole CombinedLoss ----
    crit = build_loss(dict(type="CombinedLoss", state_dict=seeded_vgg())).to(dev)
    xc = pred.clone().requires_grad_(True)

    def c_fb():
        xc.grad = None
        crit(xc, gt).backward()
    cf = [timed(c_fb, a.iters) for _ in range(3)]
    parts = ", ".join(f"{k} {float(v):.4f}" for k, v in crit.parts.items())
    lines.append(f"  CombinedLoss (pixstat + SSIM + VGG19[:16]-MSE) forward + backward: {spread(cf)}; pixstat is {100 * mhfb / sorted(cf)[1]:.1f} % of it   ({parts})")

    # ---- 3. the training step with and without the block, alternating ----
    import yaml

    from basicsr.models import build_model
    from bem.pipeline import synthetic_pair
    with open(os.path.join(ROOT, "bayesian-enhancement-model_amd", "Options", "DecompDualBranch2DDWavelet_4.yml")) as f:
        opt = yaml.safe_load(f)
    opt.update(is_train=True, dist=False, rank=0, world_size=1)
    opt["path"] = dict(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    opt_c = copy.deepcopy(opt)
    opt_c["train"]["combined_opt"] = dict(type="CombinedLoss", state_dict=seeded_vgg())
    opt_p = copy.deepcopy(opt)
    opt_p["train"]["combined_opt"] = dict(type="CombinedLoss", alpha2=0, alpha4=0)
    models = []
    for o in (opt, opt_p, opt_c):
        torch.manual_seed(100)
        models.append(build_model(o))
    B, S = 16, 256
    lq, gtt = synthetic_pair((B, 3, S, S), seed=9)
    data = dict(lq=lq.to(dev), gt=gtt.to(dev), gt_down=F.interpolate(gtt, scale_factor=1 / 16, mode="bilinear").to(dev))
    it = [0]

    def step(m):
        def run():
            it[0] += 1
            m.feed_train_data(data)
            m.optimize_parameters(it[0])
        return run
    n = max(3, a.iters // 2)
    ts = [[], [], []]
    for r in range(3):
        for t, m in zip(ts, models):
            t.append(timed(step(m), n, warmup=2 if r == 0 else 1))
    a0, ap_, ac = (sorted(t)[1] for t in ts)
    own = " + ".join(k for k in models[0].log_dict)
    lines.append(f"training step DecompDualBranchDDWavelet n_feat 40, batch {B}, {S}x{S}: {own} only {a0:.2f} ms; + combined_opt with alpha2 = alpha4 = 0 "
                 f"(pixstat alone) {ap_:.2f} ms, adds {ap_ - a0:.2f} ms = {100 * (ap_ - a0) / ap_:.2f} % of the step; + combined_opt (all six parts) {ac:.2f} ms, "
                 f"adds {ac - a0:.2f} ms = {100 * (ac - a0) / ac:.2f} %   (rounds: {', '.join(f'{x:.2f}/{y:.2f}/{z:.2f}' for x, y, z in zip(*ts))}; "
                 f"l_comb {float(models[2].log_dict['l_comb']):.4f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
