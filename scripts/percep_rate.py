#!/usr/bin/env python3
"""Rate of the VGG19 perceptual loss on the GPU (HIP events, warm-up, seeded weights):

  1. ms of PerceptualLoss({'conv5_4': 1}, weight 0.01) forward + backward at batch 16, 256x256, and the memory the node keeps
     between the two;
  2. the same split per VGG block: each block's convolutions forward on the 2B-row batch and their input-gradient convolutions on the
     B-row half, with the GFLOP they stand for and the rate that makes;
  3. a DecompDualBranchDDWavelet training step (Options/DecompDualBranch2DDWavelet_4.yml's net, batch 16, 256x256) with and without
     the term, the two alternating in one run.

  python scripts/percep_rate.py [--batch 16] [--size 256] [--iters 5] [--out profiles/percep_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-enhancement-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


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


def seeded_state_dict(seed=5):
    """Kaiming-normal weights and small biases for all 16 convolutions, keyed like torchvision's vgg19 state dict."""
    from bem.percep import VGG19_NAMES, conv_shape
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, n in enumerate(VGG19_NAMES):
        if n.startswith("conv"):
            shp = conv_shape(n)
            sd[f"features.{i}.weight"] = torch.randn(shp, generator=g) * (2.0 / (shp[0] * 9)) ** 0.5
            sd[f"features.{i}.bias"] = torch.randn(shp[0], generator=g) * 0.05
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "percep_rate.txt"))
    a = ap.parse_args()
    from bem import ops
    from bem.percep import VGG19_NAMES, PerceptualLoss, conv_shape
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    sd = seeded_state_dict()
    lines = [f"percep_rate: {torch.cuda.get_device_name(0)}, batch {B}, {S}x{S}, median of {a.iters} after 2 warm-up runs, HIP events"]

    # ---- 1. the loss, forward + backward ----
    crit = PerceptualLoss({"conv5_4": 1.0}, perceptual_weight=0.01, state_dict=sd).to(dev)
    g = torch.Generator().manual_seed(1)
    pred = torch.rand(B, 3, S, S, generator=g).to(dev).requires_grad_(True)
    gt = torch.rand(B, 3, S, S, generator=g).to(dev)

    def fwd_bwd():
        pred.grad = None
        crit(pred, gt)[0].backward()

    def fwd():
        with torch.no_grad():
            crit(pred, gt)
    t_fb, t_f = timed(fwd_bwd, a.iters), timed(fwd, a.iters)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = crit(pred, gt)[0]
    torch.cuda.synchronize()
    held, peak = torch.cuda.memory_allocated() - base, torch.cuda.max_memory_allocated() - base
    del loss
    lines.append(f"PerceptualLoss conv5_4: forward + backward {t_fb:.2f} ms, forward alone (no grad) {t_f:.2f} ms; "
                 f"held between forward and backward {held / 2**30:.2f} GiB, peak inside the forward {peak / 2**30:.2f} GiB")

    # ---- 2. per block: the convolutions forward (2B rows, ReLU fused) and their input gradients (B rows) ----
    w = crit.vgg.conv_operands()
    H = S
    tot_f = tot_b = 0.0
    lines.append("block  plane      convs  fwd ms  fwd TF/s  bwd ms  bwd TF/s   (fwd: 2B rows; bwd: input gradients, B rows; f32 GEMM flops)")
    for blk in range(1, 6):
        names = [n for n in VGG19_NAMES if n.startswith(f"conv{blk}_")]
        shapes = [conv_shape(n) for n in names]
        cin0 = 8 if blk == 1 else shapes[0][1]
        x = torch.rand(2 * B, cin0, H, H, device=dev)
        dy = torch.rand(B, shapes[-1][0], H, H, device=dev)

        def f_blk():
            t = x
            for n in names:
                t = ops.conv2d(t, w[n][0], w[n][1], relu=True)

        def b_blk():
            t = dy
            for n in reversed(names):
                t = ops.conv2d(t, w[n][0].input_grad(), None)
        tf, tb = timed(f_blk, a.iters), timed(b_blk, a.iters)
        fl = sum(2.0 * co * ci * 9 * H * H for co, ci, _, _ in shapes)
        lines.append(f"{blk:>5}  {H:>3}x{H:<3}  {len(names):>7}  {tf:6.2f}  {2 * B * fl / tf / 1e9:8.1f}  {tb:6.2f}  {B * fl / tb / 1e9:8.1f}")
        tot_f, tot_b = tot_f + tf, tot_b + tb
        H //= 2
    lines.append(f"convolutions: forward {tot_f:.2f} ms, backward {tot_b:.2f} ms; the rest of forward + backward (prep, pools, ReLU masks, L1, row "
                 f"copies) {t_fb - tot_f - tot_b:.2f} ms")

    # ---- 3. the training step with and without the term, alternating ----
    import yaml

    from basicsr.models import build_model
    with open(os.path.join(ROOT, "bayesian-enhancement-model_amd", "Options", "DecompDualBranch2DDWavelet_4.yml")) as f:
        opt = yaml.safe_load(f)
    opt.update(is_train=True, dist=False, rank=0, world_size=1)
    opt["path"] = dict(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    import copy
    opt_p = copy.deepcopy(opt)
    opt_p["train"]["perceptual_opt"] = dict(type="PerceptualLoss", layer_weights={"conv5_4": 1}, vgg_type="vgg19", use_input_norm=True,
                                            range_norm=False, perceptual_weight=0.01, style_weight=0, criterion="l1")
    import tempfile
    fd, path = tempfile.mkstemp(suffix=".pth")
    os.close(fd)
    torch.save(sd, path)
    os.environ["BEM_VGG19_WEIGHTS"] = path
    del crit, w
    torch.manual_seed(100)
    m0 = build_model(opt)
    torch.manual_seed(100)
    m1 = build_model(opt_p)
    os.remove(path)
    import torch.nn.functional as F
    from bem.pipeline import synthetic_pair
    lq, gtt = synthetic_pair((B, 3, S, S), seed=9)
    data = dict(lq=lq.to(dev), gt=gtt.to(dev), gt_down=F.interpolate(gtt, scale_factor=1 / 16, mode="bilinear").to(dev))
    it = [0]

    def step(m):
        def run():
            it[0] += 1
            m.feed_train_data(data)
            m.optimize_parameters(it[0])
        return run
    t0, t1 = [], []
    for r in range(3):                                   # L1, L1 + perceptual, L1, ...: both see the same clocks and neighbours
        t0.append(timed(step(m0), a.iters, warmup=2 if r == 0 else 1))
        t1.append(timed(step(m1), a.iters, warmup=2 if r == 0 else 1))
    m0_, m1_ = sorted(t0)[1], sorted(t1)[1]
    lines.append(f"training step DecompDualBranchDDWavelet n_feat 40: L1 only {m0_:.2f} ms ({B / m0_ * 1e3:.0f} img/s), "
                 f"L1 + perceptual {m1_:.2f} ms ({B / m1_ * 1e3:.0f} img/s), the term adds {m1_ - m0_:.2f} ms   "
                 f"(rounds: {', '.join(f'{x:.2f}/{y:.2f}' for x, y in zip(t0, t1))})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
