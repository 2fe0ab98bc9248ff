#!/usr/bin/env python3
"""Cost of the averaged weights (train.ema_decay) per training step (HIP events, warm-up, seeded synthetic data):

  1. a Stage-II (Options/DecompDualBranch2DDWavelet_4.yml, batch 8, 128x128) and a Stage-I (Options/CG_UNet_LOLv1.yml, batch 8, the
     captured-graph path) training step with ``ema_decay`` absent and with 0.999: two models built from the same seed, alternating in one
     process, five rounds of --steps steps, each after 10 warm-up steps; medians and the spread between rounds;
  2. bem_ema_update_f32 alone on the Stage-II model's flat buffers: device events around --launches launches.

  python scripts/ema_rate.py [--steps 40] [--launches 200] [--off-only] [--out profiles/ema_rate.txt]

``--off-only`` measures the rows without EMA only: the form that also runs on a tree from before the feature, for the comparison of the
unchanged step with its parent.
"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bayesian-enhancement-model_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WARM, ROUNDS, DECAY = 10, 5, 0.999


def steps_ms(model, loader, epoch, count, it0):
    loader.set_epoch(epoch)
    it = iter(loader)
    for k in range(WARM):                                # lazy buffers, the captured graph of Stage I, and the clocks of a round's first steps
        model.feed_train_data(next(it))
        model.optimize_parameters(it0 + k + 1)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for k in range(count):
        model.feed_train_data(next(it))
        model.optimize_parameters(it0 + WARM + 1 + k)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / count


def kernel_us(model, launches):
    """us per bem_ema_update_f32 launch over the model's flat buffers (all groups), and the bytes one such pass moves."""
    from bem import ops
    pairs = model.weight_ema._pairs
    scratch = [(e.clone(), p) for e, p in pairs]         # the timing must not move the model's average
    for _ in range(20):
        for e, p in scratch:
            ops.ema_update_(e, p, DECAY)
    torch.cuda.synchronize()
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        for e, p in scratch:
            ops.ema_update_(e, p, DECAY)
    t.record()
    t.synchronize()
    return s.elapsed_time(t) * 1e3 / launches, 12 * sum(e.numel() for e, _ in scratch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_rate.txt"))
    a = ap.parse_args()
    import yaml

    from basicsr.data import build_dataloader, build_dataset
    from basicsr.models import build_model
    dev = torch.device("cuda", 0)
    B, S = 8, 128
    lines = [f"ema_rate: {torch.cuda.get_device_name(0)}, batch {B}, {S}x{S}, synthetic pairs on the device; HIP events around {a.steps} steps, "
             f"{ROUNDS} rounds after {WARM} warm-up steps each" + ("" if a.off_only else f", ema_decay absent / {DECAY} alternating in one process")]
    for yml, tag in (("DecompDualBranch2DDWavelet_4.yml", "Stage II"), ("CG_UNet_LOLv1.yml", "Stage I (graph replay)")):
        with open(os.path.join(PKG, "Options", yml)) as f:
            opt = yaml.safe_load(f)
        opt.update(is_train=True, dist=False, rank=0, world_size=1)
        opt["path"] = dict(pretrain_network_g=None, strict_load_g=True, resume_state=None)
        opt["train"].pop("ema_decay", None)
        dopt = dict(type="Synthetic", num_images=64, image_size=S, gt_size=S, batch_size_per_gpu=B, use_shuffle=True, dataset_enlarge_ratio=8,
                    condition=opt.get("condition", {"type": "mean", "scale_down": 16}), model_type=opt["model_type"], phase="train")
        if opt["model_type"] == "ConditionGenerator":
            dopt["mask_ratio"] = 0.4
        loader = build_dataloader(build_dataset(dopt), dopt, seed=100, device=dev, train=True)
        torch.manual_seed(100)
        m_off = build_model(copy.deepcopy(opt))
        m_on = None
        if not a.off_only:
            opt["train"]["ema_decay"] = DECAY
            torch.manual_seed(100)
            m_on = build_model(copy.deepcopy(opt))
        t_off, t_on, it0 = [], [], 0
        for r in range(ROUNDS):
            t_off.append(steps_ms(m_off, loader, r, a.steps, it0))
            if m_on is not None:
                t_on.append(steps_ms(m_on, loader, r, a.steps, it0))
            it0 += a.steps + WARM
        med = lambda t: sorted(t)[len(t) // 2]
        nparam = sum(p.numel() for p in m_off.net_g.parameters() if p.requires_grad)
        line = (f"{tag} ({yml}, {nparam} trained parameters): ema off {med(t_off):.3f} ms per step, spread between rounds "
                f"{max(t_off) - min(t_off):.3f} ms (rounds: {', '.join(f'{x:.3f}' for x in t_off)})")
        if m_on is not None:
            line += (f"; ema {DECAY} {med(t_on):.3f} ms, spread {max(t_on) - min(t_on):.3f} ms (rounds: {', '.join(f'{x:.3f}' for x in t_on)}); "
                     f"difference of the medians {med(t_on) - med(t_off):+.3f} ms")
        lines.append(line)
        if m_on is not None and opt["model_type"] == "ImageEnhancer":
            us, nbytes = kernel_us(m_on, a.launches)
            lines.append(f"bem_ema_update_f32 alone on the Stage-II flat buffers ({nbytes / 12:.0f} floats, {nbytes / 1e6:.1f} MB per pass): "
                         f"{us:.2f} us per pass over {a.launches} back-to-back passes = {nbytes / us / 1e3:.0f} GB/s")
        del m_off, m_on
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
