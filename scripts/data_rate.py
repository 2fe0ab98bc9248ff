#!/usr/bin/env python3
"""Rate of batch assembly from the device-resident image store against the tensor shim (HIP events, warm-up, seeded data):

  1. 485 seeded pairs of 400x600 (LOLv1's shape), held once in the uint8 store of basicsr.data.paired_image_dataset and once as the
     float tensors of the shim's TensorPairs;
  2. ms per batch of both loaders at batch 8, gt_size 128, geometric_augs on: device events around 200 batches, the two loaders
     alternating in one process after a warm-up pass, three repeats (the epoch plan / permutation is made before the first event);
  3. a Stage-I (Options/CG_UNet_LOLv1.yml) and a Stage-II (Options/DecompDualBranch2DDWavelet_4.yml) training step fed by each: five
     alternating rounds of --steps steps, each after 10 warm-up steps.

  python scripts/data_rate.py [--pairs 485] [--batches 200] [--steps 40] [--out profiles/data_rate.txt]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_datasets(n, H, W, dev):
    """The same n pairs as a PairedImageMaskDataset (host uint8 arenas) and as a TensorPairDataset (float (N,3,H,W), already on the device)."""
    from basicsr.data import TensorPairDataset
    from basicsr.data.paired_image_dataset import PairedImageMaskDataset
    g = torch.Generator(device=dev).manual_seed(485)
    gt = torch.randint(0, 256, (n, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    lq = (gt.float() * 0.2).to(torch.uint8)
    store = PairedImageMaskDataset.__new__(PairedImageMaskDataset)
    store.opt = {"name": "rate"}
    store.lq, store.gt = lq.reshape(-1).cpu().numpy(), gt.reshape(-1).cpu().numpy()
    store.table = np.stack([np.arange(n, dtype=np.int64) * H * W * 3, np.full(n, H, np.int64), np.full(n, W, np.int64)], 1)
    store.paths = [dict(lq_path=f"lq/{i:04d}.png", gt_path=f"gt/{i:04d}.png") for i in range(n)]
    shim = TensorPairDataset.__new__(TensorPairDataset)
    shim.opt = {"name": "rate"}
    shim.lq, shim.gt = (lq.permute(0, 3, 1, 2).float() / 255).contiguous(), (gt.permute(0, 3, 1, 2).float() / 255).contiguous()
    return store, shim


def batches_ms(loader, epoch, count):
    """ms per batch over ``count`` batches of one epoch; the iterator is primed (plan / permutation made, one batch drawn) before the first event."""
    loader.set_epoch(epoch)
    it = iter(loader)
    next(it)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(count):
        next(it)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / count


WARM = 10


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=485)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_rate.txt"))
    a = ap.parse_args()
    import yaml

    from basicsr.data import build_dataloader
    from basicsr.models import build_model
    dev = torch.device("cuda", 0)
    B, S, H, W = 8, 128, 400, 600
    store, shim = make_datasets(a.pairs, H, W, dev)
    need = max(a.batches, a.steps + WARM) + 8
    ratio = -(-need * B // a.pairs)
    dopt = dict(batch_size_per_gpu=B, gt_size=S, geometric_augs=True, use_shuffle=True, dataset_enlarge_ratio=ratio,
                condition={"type": "mean", "scale_down": 16}, model_type="ImageEnhancer", phase="train")
    new = build_dataloader(store, dict(dopt, type="Dataset_PairedImage_Mask"), seed=100, device=dev, train=True)
    old = build_dataloader(shim, dict(dopt, type="TensorPairs"), seed=100, device=dev, train=True)
    lines = [f"data_rate: {torch.cuda.get_device_name(0)}, {a.pairs} pairs of {H}x{W}, batch {B}, gt_size {S}, geometric_augs on; store 2 x "
             f"{store.lq.nbytes / 2 ** 20:.0f} MiB uint8, shim 2 x {shim.lq.numel() * 4 / 2 ** 20:.0f} MiB float32; HIP events around "
             f"{a.batches} batches, loaders alternating after one warm-up pass each"]
    batches_ms(new, 0, 20), batches_ms(old, 0, 20)
    t_new, t_old = [], []
    for r in range(3):
        t_new.append(batches_ms(new, r + 1, a.batches))
        t_old.append(batches_ms(old, r + 1, a.batches))
    lines.append(f"ms per batch, folder loader (one batch_assemble launch): {', '.join(f'{t:.4f}' for t in t_new)}   median {sorted(t_new)[1]:.4f}")
    lines.append(f"ms per batch, tensor shim (index, crop, flip, 2 x resize_down): {', '.join(f'{t:.4f}' for t in t_old)}   median {sorted(t_old)[1]:.4f}")
    lines.append(f"spread between repeats: folder loader {max(t_new) - min(t_new):.4f} ms, shim {max(t_old) - min(t_old):.4f} ms; "
                 f"folder loader / shim = {sorted(t_new)[1] / sorted(t_old)[1]:.3f}")

    for yml, tag in (("CG_UNet_LOLv1.yml", "Stage I"), ("DecompDualBranch2DDWavelet_4.yml", "Stage II")):
        with open(os.path.join(PKG, "Options", yml)) as f:
            opt = yaml.safe_load(f)
        opt.update(is_train=True, dist=False, rank=0, world_size=1)
        opt["path"] = dict(pretrain_network_g=None, strict_load_g=True, resume_state=None)
        torch.manual_seed(100)
        m_new = build_model(copy.deepcopy(opt))
        torch.manual_seed(100)
        m_old = build_model(copy.deepcopy(opt))
        s_new, s_old, it0 = [], [], 0
        for r in range(5):
            s_new.append(steps_ms(m_new, new, 10 + r, a.steps, it0))
            s_old.append(steps_ms(m_old, old, 10 + r, a.steps, it0))
            it0 += a.steps + WARM
        mn, mo = sorted(s_new)[2], sorted(s_old)[2]
        lines.append(f"{tag} training step ({yml}, batch {B}, {S}x{S}) incl. its batch: folder loader {mn:.3f} ms ({B / mn * 1e3:.0f} img/s), "
                     f"shim {mo:.3f} ms ({B / mo * 1e3:.0f} img/s), medians of 5 rounds of {a.steps} steps after {WARM}   (rounds: {', '.join(f'{x:.3f}/{y:.3f}' for x, y in zip(s_new, s_old))})")
        del m_new, m_old
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
