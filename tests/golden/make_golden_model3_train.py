#!/usr/bin/env python3
"""Golden vectors of QD model3 in train() mode, generated like make_golden_r2.py by running the REFERENCE ITSELF on CPU (build container):

  g19_model3_train.npz   basicsr/QD/model3.py:98,124-131: nn.Dropout(0.1) on the two softmaxed channel-attention maps is live whenever the
                         module is in train() mode.  torch.nn.functional.dropout is replaced for the run by a function that draws the 0 / 1
                         keep mask from a seeded generator, records it and returns x * mask / (1 - p), so the masks can be injected on the
                         device.
                         (a) a (2,3,32,40) image through create_my_decomp('model3') (Q1_w / Q2_w) and model3.Decomp (Q1 / Q2) with the
                             shipped weights in train() mode, and the two masks of each call as one (B,2,32,32) array;
                         (b) two training steps of DecompDualBranch(decomp_model='model3') at the geometry of g12 (n_feat 16, one block per
                             level, parameters moved off their initial values the same way), L1 only, AdamW 2e-4 / 1e-4 with clip 1 as in
                             g10_train: the masks in call order, both losses, both gradient norms, every gradient of step 1, the parameters
                             before step 1 and after step 2.
  g19_model3_train_p<k>.npz   the three parameter-sized dicts of (b) (sd, grads, params: 352 332 floats each), cut into files below the size
                         limit of a committed file; tests merge them back by key.
Data only (inputs, expected outputs); no reference code is copied."""
import glob
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402
from make_golden import save, synth  # noqa: E402

PART_BYTES = 900 * 1024


class RecordedDropout:
    """Stands in for torch.nn.functional.dropout while the reference runs."""

    def __init__(self, seed):
        self.gen, self.masks = torch.Generator().manual_seed(seed), []

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return x
        m = (torch.rand(x.shape, generator=self.gen) >= p).to(x.dtype)
        self.masks.append(m)
        return x * m / (1 - p)

    def __enter__(self):
        self.orig, torch.nn.functional.dropout = torch.nn.functional.dropout, self
        return self

    def __exit__(self, *a):
        torch.nn.functional.dropout = self.orig

    def per_call(self):
        """[(B,1,32,32) attn_1 mask, attn_2 mask, ...] -> one (B,2,32,32) tensor per decomposition call."""
        assert len(self.masks) % 2 == 0 and all(m.shape[1:] == (1, 32, 32) for m in self.masks)
        return [torch.cat(self.masks[i:i + 2], 1) for i in range(0, len(self.masks), 2)]


def save_parts(name, dicts):
    """{'sd': {...}, ...} -> <name>_p<k>.npz with 'sd/<key>' entries, each file at most PART_BYTES of array data."""
    for old in glob.glob(os.path.join(HERE, name + "_p*.npz")):
        os.remove(old)
    flat = [(f"{d}/{k}", v.detach().cpu().numpy()) for d, kv in dicts.items() for k, v in kv.items()]
    parts, cur, size = [], {}, 0
    for k, v in flat:
        if cur and size + v.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    parts.append(cur)
    for i, part in enumerate(parts):
        path = os.path.join(HERE, f"{name}_p{i}.npz")
        np.savez(path, **part)
        print(f"  {os.path.basename(path)}  {os.path.getsize(path) / 1024:.1f} KiB")
        assert os.path.getsize(path) < 1 << 20


def main():
    ns = rh.load()
    import importlib
    torch.set_num_threads(8)
    m3 = importlib.import_module("basicsr.QD.model3")
    img, _ = synth((2, 3, 32, 40), 19)
    arrs = dict(img=img)
    with rh.ref_ctor_env():
        my = ns.ddw.create_my_decomp("model3")
        d = m3.Decomp(use_wavelets=True)
        d.load_state_dict(torch.load("basicsr/QD/checkpoints/model3_999.pth")["model_state_dict"])
    my.train(); d.train()
    with RecordedDropout(190) as rec, torch.no_grad():
        a, b = my(img)
        c, e = d(img)
    mw, mf = rec.per_call()
    arrs.update(q1w=a, q2w=b, q1=c, q2=e, mask_w=mw, mask_full=mf)
    my.eval(); d.eval()
    with torch.no_grad():
        # the dropout was live; with the shipped weights it moves the maps by ~5e-4 of their largest entry
        arrs.update(q1w_eval=my(img)[0], q1_eval=d(img)[0])
        assert float((arrs["q1w_eval"] - a).abs().max()) > 5e-4 and float((arrs["q1_eval"] - c).abs().max()) > 1e-4

    # ---- two training steps of DecompDualBranch + model3, reference modules + torch optimizer ----
    kw = dict(in_channels=6, out_channels=3, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=True,
              drop_path=0.0, sam=False, stage=1, decomp_model="model3")
    torch.manual_seed(100)
    with rh.ref_ctor_env():
        net = ns.dualse.DecompDualBranch(n_feat=16, num_blocks=[1, 1, 1], **kw)
    gg = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.startswith("decomp."):
                continue
            if "norm" in n or n.endswith("bias") or n.endswith(".gate"):
                p.add_(0.05 * torch.randn(p.shape, generator=gg))
            elif "_se" in n or "spatial_attention" in n:
                p.add_(1.0 * torch.randn(p.shape, generator=gg))
    net.train()
    assert net.decomp.training and not any(p.requires_grad for p in net.decomp.parameters())
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items() if not k.startswith("decomp.")}
    lq, gt = synth((2, 3, 32, 32), 191)
    gen = torch.Generator().manual_seed(33)
    gt_down = torch.nn.functional.interpolate(gt, scale_factor=1 / 16, mode="bilinear") + 0.1 * torch.randn(2, 3, 2, 2, generator=gen)
    params = [p for p in net.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=2e-4, weight_decay=1e-4, betas=(0.9, 0.999))
    losses, norms, grads = [], [], None
    with RecordedDropout(192) as rec:
        for it in range(2):
            opt.zero_grad()
            up = torch.nn.functional.interpolate(gt_down, scale_factor=16, mode="bilinear", align_corners=False)
            _, preds = net(torch.cat([lq, up], 1), mask=None)
            loss = torch.nn.functional.l1_loss(preds, gt)
            loss.backward()
            if it == 0:
                grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.requires_grad}
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, 1.0)))
            opt.step()
            losses.append(float(loss.detach()))
    masks = rec.per_call()
    assert len(masks) == 2                                   # one decomposition call per forward (the condition is not decomposed, :294-301)
    save("g19_model3_train", lq=lq, gt=gt, gt_down=gt_down, loss=np.array(losses), grad_norm=np.array(norms), step_masks=torch.stack(masks), **arrs)
    save_parts("g19_model3_train", dict(sd=sd0, grads=grads, params={k: p.detach() for k, p in net.named_parameters() if p.requires_grad}))
    print("done")


if __name__ == "__main__":
    main()
