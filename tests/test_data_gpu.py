"""GPU: training batches from image folders.  bem_batch_assemble_u8 (one launch per batch: symmetric pad, crop, the 8 geometric modes,
/ 255, label noise, the condition planes) against the numpy oracle of tests/data_ref.py on the smallest store at which it can go wrong;
its argument checks; basicsr/train.py on folders of PNGs for Stage II, Stage I (launched and captured step) and a resumed run; the
tensor shim's validation branch after its pad-and-condition lines moved into a helper."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import data_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


# 37x53x3 bytes is odd (the next image starts at an odd offset); 20x70 is shorter than the 32 crop
SHAPES = [(37, 53), (64, 64), (20, 70)]


@pytest.fixture(scope="module")
def store(dev):
    rng = np.random.RandomState(1810)
    lq = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    gt = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    offs = np.cumsum([0] + [h * w * 3 for h, w in SHAPES])
    table = torch.tensor([[int(offs[i]), h, w] for i, (h, w) in enumerate(SHAPES)], dtype=torch.int64)
    arena = lambda imgs: torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    return dict(lq=lq, gt=gt, table=table, table_dev=table.to(dev), lq_dev=arena(lq), gt_dev=arena(gt))


def _run(store, rows, Sh, Sw, s, noise=None, steps=0, dev=None):
    from bem import ops
    plan = torch.tensor(rows, dtype=torch.int32)
    nz = None if noise is None else torch.tensor(noise, dtype=torch.float32).to(store["lq_dev"].device)
    out = ops.batch_assemble(store["lq_dev"], store["gt_dev"], store["table"], store["table_dev"], plan, plan.to(store["lq_dev"].device), 0, len(rows),
                             Sh, Sw, s, noise_dev=nz, noise_steps=steps)
    torch.cuda.synchronize()
    return out


def _oracle(store, rows, Sh, Sw, noise=None, steps=0):
    lq = np.stack([R.assemble_ref(store["lq"][i], t, l, m, Sh, Sw) for i, t, l, m in rows])
    gt = np.stack([R.assemble_ref(store["gt"][i], t, l, m, Sh, Sw) for i, t, l, m in rows])
    if steps:
        gt = np.stack([R.label_noise_ref(g, *f, steps=steps) for g, f in zip(gt, noise)])
    return lq, gt


# all 8 modes on the 37x53 image at its four extreme corners; the 20x70 image at top = 0 with the symmetric padding in play (plain and
# rotated); the 64x64 image; row 11 carries the label noise
ROWS32 = [(0, (0, 5)[(m >> 1) & 1], (0, 21)[m & 1], m) for m in range(8)] + [(2, 0, 38, 0), (2, 0, 0, 3), (1, 32, 32, 5), (1, 17, 9, 6)]
ROWS16 = [(0, 21, 37, 0), (0, 0, 0, 1), (2, 4, 54, 2), (2, 0, 1, 3), (1, 48, 48, 4), (1, 0, 47, 5), (0, 20, 0, 6), (2, 3, 27, 7)]


@pytest.mark.parametrize("S,s,rows", [(32, 16, ROWS32), (16, 16, ROWS16)], ids=["S32_s16", "S16_s16"])
def test_batch_assemble_is_bit_equal_to_the_oracle(dev, store, S, s, rows):
    from bem import ops
    lq, gt, lqd, gtd = _run(store, rows, S, S, s)
    rl, rg = _oracle(store, rows, S, S)
    dl, dg = np.abs(lq.cpu().numpy() - rl).max(), np.abs(gt.cpu().numpy() - rg).max()
    dd = max(float((lqd - ops.resize_down(lq, s)).abs().max()), float((gtd - ops.resize_down(gt, s)).abs().max()))
    do = max(np.abs(lqd.cpu().numpy() - R.resize_down_ref(rl, s)).max(), np.abs(gtd.cpu().numpy() - R.resize_down_ref(rg, s)).max())
    print(f"PARITY batch_assemble S={S} s={s} rows={len(rows)}: max|lq - oracle| = {dl:.1e}, max|gt - oracle| = {dg:.1e}, "
          f"max|down - resize_down(own output)| = {dd:.1e}, max|down - oracle| = {do:.1e} (all must be 0)")
    assert lq.shape == gt.shape == (len(rows), 3, S, S) and lqd.shape == gtd.shape == (len(rows), 3, S // s, S // s)
    assert (lq.cpu().numpy() == rl).all() and (gt.cpu().numpy() == rg).all()
    assert torch.equal(lqd, ops.resize_down(lq, s)) and torch.equal(gtd, ops.resize_down(gt, s))
    assert (lqd.cpu().numpy() == R.resize_down_ref(rl, s)).all() and (gtd.cpu().numpy() == R.resize_down_ref(rg, s)).all()


def test_batch_assemble_label_noise_within_one_ulp(dev, store):
    from bem import ops
    noise = [(1.0, 1.0, 1.0)] * 11 + [(1.02, 1.2, 0.9)]
    lq, gt, lqd, gtd = _run(store, ROWS32, 32, 32, 16, noise=noise, steps=7)
    rl, rg = _oracle(store, ROWS32, 32, 32, noise=noise, steps=7)
    plain = _oracle(store, ROWS32, 32, 32)[1]
    ulp = R.ulp_diff(gt.cpu().numpy(), rg)
    ulp11 = R.ulp_diff(gt[11].cpu().numpy(), rg[11])
    moved = float(np.abs(rg[11] - plain[11]).max())
    top = R.contrast_ref(np.float32([1.0]), 0.9)[0]                            # where an element clipped to 1 by the brightness step ends
    print(f"PARITY batch_assemble label noise (1.02, 1.2, 0.9): gt row 11 vs oracle {ulp11} ulp, all rows {ulp} ulp (bound 1); "
          f"the noise moves the row by up to {moved:.3f}; clipped by the brightness step: {int((rg[11] == top).sum())} elements")
    assert moved > 0.1 and (rg[11] == top).any()
    assert ulp <= 1
    assert (lq.cpu().numpy() == rl).all()                                      # lq carries no label noise
    assert torch.equal(gtd, ops.resize_down(gt, 16)) and torch.equal(lqd, ops.resize_down(lq, 16))     # gt_down is taken after the noise
    # single steps: the reference's switches (labelnoise.py:59-66)
    for steps in (1, 2, 4):
        g1 = _run(store, ROWS32[8:], 32, 32, 16, noise=noise[8:], steps=steps)[1]
        assert R.ulp_diff(g1.cpu().numpy(), _oracle(store, ROWS32[8:], 32, 32, noise=noise[8:], steps=steps)[1]) <= 1, steps


def test_batch_assemble_rectangular_crops(dev, store):
    """Modes 0, 1, 4, 5 on a 20x64 crop, and the validation form: the whole 37x53 image, mode 0, no condition planes."""
    from bem import ops
    rows = [(2, 0, 6, 0), (2, 0, 0, 1), (1, 44, 0, 4), (0, 17, 0, 5)]
    lq, gt, lqd, gtd = _run(store, rows, 20, 64, 4)
    rl, rg = _oracle(store, rows, 20, 64)
    assert (lq.cpu().numpy() == rl).all() and (gt.cpu().numpy() == rg).all()
    assert torch.equal(lqd, ops.resize_down(lq, 4)) and torch.equal(gtd, ops.resize_down(gt, 4)) and lqd.shape == (4, 3, 5, 16)
    lq, gt, lqd, gtd = _run(store, [(0, 0, 0, 0)], 37, 53, 0)
    assert lqd is None and gtd is None
    assert (lq[0].cpu().numpy() == (store["lq"][0].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)).all()
    assert (gt[0].cpu().numpy() == (store["gt"][0].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)).all()


def test_batch_assemble_refuses_bad_arguments(dev, store):
    """Each refusal comes from the host-side checks of the ABI entry (rc 1 = BEM_ERR_INVALID, before any launch)."""
    from bem.native import BemNativeError
    with pytest.raises(BemNativeError, match=r"rc=1.*rotates"):
        _run(store, [(1, 0, 0, 2)], 16, 32, 16)
    with pytest.raises(BemNativeError, match=r"rc=1.*scale_down 12"):
        _run(store, [(1, 0, 0, 0)], 32, 32, 12)
    with pytest.raises(BemNativeError, match=r"rc=1.*names image 3 of 3"):
        _run(store, [(1, 0, 0, 0), (3, 0, 0, 0)], 32, 32, 16)
    with pytest.raises(BemNativeError, match=r"rc=1.*crops at"):
        _run(store, [(0, 6, 0, 0)], 32, 32, 16)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the driver
def _png_folders(root, n, h=48, w=80, seed=7):
    rng = np.random.RandomState(seed)
    for d in ("train_gt", "train_lq", "val_gt", "val_lq"):
        (root / d).mkdir(parents=True)
    for i in range(n):
        base = rng.randint(0, 256, (h // 8, w // 8, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)
        gt = np.clip(base.astype(np.int32) + rng.randint(-6, 7, base.shape), 0, 255).astype(np.uint8)
        lq = (gt * 0.3).astype(np.uint8)
        for d, k in (("train", n), ("val", 2)):
            if i < k:
                Image.fromarray(gt).save(root / f"{d}_gt" / f"{i:02d}.png")
                Image.fromarray(lq).save(root / f"{d}_lq" / f"{i:02d}.png")
    return [f"datasets:train:dataroot_gt={root / 'train_gt'}", f"datasets:train:dataroot_lq={root / 'train_lq'}",
            f"datasets:val:dataroot_gt={root / 'val_gt'}", f"datasets:val:dataroot_lq={root / 'val_lq'}"]


def _drive(root, yml, roots, total, resume=False, save=100):
    from basicsr.train import train_pipeline
    argv = ["--opt", yml, "--force_yml", "network_g:n_feat=16", "network_g:num_blocks=[1,1,1]", f"train:total_iter={total}",
            f"logger:save_checkpoint_freq={save}", "logger:print_freq=1", "datasets:train:batch_size_per_gpu=2", "datasets:train:gt_size=64",
            "train:scheduler:periods=[4,4,4]"] + roots
    if resume:
        argv.append("--auto_resume")
    torch.manual_seed(100)
    return train_pipeline(str(root), argv=argv)


def test_training_driver_stage2_on_folders(dev, tmp_path, capsys):
    """basicsr/train.py --opt Options/DecompDualBranch2DDWavelet_4.yml with neither --synthetic nor --pairs: raised NotImplementedError in
    build_dataset before the folder dataset existed."""
    roots = _png_folders(tmp_path / "data", 6)
    model, info = _drive(tmp_path / "run", os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml"), roots, 2)
    out = capsys.readouterr().out
    assert info["iter"] == 2 and math.isfinite(float(model.log_dict["l_pix"]))
    assert "6 pairs decoded" in out and "2 pairs decoded" in out and "Require iter number per epoch: 3" in out
    assert out.count("Validation") >= 1 and math.isfinite(model.metric_results["psnr"])
    assert tuple(model.lq.shape) == (1, 3, 64, 128)                    # the last thing fed was a padded 48x80 validation image


def _stage1_yml(tmp_path):
    txt = open(os.path.join(PKG, "Options", "CG_UNet_LOLv1.yml")).read()
    key = "    geometric_augs: true\n"
    assert txt.count(key) == 1
    path = tmp_path / "CG_UNet_LOLv1.yml"
    path.write_text(txt.replace(key, key + "    mim:\n      mask_ratio: 0.75\n      mask_patch_size: 1\n      model_patch_size: 1\n"))
    return str(path)


def test_training_driver_stage1_on_folders_captured_equals_launched(dev, tmp_path, monkeypatch):
    """Stage I from folders with a ``mim:`` block: the batch carries a mask of exactly ceil(0.75 * 16) ones per sample, and the step replayed
    from a HIP graph ends where the step launched kernel by kernel ends (the equality test_stage1_captured_step_equals_the_launched_one
    asserts for the tensor shim)."""
    from basicsr.data import build_dataloader, build_dataset
    roots = _png_folders(tmp_path / "data", 6)
    yml = _stage1_yml(tmp_path)
    monkeypatch.setenv("BEM_STAGE1_GRAPH", "0")
    a, ia = _drive(tmp_path / "A", yml, roots, 8)
    assert not getattr(a, "_graphs", None)
    monkeypatch.setenv("BEM_STAGE1_GRAPH", "1")
    b, ib = _drive(tmp_path / "B", yml, roots, 8)
    assert ia["iter"] == ib["iter"] == 8 and math.isfinite(float(b.log_dict["l_pix"]))
    assert [g for g in b._graphs.values() if isinstance(g, dict)]
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    print(f"PARITY stage-I folder loader, captured vs launched step after 8 iterations: max parameter difference {worst:.2e} (bound 4e-5)")
    assert worst <= 4e-5, worst
    # the batches the driver was fed
    opt = dict(b.opt["datasets"]["train"])
    loader = build_dataloader(build_dataset(opt), opt, seed=b.opt["manual_seed"], device=dev, train=True)
    assert len(loader) == 3
    batches = list(loader)
    assert len(batches) == 3
    for d in batches:
        assert set(d) == {"lq", "gt", "lq_down", "gt_down", "mask", "lq_path"} and len(d["lq_path"]) == 2
        assert d["mask"].shape == (2, 4, 4) and d["mask"].dtype == torch.float32 and d["lq_down"].shape == (2, 3, 4, 4)
        assert d["mask"].sum((1, 2)).tolist() == [12.0, 12.0] == [float(math.ceil(0.75 * 16))] * 2
    # CG_UNet_LOLv1.yml as shipped has no mim: block -> no mask, and the driver does not inject one
    opt.pop("mim")
    assert "mask_ratio" not in opt
    assert all("mask" not in d for d in build_dataloader(build_dataset(opt), opt, seed=1, device=dev, train=True))


def test_training_driver_resume_on_folders(dev, tmp_path):
    """5 pairs, batch 2: an epoch yields 2 batches (the partial third is dropped).  A run broken after 3 iterations -- one batch into epoch
    1 -- and resumed with --auto_resume ends where the uninterrupted run ends."""
    roots = _png_folders(tmp_path / "data", 5)
    yml = os.path.join(PKG, "Options", "TwoBranch_3.yml")
    a, ia = _drive(tmp_path / "A", yml, roots, 6, save=3)
    _drive(tmp_path / "B", yml, roots, 3, save=3)
    assert (tmp_path / "B" / "experiments" / "FusedTwoBranch_3" / "training_states" / "3.state").is_file()
    b, ib = _drive(tmp_path / "B", yml, roots, 6, resume=True, save=3)
    assert ia["iter"] == ib["iter"] == 6
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    print(f"PARITY folder loader, resumed vs uninterrupted run after 6 iterations: max parameter difference {worst:.2e} (bound 4e-5)")
    assert worst <= 4e-5, worst


# ------------------------------------------------------------------------------------------------------------- the tensor shim
def test_shim_validation_branch_is_unchanged(dev):
    """The shim's validation batches against the lines they were made by before those moved into pad_and_condition: reflect pad to a
    multiple of 4 * scale_down, then the condition planes."""
    from basicsr.data import build_dataloader, build_dataset
    from bem import ops
    opt = dict(type="Synthetic", num_images=2, image_size=60, seed=5, condition={"type": "mean", "scale_down": 4}, phase="val")
    ds = build_dataset(opt)
    batches = list(build_dataloader(ds, opt, seed=3, device=dev, train=False))
    assert len(batches) == 2
    for i, d in enumerate(batches):
        lq, gt = ds.lq[i:i + 1].to(dev).contiguous(), ds.gt[i:i + 1].to(dev).contiguous()
        lqp, gtp = ops.pad_reflect(lq, 64, 64), ops.pad_reflect(gt, 64, 64)
        want = dict(lq=lqp, gt=gtp, lq_down=ops.resize_down(lqp, 4), gt_down=ops.resize_down(gtp, 4))
        assert all(torch.equal(d[k], want[k]) for k in want)
        assert d["crop_hw"] == (60, 60) and d["lq_path"] == [f"tensor_{i:05d}"] and set(d) == set(want) | {"crop_hw", "lq_path"}
    # a size that needs no pad passes through
    opt = dict(opt, image_size=32)
    ds = build_dataset(opt)
    d = next(iter(build_dataloader(ds, opt, seed=3, device=dev, train=False)))
    assert torch.equal(d["lq"], ds.lq[:1].to(dev)) and torch.equal(d["lq_down"], ops.resize_down(ds.lq[:1].to(dev).contiguous(), 4)) and d["crop_hw"] == (32, 32)
