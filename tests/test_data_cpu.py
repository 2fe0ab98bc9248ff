"""CPU: the folder dataset (basicsr.data.paired_image_dataset) without a GPU -- pairing and its errors, the numpy oracle of the batch
kernel (tests/data_ref.py) against what the reference's own functions returned (tests/golden/g18_data.npz), and the epoch plan:
determinism, sharding, per-sample draws, switches, length."""
import math

import numpy as np
import pytest
import torch
from PIL import Image

import data_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def g18():
    return load_golden("g18_data")


def _write(folder, name, h, w, seed):
    folder.mkdir(exist_ok=True)
    a = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    Image.fromarray(a).save(folder / name)
    return a


def _folders(tmp_path, sizes, tmpl="{}", ext=".png"):
    lq, gt = {}, {}
    for i, (h, w) in enumerate(sizes):
        gt[i] = _write(tmp_path / "gt", f"{i:03d}.png", h, w, 100 + i)
        lq[i] = _write(tmp_path / "lq", tmpl.format(f"{i:03d}") + ext, h, w, 200 + i)
    return lq, gt


def _opt(tmp_path, **kw):
    o = dict(type="Dataset_PairedImage_Mask", name="T", phase="train", dataroot_gt=str(tmp_path / "gt"), dataroot_lq=str(tmp_path / "lq"),
             io_backend={"type": "disk"}, condition={"type": "mean", "scale_down": 16}, model_type="ImageEnhancer", gt_size=32,
             batch_size_per_gpu=2, geometric_augs=True)
    o.update(kw)
    return o


# ---------------------------------------------------------------------------------------------------------------- pairing
def test_build_dataset_returns_the_folder_dataset(tmp_path):
    """Raised NotImplementedError ("file-backed datasets are host I/O outside the HIP path") before the folder dataset existed."""
    from basicsr.data import build_dataset
    lq, gt = _folders(tmp_path, [(37, 53), (64, 64), (20, 70)])
    ds = build_dataset(_opt(tmp_path))
    assert len(ds) == 3 and ds.table.tolist() == [[0, 37, 53], [37 * 53 * 3, 64, 64], [37 * 53 * 3 + 64 * 64 * 3, 20, 70]]
    assert ds.lq.dtype == np.uint8 and ds.lq.shape == ds.gt.shape == (37 * 53 * 3 + 64 * 64 * 3 + 20 * 70 * 3,)
    for i in range(3):
        off, H, W = ds.table[i]
        assert (ds.lq[off:off + H * W * 3].reshape(H, W, 3) == lq[i]).all() and (ds.gt[off:off + H * W * 3].reshape(H, W, 3) == gt[i]).all()
    assert [p["gt_path"].endswith(f"{i:03d}.png") for i, p in enumerate(ds.paths)] == [True] * 3


def test_filename_tmpl_and_lq_extension(tmp_path):
    from basicsr.data import build_dataset
    lq, gt = _folders(tmp_path, [(8, 9), (10, 8)], tmpl="{}_low", ext=".bmp")
    ds = build_dataset(_opt(tmp_path, filename_tmpl="{}_low"))
    assert [p["lq_path"].rsplit("/", 1)[1] for p in ds.paths] == ["000_low.bmp", "001_low.bmp"]
    assert (ds.lq[:8 * 9 * 3].reshape(8, 9, 3) == lq[0]).all()
    with pytest.raises(ValueError, match="000"):
        build_dataset(_opt(tmp_path))                       # without the template no partner of 000.png


def test_pairing_errors_name_the_file(tmp_path):
    from basicsr.data import build_dataset
    _folders(tmp_path, [(8, 9), (10, 8)])
    _write(tmp_path / "gt", "zzz.png", 8, 8, 1)
    with pytest.raises(ValueError, match="different number of images: 2 .* 3 "):
        build_dataset(_opt(tmp_path))
    _write(tmp_path / "lq", "yyy.png", 8, 8, 2)
    with pytest.raises(ValueError, match=r"zzz\.\*.*zzz\.png"):
        build_dataset(_opt(tmp_path))
    (tmp_path / "lq" / "yyy.png").unlink()
    _write(tmp_path / "lq", "zzz.png", 8, 9, 3)
    with pytest.raises(ValueError, match=r"lq/zzz\.png.*gt/zzz\.png.*different shapes: 8x9 and 8x8"):
        build_dataset(_opt(tmp_path))


def test_unsupported_options_raise_by_name(tmp_path):
    from basicsr.data import build_dataset
    _folders(tmp_path, [(8, 9)])
    for kw, word in ((dict(io_backend={"type": "lmdb"}), "lmdb"), (dict(meta_info_file="m.txt"), "meta_info_file"), (dict(mean=[0.5] * 3), "mean"),
                     (dict(std=[0.5] * 3), "std"), (dict(condition={"type": "histogram"}), "histogram")):
        with pytest.raises(NotImplementedError, match=word):
            build_dataset(_opt(tmp_path, **kw))
    with pytest.raises(ValueError, match=r"resident_limit_gb"):
        build_dataset(_opt(tmp_path, resident_limit_gb=1e-9))


# ------------------------------------------------------------------------------------------------- oracle against the fixture
def test_oracle_augmentation_modes_match_the_reference(g18):
    img = g18["aug_in"]
    seen = set()
    for mode in range(8):
        assert (R.augment_ref(img, mode) == g18[f"aug_{mode}"]).all(), mode
        x = R.assemble_ref(img, 0, 0, mode, 6)
        assert (x == (g18[f"aug_{mode}"].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)).all()
        seen.add(g18[f"aug_{mode}"].tobytes())
    assert len(seen) == 8


def test_oracle_symmetric_pad_repeats_the_edge():
    src = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    x = R.assemble_ref(src, 0, 0, 0, 5)                                   # rows 0 1 | 1 0 0, columns 0 1 2 | 2 1
    rows, cols = [0, 1, 1, 0, 0], [0, 1, 2, 2, 1]
    assert (x == (src[rows][:, cols].astype(np.float32) / np.float32(255)).transpose(2, 0, 1)).all()


def test_masks_exact_count_and_blocks(g18):
    from basicsr.data.paired_image_dataset import mim_geometry, mim_masks
    for tag, ones in (("a", 48), ("b", 28)):
        size, mp, pp, ratio = (float(v) for v in g18[f"mask_{tag}_args"])
        rand, scale = int(size // mp), int(mp // pp)
        count = int(np.ceil(rand * rand * ratio))
        for m in g18[f"mask_{tag}"]:                                       # the reference's masks have the structure the oracle checks
            assert int(m.sum()) == ones and R.mask_structure_ok(m, rand, scale, count)
        opt = dict(mim=dict(mask_patch_size=int(mp), model_patch_size=int(pp), mask_ratio=ratio), gt_size=int(size), model_type="ImageEnhancer")
        assert mim_geometry(opt) == (rand, scale, count)
        ours = mim_masks(50, rand, scale, count, torch.Generator().manual_seed(3))
        assert ours.shape == (50, 8, 8) and ours.dtype == torch.float32
        assert all(int(m.sum()) == ones and R.mask_structure_ok(m.numpy(), rand, scale, count) for m in ours)
        assert len({m.numpy().tobytes() for m in ours}) > 40
    # ConditionGenerator: input_size = gt_size / scale_down (paired_image_dataset.py:278)
    opt = dict(mim=dict(mask_patch_size=1, model_patch_size=1, mask_ratio=0.75), gt_size=64, model_type="ConditionGenerator", condition={"scale_down": 16})
    assert mim_geometry(opt) == (4, 1, 12)


def test_sampler_lists_match_the_reference(g18):
    from basicsr.data.paired_image_dataset import sampler_indices
    for epoch in (0, 1):
        for rank in range(3):
            want = g18[f"sampler_e{epoch}_r{rank}"].tolist()
            assert R.sampler_ref(10, 3, rank, 1, epoch) == want
            assert sampler_indices(10, 3, rank, 1, epoch).tolist() == want


def test_oracle_label_noise_matches_the_reference(g18):
    bgr = g18["noise_in_bgr"].numpy()
    rgb = bgr[..., ::-1]
    t, b, c = (float(v) for v in g18["noise_factors"])
    tem = R.temperature_ref(rgb, t)
    assert tem.dtype == np.float32 and (tem == g18["noise_temperature_f64"].numpy().astype(np.float32)[..., ::-1]).all()
    assert (R.brightness_ref(rgb, b) == g18["noise_brightness"].numpy()[..., ::-1]).all()
    assert (R.contrast_ref(rgb, c) == g18["noise_contrast"].numpy()[..., ::-1]).all()
    chain = R.label_noise_ref(np.ascontiguousarray(rgb.transpose(2, 0, 1)), t, b, c)
    assert (chain == g18["noise_chain"].numpy()[..., ::-1].transpose(2, 0, 1)).all()
    assert R.brightness_ref(rgb, b).max() == 1.0 and (rgb * np.float32(b)).max() > 1.0      # the clip was hit


def test_oracle_resize_down_is_the_centre_tap_mean():
    x = np.random.RandomState(0).rand(3, 32, 32).astype(np.float32)
    d = R.resize_down_ref(x, 16)
    assert d.shape == (3, 2, 2) and d.dtype == np.float32
    assert d[1, 1, 0] == np.float32(0.25) * (((x[1, 23, 7] + x[1, 24, 7]) + x[1, 23, 8]) + x[1, 24, 8])


# ------------------------------------------------------------------------------------------------------------------ plan
SIZES = np.array([[37, 53], [64, 64], [20, 70], [400, 600], [32, 32], [16, 16], [90, 33]])


def _plan(seed=100, epoch=0, rank=0, world=1, **kw):
    from basicsr.data.paired_image_dataset import epoch_plan
    o = dict(gt_size=32, batch_size_per_gpu=2, geometric_augs=True, dataset_enlarge_ratio=1, condition={"scale_down": 16}, model_type="ImageEnhancer")
    o.update(kw)
    return epoch_plan(SIZES, o, seed, epoch, rank, world)


def _same(a, b):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and torch.equal(a[k], b[k])) for k in ("rows", "noise", "mask"))


def test_plan_is_a_function_of_seed_epoch_rank():
    kw = dict(labelnoise=dict(tem_var=0.03), mim=dict(mask_patch_size=4, model_patch_size=1, mask_ratio=0.6), dataset_enlarge_ratio=8)
    a = _plan(100, 3, 1, 2, **kw)
    assert _same(a, _plan(100, 3, 1, 2, **kw))
    for other in (_plan(100, 4, 1, 2, **kw), _plan(100, 3, 0, 2, **kw), _plan(101, 3, 1, 2, **kw)):
        assert not torch.equal(a["rows"], other["rows"]) and not torch.equal(a["noise"], other["noise"]) and not torch.equal(a["mask"], other["mask"])
    # a different manual_seed keeps the sample order (the sampler is keyed by the epoch alone) and changes the draws
    assert torch.equal(a["rows"][:, 0], _plan(101, 3, 1, 2, **kw)["rows"][:, 0])


def test_plan_shards_partition_one_permutation():
    from basicsr.data.paired_image_dataset import sampler_indices
    n, world, ratio = len(SIZES), 3, 5
    shards = [sampler_indices(n, world, r, ratio, 2).tolist() for r in range(world)]
    num = math.ceil(n * ratio / world)
    g = torch.Generator()
    g.manual_seed(2)
    perm = torch.randperm(num * world, generator=g).tolist()
    merged = [None] * (num * world)
    for r in range(world):
        assert len(shards[r]) == num
        merged[r::world] = shards[r]
    assert merged == [v % n for v in perm]                                 # interleaved, the shards are the one permutation
    assert sorted(perm) == list(range(num * world))
    for r in range(world):                                                 # and each plan takes its shard's whole batches in order
        p = _plan(100, 2, r, world, dataset_enlarge_ratio=ratio, batch_size_per_gpu=4)
        assert p["rows"][:, 0].tolist() == shards[r][:(num // 4) * 4] and p["batches"] == num // 4


def test_plan_per_sample_draws():
    p = _plan(100, 0, dataset_enlarge_ratio=40)
    rows = p["rows"].numpy()
    assert rows.dtype == np.int32 and len(rows) >= 200
    H, W = SIZES[rows[:, 0], 0], SIZES[rows[:, 0], 1]
    assert (rows[:, 1] >= 0).all() and (rows[:, 1] <= np.maximum(H, 32) - 32).all()
    assert (rows[:, 2] >= 0).all() and (rows[:, 2] <= np.maximum(W, 32) - 32).all()
    small = (H < 32) | (W < 32)
    assert small.any() and (rows[H <= 32, 1] == 0).all() and (rows[W <= 32, 2] == 0).all()
    big = rows[rows[:, 0] == 3]
    assert len(set(big[:, 1])) > 5 and len(set(big[:, 2])) > 5 and big[:, 1].max() > 184 and big[:, 2].max() > 284     # the range is used
    assert set(rows[:200, 3]) == set(range(8))
    pairs = rows.reshape(-1, 2, 4)
    assert (np.abs(pairs[:, 0, 1:] - pairs[:, 1, 1:]).sum(1) > 0).mean() > 0.9      # two samples of one batch: own offset / mode
    assert (_plan(100, 0, geometric_augs=False)["rows"][:, 3] == 0).all()


def test_plan_switches():
    p = _plan()
    assert p["mask"] is None and p["noise"] is None and p["noise_steps"] == 0
    p = _plan(labelnoise=dict(tem_var=0.03), dataset_enlarge_ratio=200)
    assert p["mask"] is None and p["noise_steps"] == 7 and p["noise"].shape == (len(p["rows"]), 3) and p["noise"].dtype == torch.float32
    m, s = p["noise"].double().mean(0), p["noise"].double().std(0)
    assert torch.allclose(m, torch.tensor([1.0, 1.15, 1.15], dtype=torch.float64), atol=0.03) and torch.allclose(s, torch.tensor([0.03, 0.15, 0.15], dtype=torch.float64), rtol=0.15)
    assert _plan(labelnoise=dict(tem_mean=1, tem_var=0))["noise_steps"] == 6
    p = _plan(mim=dict(mask_patch_size=4, model_patch_size=2, mask_ratio=0.6))
    assert p["noise"] is None and p["mask"].shape == (len(p["rows"]), 16, 16)
    assert all(R.mask_structure_ok(m.numpy(), 8, 2, 39) for m in p["mask"])


@pytest.mark.parametrize("n,batch,world,ratio", [(5, 2, 1, 1), (7, 2, 3, 1), (7, 4, 2, 3), (6, 2, 1, 1)])
def test_loader_length_is_the_batches_yielded(n, batch, world, ratio):
    from basicsr.data.paired_image_dataset import PairedImageBatchLoader, epoch_plan
    opt = dict(gt_size=32, batch_size_per_gpu=batch, dataset_enlarge_ratio=ratio, condition={"scale_down": 16})
    ld = PairedImageBatchLoader.__new__(PairedImageBatchLoader)
    ld.dataset, ld.opt, ld.batch, ld.world, ld.train = list(range(n)), opt, batch, world, True
    for rank in range(world):
        p = epoch_plan(SIZES[:n], opt, 1, 0, rank, world)
        assert len(ld) == p["batches"] == len(p["rows"]) // batch == math.ceil(n * ratio / world) // batch
    if (n, batch, world) == (5, 2, 1):
        assert len(ld) == 2                                                # math.ceil(5 / 2) = 3 is what the shim's len() says
