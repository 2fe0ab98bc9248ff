"""``Dataset_PairedImage_Mask`` from image folders (basicsr/data/paired_image_dataset.py:234-412 of the reference), device-resident.

The reference decodes, pads, crops, augments and resizes one sample per ``__getitem__`` call in worker processes.  Here the folders are
decoded once on the host into a ragged uint8 store -- one byte arena for lq, one for gt, a table ``(offset, H, W)`` per image; images
need not share a size and are not aligned in the arena (the kernel reads bytes) -- which is uploaded once.  What is random is drawn on
the host once per epoch into a plan (``epoch_plan``); a training step is then one ``bem.ops.batch_assemble`` launch over its rows of
the plan plus a view of the epoch's mask table: no host synchronisation and no host-to-device copy per step.

Draw order of an epoch plan (documented because a resumed run must redraw it): the sample order is the reference's ``EnlargedSampler``
(data/data_sampler.py:21-42): ``torch.Generator().manual_seed(epoch)``, ``randperm(total_size) % len``, ``[rank::world]`` -- one
permutation for all ranks, the shards partition it.  Everything else comes from one generator seeded by ``plan_seed(manual_seed, epoch,
rank)``, in this order over the R samples of the shard that fall into whole batches:
  1. ``rand(R)`` float64 -> top  = floor(u * (max(H,S) - S + 1));
  2. ``rand(R)`` float64 -> left = floor(u * (max(W,S) - S + 1));
  3. ``randint(0, 8, (R,))`` -> mode (only when ``geometric_augs``);
  4. ``randn(R, 3)`` float64 -> mean + var * z for (temperature, brightness, contrast) (only when ``labelnoise``);
  5. ``rand(R, tokens)`` float64, argsort per row -> the first ``ceil(mask_ratio * tokens)`` entries are masked (only when ``mim``)."""
import math
import os
import os.path as osp
import time

import numpy as np
import torch

__all__ = ["PairedImageMaskDataset", "PairedImageBatchLoader", "paired_paths_from_folder", "sampler_indices", "epoch_plan",
           "mim_masks", "plan_seed", "DATASET_TYPE"]

DATASET_TYPE = "Dataset_PairedImage_Mask"
_IMG_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".ppm", ".webp")


def _images(folder):
    if not osp.isdir(folder):
        raise ValueError(f"{folder} is not a folder")
    return sorted(f for f in os.listdir(folder) if f.lower().endswith(_IMG_EXT) and osp.isfile(osp.join(folder, f)))


def paired_paths_from_folder(lq_folder, gt_folder, filename_tmpl="{}"):
    """data_util.py:208-253: the gt folder's images sorted by name, each paired with ``filename_tmpl.format(basename)`` + the extension
    that name has in the lq folder."""
    gts, lqs = _images(gt_folder), _images(lq_folder)
    if len(gts) != len(lqs):
        raise ValueError(f"lq and gt datasets have different number of images: {len(lqs)} in {lq_folder}, {len(gts)} in {gt_folder}.")
    by_stem = {osp.splitext(f)[0]: f for f in lqs}
    paths = []
    for g in gts:
        stem = filename_tmpl.format(osp.splitext(g)[0])
        if stem not in by_stem:
            raise ValueError(f"{stem}.* (the lq partner of {osp.join(gt_folder, g)}) is not in {lq_folder}.")
        paths.append(dict(lq_path=osp.join(lq_folder, by_stem[stem]), gt_path=osp.join(gt_folder, g)))
    return paths


class PairedImageMaskDataset:
    """The decoded folders on the host: ``lq`` / ``gt`` uint8 arenas (numpy), ``table`` (n,3) int64 ``(offset, H, W)``, ``paths``."""

    def __init__(self, opt):
        from PIL import Image
        self.opt = opt
        if (opt.get("io_backend") or {}).get("type", "disk") == "lmdb":
            raise NotImplementedError("Dataset_PairedImage_Mask: io_backend.type lmdb is not used by the shipped option files")
        if opt.get("meta_info_file") is not None:
            raise NotImplementedError("Dataset_PairedImage_Mask: meta_info_file is not used by the shipped option files")
        if opt.get("mean") is not None or opt.get("std") is not None:
            raise NotImplementedError("Dataset_PairedImage_Mask: mean / std normalisation is not used by the shipped option files")
        cond = opt.get("condition") or {}
        if cond.get("type", "mean") == "histogram":
            raise NotImplementedError("Dataset_PairedImage_Mask: condition type 'histogram' is not used by the shipped option files")
        if cond.get("type", "mean") != "mean":
            raise ValueError(f"condition type {cond.get('type')} not supported")
        self.paths = paired_paths_from_folder(opt["dataroot_lq"], opt["dataroot_gt"], opt.get("filename_tmpl") or "{}")
        if not self.paths:
            raise ValueError(f"no images in {opt['dataroot_gt']}")
        t0 = time.time()
        # sizes first (PIL reads the header only): the store is summed before anything is allocated
        table = np.zeros((len(self.paths), 3), np.int64)
        total = 0
        for i, p in enumerate(self.paths):
            with Image.open(p["gt_path"]) as g, Image.open(p["lq_path"]) as q:
                if g.size != q.size:
                    raise ValueError(f"pair {p['lq_path']} / {p['gt_path']} has different shapes: {q.size[1]}x{q.size[0]} and {g.size[1]}x{g.size[0]}")
                table[i] = (total, g.size[1], g.size[0])
            total += int(table[i, 1] * table[i, 2] * 3)
        limit = float(opt.get("resident_limit_gb", 32))
        if 2 * total > limit * 2 ** 30:
            raise ValueError(f"Dataset_PairedImage_Mask: the decoded store is {2 * total / 2 ** 30:.2f} GiB, more than datasets.<phase>.resident_limit_gb = {limit:g}")
        self.lq, self.gt = np.empty(total, np.uint8), np.empty(total, np.uint8)
        for i, p in enumerate(self.paths):
            off, H, W = (int(v) for v in table[i])
            for key, arena in (("lq_path", self.lq), ("gt_path", self.gt)):
                with Image.open(p[key]) as im:
                    arena[off:off + H * W * 3] = np.asarray(im.convert("RGB"), np.uint8).reshape(-1)
        self.table = table
        print(f"Dataset_PairedImage_Mask {opt.get('name', '')}: {len(self.paths)} pairs decoded in {time.time() - t0:.2f} s, "
              f"store 2 x {total / 2 ** 20:.1f} MiB uint8", flush=True)

    def __len__(self):
        return len(self.paths)

    def sizes(self):
        return self.table[:, 1:3]


def sampler_indices(n, world, rank, ratio, epoch):
    """EnlargedSampler.__iter__ (data_sampler.py:29-42)."""
    num_samples = math.ceil(n * ratio / world)
    total_size = num_samples * world
    g = torch.Generator()
    g.manual_seed(int(epoch))
    idx = torch.randperm(total_size, generator=g) % n
    return idx[rank:total_size:world]


def plan_seed(seed, epoch, rank):
    """(manual_seed, epoch, rank) mixed into the 32 bits torch's CPU generator takes its state from (it drops the high half of a seed)."""
    m = (1 << 64) - 1
    x = (int(seed or 0) * 0x9E3779B97F4A7C15 + int(epoch) * 0xBF58476D1CE4E5B9 + int(rank) * 0x94D049BB133111EB + 0x2545F4914F6CDD1D) & m
    x = ((x ^ (x >> 31)) * 0xD6E8FEB86659FD93) & m
    return (x ^ (x >> 32)) & 0xFFFFFFFF


def mim_geometry(opt):
    """MaskGenerator.__init__ (utils/mask.py:4-17) with the input_size of paired_image_dataset.py:276-282: (rand_size, scale, count)."""
    mim = opt["mim"]
    s = int((opt.get("condition") or {}).get("scale_down", 1))
    size = int(opt["gt_size"]) if opt.get("model_type") == "ImageEnhancer" else int(int(opt["gt_size"]) / s)
    mp, pp = int(mim["mask_patch_size"]), int(mim["model_patch_size"])
    if size % mp or mp % pp:
        raise ValueError(f"mim: input_size {size} % mask_patch_size {mp} and mask_patch_size % model_patch_size {pp} must be 0")
    rand = size // mp
    return rand, mp // pp, int(np.ceil(rand * rand * float(mim["mask_ratio"])))


def mim_masks(R, rand, scale, count, g):
    """R masks of MaskGenerator.__call__ (utils/mask.py:19-27): exactly ``count`` of the rand x rand patches of a random permutation,
    each repeated ``scale`` times along both axes -> float (R, rand*scale, rand*scale)."""
    perm = torch.rand(R, rand * rand, generator=g, dtype=torch.float64).argsort(dim=1)
    m = torch.zeros(R, rand * rand)
    m.scatter_(1, perm[:, :count], 1.0)
    return m.view(R, rand, rand).repeat_interleave(scale, 1).repeat_interleave(scale, 2).contiguous()


def labelnoise_setup(ln):
    """add_label_noise's switches and moments (labelnoise.py:55-69, paired_image_dataset.py:344-352): (steps bitmask, means, vars)."""
    mean = [float(ln.get("tem_mean", 1)), float(ln.get("bright_mean", 1.15)), float(ln.get("contrast_mean", 1.15))]
    var = [float(ln.get("tem_var", 0.03)), float(ln.get("bright_var", 0.15)), float(ln.get("contrast_var", 0.15))]
    steps = sum(1 << k for k in range(3) if mean[k] != 1 or var[k] != 0)
    return steps, mean, var


def epoch_plan(sizes, opt, seed, epoch, rank=0, world=1):
    """The plan of one epoch of one rank, host tensors: ``rows`` (R,4) int32 (image, top, left, mode), ``noise`` (R,3) float32 or None,
    ``noise_steps``, ``mask`` (R,size,size) float32 or None, ``batches``.  R = batches * batch_size_per_gpu: a partial last batch is dropped."""
    sizes = torch.as_tensor(np.asarray(sizes), dtype=torch.int64)
    n, S, B = sizes.shape[0], int(opt["gt_size"]), int(opt.get("batch_size_per_gpu", 1))
    order = sampler_indices(n, world, rank, opt.get("dataset_enlarge_ratio", 1), epoch)
    nb = len(order) // B
    order = order[:nb * B]
    R = nb * B
    g = torch.Generator().manual_seed(plan_seed(seed, epoch, rank))
    hw = sizes[order]
    rng_t, rng_l = (hw[:, 0].clamp(min=S) - S), (hw[:, 1].clamp(min=S) - S)
    top = torch.minimum((torch.rand(R, generator=g, dtype=torch.float64) * (rng_t + 1)).floor().long(), rng_t)
    left = torch.minimum((torch.rand(R, generator=g, dtype=torch.float64) * (rng_l + 1)).floor().long(), rng_l)
    mode = torch.randint(0, 8, (R,), generator=g) if opt.get("geometric_augs", False) else torch.zeros(R, dtype=torch.int64)
    rows = torch.stack([order, top, left, mode], 1).to(torch.int32).contiguous()
    noise, steps = None, 0
    if opt.get("labelnoise"):
        steps, mean, var = labelnoise_setup(opt["labelnoise"])
        z = torch.randn(R, 3, generator=g, dtype=torch.float64)
        noise = (torch.tensor(mean, dtype=torch.float64) + torch.tensor(var, dtype=torch.float64) * z).float().contiguous()
    mask = None
    if opt.get("mim"):
        mask = mim_masks(R, *mim_geometry(opt), g)
    return dict(rows=rows, noise=noise, noise_steps=steps, mask=mask, batches=nb)


def pad_and_condition(lq, gt, s):
    """Validation on whole images: reflect-pad to a multiple of 4 * scale_down like eval.py:146-153, then the condition planes.
    Returns the batch dict without its paths; ``crop_hw`` is the unpadded size."""
    from bem import ops
    f = 4 * s
    hp, wp = lq.shape[-2] % f, lq.shape[-1] % f
    if hp or wp:
        Hp, Wp = lq.shape[-2] + (f - hp) % f, lq.shape[-1] + (f - wp) % f
        lqp, gtp = ops.pad_reflect(lq, Hp, Wp), ops.pad_reflect(gt, Hp, Wp)
    else:
        lqp, gtp = lq, gt
    return dict(lq=lqp, gt=gtp, lq_down=ops.resize_down(lqp, s), gt_down=ops.resize_down(gtp, s), crop_hw=tuple(lq.shape[-2:]))


class PairedImageBatchLoader:
    """One epoch of device batches from a PairedImageMaskDataset.  ``len()`` is the number of batches an epoch yields."""

    def __init__(self, dataset, dataset_opt, device, seed=0, rank=0, world=1, train=True):
        self.dataset, self.opt, self.device, self.seed, self.rank, self.world, self.train = dataset, dataset_opt, device, int(seed or 0), rank, world, train
        self.batch = int(dataset_opt.get("batch_size_per_gpu", 1)) if train else 1
        self.scale_down = int((dataset_opt.get("condition") or {}).get("scale_down", 16))
        self.epoch = 0
        if train:
            if dataset_opt.get("gt_size") is None:
                raise ValueError("Dataset_PairedImage_Mask: the train phase needs gt_size")
            S = int(dataset_opt["gt_size"])
            if self.scale_down % 2 or S % self.scale_down:
                raise ValueError(f"Dataset_PairedImage_Mask: condition.scale_down {self.scale_down} must be even and divide gt_size {S}")
        self.lq = torch.from_numpy(dataset.lq).to(device)
        self.gt = torch.from_numpy(dataset.gt).to(device)
        self.table = torch.from_numpy(dataset.table).contiguous()
        self.table_dev = self.table.to(device)

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        if not self.train:
            return len(self.dataset)
        return math.ceil(len(self.dataset) * self.opt.get("dataset_enlarge_ratio", 1) / self.world) // self.batch

    def __iter__(self):
        from bem import ops
        if not self.train:
            # one whole image per batch: a rectangular mode-0 crop of the full image, no condition planes from the kernel (s = 0)
            rows = torch.zeros(len(self.dataset), 4, dtype=torch.int32)
            rows[:, 0] = torch.arange(len(self.dataset), dtype=torch.int32)
            rows_dev = rows.to(self.device)
            for i in range(len(self.dataset)):
                H, W = int(self.table[i, 1]), int(self.table[i, 2])
                lq, gt, _, _ = ops.batch_assemble(self.lq, self.gt, self.table, self.table_dev, rows, rows_dev, i, 1, H, W, 0)
                out = pad_and_condition(lq, gt, self.scale_down)
                out["lq_path"] = [self.dataset.paths[i]["lq_path"]]
                yield out
            return
        plan = epoch_plan(self.dataset.sizes(), self.opt, self.seed, self.epoch, self.rank, self.world)
        rows, B, S = plan["rows"], self.batch, int(self.opt["gt_size"])
        # the epoch's three uploads; every step below reads its rows by offset
        rows_dev = rows.to(self.device)
        noise_dev = None if plan["noise"] is None else plan["noise"].to(self.device)
        mask_dev = None if plan["mask"] is None else plan["mask"].to(self.device)
        paths = self.dataset.paths
        for b in range(plan["batches"]):
            lq, gt, lqd, gtd = ops.batch_assemble(self.lq, self.gt, self.table, self.table_dev, rows, rows_dev, b * B, B, S, S, self.scale_down,
                                                  noise_dev=noise_dev, noise_steps=plan["noise_steps"])
            out = dict(lq=lq, gt=gt, lq_down=lqd, gt_down=gtd, lq_path=[paths[int(i)]["lq_path"] for i in rows[b * B:(b + 1) * B, 0]])
            if mask_dev is not None:
                out["mask"] = mask_dev[b * B:(b + 1) * B]
            yield out
