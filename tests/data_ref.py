"""numpy oracle of the folder dataset's batch preparation, written from the reference's semantics (not from the kernel):

    P    = np.pad(src, ((0, max(0, S-H)), (0, max(0, S-W)), (0, 0)), 'symmetric')   cv2.BORDER_REFLECT, utils/img_util.py:196-211
    crop = P[top:top+S, left:left+S]
    aug  = rot90(crop, mode // 2), then flipud if mode % 2                           data/transforms.py:228-273
    x    = aug.astype(float32) / float32(255)

plus utils/labelnoise.py:55-69 in the RGB layout, utils/mask.py's structure, data/data_sampler.py:21-42 and the x1/s INTER_LINEAR
plane of an even s (0.25 * the four centre taps).  tests/golden/g18_data.npz pins these against the reference's own functions."""
import math

import numpy as np
import torch


def augment_ref(a, mode):
    out = np.rot90(a, mode // 2)
    return np.flipud(out) if mode % 2 else out


def assemble_ref(src, top, left, mode, Sh, Sw=None):
    """src (H,W,3) uint8 RGB -> (3,Sh,Sw) float32 (rotating modes: Sh == Sw)."""
    Sw = Sh if Sw is None else Sw
    H, W, _ = src.shape
    P = np.pad(src, ((0, max(0, Sh - H)), (0, max(0, Sw - W)), (0, 0)), "symmetric")
    crop = P[top:top + Sh, left:left + Sw]
    assert crop.shape[:2] == (Sh, Sw), (crop.shape, top, left)
    x = augment_ref(crop, mode).astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def temperature_ref(x, t):
    """x (...,3) float32 RGB; the reference multiplies BGR by [t, 1, 1/t] in float64, clips, and the next step rounds to float32."""
    t = float(np.float32(t))
    adj = np.array([1.0 / t, 1.0, t])
    return np.clip(x.astype(np.float32) * adj, 0, 1).astype(np.float32)


def brightness_ref(x, b):
    return np.clip(x.astype(np.float32) * np.float32(b), 0, 1)


def contrast_ref(x, c):
    return np.clip(np.float32(c) * (x.astype(np.float32) - np.float32(0.5)) + np.float32(0.5), 0, 1)


def label_noise_ref(x_chw, t, b, c, steps=7):
    """(3,H,W) float32 RGB -> the same after add_label_noise with the given factors (steps: bit 0 temperature, 1 brightness, 2 contrast)."""
    x = x_chw.transpose(1, 2, 0)
    if steps & 1:
        x = temperature_ref(x, t)
    if steps & 2:
        x = brightness_ref(x, b)
    if steps & 4:
        x = contrast_ref(x, c)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def resize_down_ref(x, s):
    """(...,H,W) float32 -> (...,H/s,W/s): 0.25f * (p[0] + p[W] + p[1] + p[W+1]) at taps s/2-1, s/2, in that order, float32."""
    a = s // 2 - 1
    p00, p10, p01, p11 = x[..., a::s, a::s], x[..., a + 1::s, a::s], x[..., a::s, a + 1::s], x[..., a + 1::s, a + 1::s]
    return np.float32(0.25) * (((p00 + p10) + p01) + p11)


def sampler_ref(n, world, rank, ratio, epoch):
    num = math.ceil(n * ratio / world)
    g = torch.Generator()
    g.manual_seed(epoch)
    idx = [v % n for v in torch.randperm(num * world, generator=g).tolist()]
    return idx[rank:num * world:world]


def mask_structure_ok(m, rand, scale, count):
    """m (rand*scale, rand*scale) of 0/1: constant scale x scale blocks, exactly ``count`` blocks set."""
    m = np.asarray(m)
    if m.shape != (rand * scale, rand * scale) or not np.isin(m, (0, 1)).all():
        return False
    blocks = m.reshape(rand, scale, rand, scale)
    base = blocks[:, :1, :, :1]
    return bool((blocks == base).all()) and int(base.sum()) == count


def ulp_diff(a, b):
    """Largest distance in float32 units in the last place between two non-negative float32 arrays."""
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())
