"""Float64 model of QD model3's attention dropout as the fold kernel applies it (csrc/chan_attn.hip, bem_attn_fold_drop_f32), written for
the tests from QD/model3.py:100-142 and include/bem_hip.h; it imports nothing of ``bem``.

  keep flag of map entry (b, map, i, j) under (seed, stream):  e = ((b * 2 + map) * 1024 + i * 32 + j)
      counter = (lo32(e >> 2), hi32(e >> 2), lo32(stream), hi32(stream)),  key = (lo32(seed), hi32(seed)),  word = philox4x32_10(...)[e & 3]
      u = (word >> 8) * 2^-24  (exact in float32),  kept iff u >= float32(p)
  the survivors are scaled by 1 / (1 - p), p taken as the float32 the C ABI passes.

  stream id of the draw:  bit 61 | rank << 44 | iteration << 8 | call index  (16 / 36 / 8 bits)"""
import numpy as np
import torch

import philox_ref as P

NAMES = ("q1_proj", "k2_proj", "v2_proj", "q2_proj", "k1_proj", "v1_proj", "out1", "out2")     # the order of the kernel's attn_w


def keep_mask(B, p, seed, stream_id, b0=0):
    """(B,2,32,32) float32 of 0 / 1: the keep flags of images b0 .. b0 + B - 1."""
    seed, stream_id = int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1)
    e = np.arange(b0 * 2048, (b0 + B) * 2048, dtype=np.uint64)
    j = e >> np.uint64(2)
    c = P.philox4x32_10((j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), stream_id & 0xFFFFFFFF, stream_id >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    word = c[(e & np.uint64(3)).astype(np.int64), np.arange(e.size)]
    u = ((word >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)
    return (u >= np.float32(p)).astype(np.float32).reshape(B, 2, 32, 32)


def stream_id(rank, iteration, call=0):
    assert 0 <= rank < 1 << 16 and 0 <= iteration < 1 << 36 and 0 <= call < 1 << 8
    return 2 ** 61 + rank * 2 ** 44 + iteration * 2 ** 8 + call


# The (seed, stream id) the device tests draw with.  Chosen on the host: test_model3_train_cpu.py::test_keep_mask_model holds this model's
# kept fraction over 16 384 draws to 0.9 +- 5 sigma under them.
SEED, STREAM = 20260, stream_id(0, 7, 1)


def drop_scale(p):
    return 1.0 / (1.0 - float(np.float32(p)))


def _attn(q, k, mask, p):
    """softmax(q k^T / sqrt(32)) over the pixels, then the dropout: (B,32,L) x 2 -> (B,32,32)."""
    a = torch.softmax((q * 32 ** -0.5) @ k.transpose(-1, -2), dim=-1)
    return a if mask is None else a * mask.to(a.dtype) * drop_scale(p)


def direct(f1, f2, w, fuse_w, fuse_b, mask=None, p=0.0):
    """fuse(cat(out1((attn_1 o m_1 / (1 - p)) v2) + f1, out2((attn_2 o m_2 / (1 - p)) v1) + f2)) as QD/model3.py:100-142 and :262-263 state
    it.  f1, f2 (B,32,H,W); w {name: (W (32,32), b (32))}; fuse_w (32,64); mask (B,2,32,32) or None.  Everything float64."""
    B, C, H, W = f1.shape
    x1, x2 = f1.reshape(B, C, H * W), f2.reshape(B, C, H * W)
    pr = lambda n, x: w[n][0] @ x + w[n][1][:, None]
    q1, k2, v2 = pr("q1_proj", x1), pr("k2_proj", x2), pr("v2_proj", x2)
    q2, k1, v1 = pr("q2_proj", x2), pr("k1_proj", x1), pr("v1_proj", x1)
    cross1 = _attn(q1, k2, None if mask is None else mask[:, 0], p) @ v2
    cross2 = _attn(q2, k1, None if mask is None else mask[:, 1], p) @ v1
    r1, r2 = pr("out1", cross1) + x1, pr("out2", cross2) + x2
    return (fuse_w @ torch.cat([r1, r2], 1) + fuse_b[:, None]).reshape(B, C, H, W)


def folded(f1, f2, w, fuse_w, fuse_b, mask=None, p=0.0):
    """The same map as one per-image matrix and bias, the mask applied at the softmax: (W_b (B,32,64), bias_b (B,32)) with
    fused = W_b [f1; f2] + bias_b.  M1 = Wo1 A1 Wv2, c1 = Wo1 A1 bv2 + bo1 (and 2 <-> 1):
    W_b = [Wfa + Wfb M2 | Wfa M1 + Wfb],  bias_b = Wfa c1 + Wfb c2 + bf."""
    B, C, H, W = f1.shape
    x1, x2 = f1.reshape(B, C, H * W), f2.reshape(B, C, H * W)
    pr = lambda n, x: w[n][0] @ x + w[n][1][:, None]
    A1 = _attn(pr("q1_proj", x1), pr("k2_proj", x2), None if mask is None else mask[:, 0], p)
    A2 = _attn(pr("q2_proj", x2), pr("k1_proj", x1), None if mask is None else mask[:, 1], p)
    M1, c1 = w["out1"][0] @ A1 @ w["v2_proj"][0], w["out1"][0] @ (A1 @ w["v2_proj"][1])[..., None] + w["out1"][1][:, None]
    M2, c2 = w["out2"][0] @ A2 @ w["v1_proj"][0], w["out2"][0] @ (A2 @ w["v1_proj"][1])[..., None] + w["out2"][1][:, None]
    Wfa, Wfb = fuse_w[:, :32], fuse_w[:, 32:]
    Wb = torch.cat([Wfa + Wfb @ M2, Wfa @ M1 + Wfb], -1)
    bias = (Wfa @ c1 + Wfb @ c2).squeeze(-1) + fuse_b
    return Wb, bias


def apply_folded(Wb, bias, f1, f2):
    B, C, H, W = f1.shape
    return (Wb @ torch.cat([f1.reshape(B, C, -1), f2.reshape(B, C, -1)], 1) + bias[..., None]).reshape(B, C, H, W)


def random_case(B, H, W, seed, p=0.1, scale=0.15):
    """f1, f2 (B,32,H,W), the eight 1x1 layers and the fuse layer, a random 0 / 1 mask: float64, unit-scale features."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    f1, f2 = r(B, 32, H, W), r(B, 32, H, W)
    w = {n: (scale * r(32, 32), 0.1 * r(32)) for n in NAMES}
    fuse_w, fuse_b = scale * r(32, 64), 0.1 * r(32)
    mask = (torch.rand(B, 2, 32, 32, generator=g) >= p).to(torch.float64)
    return f1, f2, w, fuse_w, fuse_b, mask


def pack_attn_w(w):
    """The kernel's attn_w: 8 x (32x32 + 32) float32 in NAMES order."""
    return torch.cat([torch.cat([w[n][0].reshape(-1), w[n][1].reshape(-1)]) for n in NAMES]).float().contiguous()
