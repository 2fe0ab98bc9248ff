"""The x6-packing samplers (csrc/pack.hip sample_pack_x6_item) evaluate only the Philox counter blocks their live elements read: two
per lane when every lane's first element opens a block (K % 4 == 0), one when four or fewer elements are live, none for a lane of
padding, up to three otherwise.  Whatever they skip, every stored word must be what it was: the packed draws, decoded (the three bf16
limbs of a value add up to it exactly), are compared BIT FOR BIT with bnn_sample -- natural order, one thread per counter block, its own
indexing (bnn_sample_kernel) -- on the same (seed, stream), and the padding words (rows >= M, k >= K) must be zero limbs.
On the aligned path a lane also reads its mu and sigma as one or two float4 (four or eight live elements) when both tensors start on a
16-byte boundary, and with dword loads when they do not: test_unaligned_parameters.

Both launch forms: bnn_sample_packed(..., sigma_given=True) (sample_pack_x6_kernel) and one EvalSampleBank launch
(bem_bnn_ebank_sample_f32, ebank_sample_kernel).

  (M, K)      sets   branch
  (40, 40)    3      aligned; at kb = 2 the upper lane half lies past K (no block) and the lower half has 8 live elements
  (33, 160)   3      aligned, two blocks everywhere; rows 33..63 of the second row tile are padding
  (5, 12)     3      aligned, K % 8 = 4: the upper lane half has 4 live elements, one block
  (3, 27)     3      K % 4 != 0 and M K % 4 != 0: sets 1 and 2 start at offsets 1 and 2 in their block, the three-block path
  (1, 8)      1      the smallest aligned case"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import philox_ref as P

pytestmark = pytest.mark.gpu

SHAPES = ((40, 40, 3), (33, 160, 3), (5, 12, 3), (3, 27, 3), (1, 8, 1))
SEED = 0x0BADF00D00000007
RHO0 = float(np.log(np.expm1(0.05)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as _ops
    return _ops


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def decode_x6(Wp, M, K):
    """(nsets, packed(M, K)) -> natural (nsets, M, K) float32 and the largest |limb word| of the padding.  16-byte vector
    ((set MT + mt) KB + kb) 3 64 + limb 64 + lane holds, for row mt 32 + (lane & 31), the eight k = kb 16 + (lane >> 5) 8 + e as bf16
    pairs, even e in the low half."""
    ns, MT, KB = Wp.shape[0], (M + 31) // 32, (K + 15) // 16
    u = Wp.contiguous().view(torch.int32).view(ns, MT, KB, 3, 2, 32, 4)
    limbs = torch.stack([u & 0xFFFF, (u >> 16) & 0xFFFF], -1)                                       # (ns, MT, KB, limb, kh, row, q, j)
    limbs = limbs.permute(3, 0, 1, 5, 2, 4, 6, 7).reshape(3, ns, MT * 32, KB * 16)                  # (limb, set, row, k)
    pad = torch.ones(MT * 32, KB * 16, dtype=torch.bool, device=Wp.device)
    pad[:M, :K] = False
    vals = (limbs << 16).view(torch.float32).double().sum(0)
    return vals[:, :M, :K].float().contiguous(), int(limbs[:, :, pad].abs().max()) if bool(pad.any()) else 0


def mu_rho(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g).cuda(), (RHO0 + 4 * torch.rand(M, K, generator=g) - 2).cuda()


def test_shapes_reach_the_branches():
    """The table of the module docstring, worked out from the kernel's own indexing."""
    def lanes(M, K, ns):
        s, row, k0 = np.meshgrid(np.arange(ns), np.arange(M), np.arange(0, (K + 15) // 16 * 16, 8), indexing="ij")
        live = np.clip(K - k0, 0, 8)
        off = (s * M * K + row * K + k0) & 3
        blocks = np.where(live > 0, ((off + live - 1) >> 2) + 1, 0)
        return off[live > 0], live, blocks
    off, live, blocks = lanes(40, 40, 3)
    assert set(off) == {0} and set(live.ravel()) == {0, 8} and set(blocks.ravel()) == {0, 2}
    off, live, blocks = lanes(33, 160, 3)
    assert set(off) == {0} and set(blocks.ravel()) == {2}
    off, live, blocks = lanes(5, 12, 3)
    assert set(off) == {0} and set(live.ravel()) == {4, 8} and set(blocks.ravel()) == {1, 2}
    off, live, blocks = lanes(3, 27, 3)
    assert set(off) == {0, 1, 2, 3} and 3 in set(blocks.ravel()) and 27 % 4 and (3 * 27) % 4
    off, live, blocks = lanes(1, 8, 1)
    assert set(off) == {0} and set(blocks.ravel()) == {0, 2}                        # K = 8 of a 16-wide block: the upper lane half is padding


@pytest.mark.parametrize("M,K,ns", SHAPES)
def test_packed_sampler_equals_natural_sampler(ops, M, K, ns):
    mu, rho = mu_rho(M, K, 1000 * M + K)
    sigma = ops.bnn_sample(torch.zeros_like(mu), rho, 1, torch.ones_like(mu))[0]                    # log1p(exp(rho)) by the sampler itself
    for sid in (P.stream_id(7, 300 + ns, M * K), (1 << 62) | (9 << 44) | 0xFFFFFFFF):
        nat = ops.bnn_sample(mu, rho, ns, None, seed=SEED, stream_id=sid)
        for sig in (True, False):
            Wp = ops.bnn_sample_packed(mu, sigma if sig else rho, ns, M, K, None, seed=SEED, stream_id=sid, sigma_given=sig)
            got, pad = decode_x6(Wp, M, K)
            assert bits_equal(got, nat), f"M={M} K={K} nsets={ns} sigma_given={sig}: {int((got != nat).sum())} of {nat.numel()} draws differ"
            assert pad == 0, "padding limbs are not zero"


def test_unaligned_parameters(ops):
    """K % 4 == 0 but mu / sigma start 4, 8 or 12 bytes past a 16-byte boundary: the aligned path's dword loads, same bits."""
    M, K, ns = 40, 40, 3
    mu0, rho0 = mu_rho(M, K, 99)
    sid = P.stream_id(1, 2, 3)
    want = None
    for shift in (0, 1, 2, 3):
        mu = torch.empty(M * K + 4, device="cuda")[shift:shift + M * K].view(M, K).copy_(mu0)
        rho = torch.empty(M * K + 4, device="cuda")[shift:shift + M * K].view(M, K).copy_(rho0)
        assert mu.data_ptr() % 16 == 4 * shift and rho.data_ptr() % 16 == 4 * shift and mu.is_contiguous()
        sigma = torch.empty(M * K + 4, device="cuda")[shift:shift + M * K].view(M, K).copy_(ops.bnn_sample(torch.zeros_like(mu0), rho0, 1, torch.ones_like(mu0))[0])
        Wp = ops.bnn_sample_packed(mu, sigma, ns, M, K, None, seed=SEED, stream_id=sid, sigma_given=True)
        want = ops.bnn_sample(mu0, rho0, ns, None, seed=SEED, stream_id=sid) if want is None else want
        got, pad = decode_x6(Wp, M, K)
        assert bits_equal(got, want) and pad == 0, f"parameters {4 * shift} bytes past a 16-byte boundary"


class Leaves(nn.Module):
    def __init__(self):
        super().__init__()
        from bem.modules import Linear2dReparameterization as L
        self.leaves = nn.ModuleList([L(K, M, bias=False) for M, K, _ in SHAPES])

    def draw(self, B):
        return [m.gemm_weights(B)[0] for m in self.leaves]


def test_eval_bank_equals_natural_sampler(ops):
    """All five shapes as segments of one bem_bnn_ebank_sample_f32 launch, three sets each."""
    from bem.modules import EvalSampleBank, SampleCtx, sampling
    net = Leaves().cuda().eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.copy_((torch.randn(p.shape, generator=g) if "mu_" in name else RHO0 + 4 * torch.rand(p.shape, generator=g) - 2).to(p.device))
    ns, rank, epoch = 3, 513, 70001
    with sampling(SampleCtx(ns, None, seed=SEED, rank=rank, epoch=epoch)):
        net.draw(ns)                                                                                # leaf by leaf: records form and stream of every leaf
    bank = EvalSampleBank(net)
    ctx = SampleCtx(ns, None, seed=SEED, rank=rank, epoch=epoch)
    ctx.counter0 = ctx.counter
    assert bank.usable(ctx)
    bank.sample(ctx)
    assert ctx.bank is bank and bank.nrows == len(SHAPES)
    with sampling(ctx):
        banked = net.draw(ns)
    for t, (m, Wp, (M, K, _)) in enumerate(zip(net.leaves, banked, SHAPES), 1):
        assert m._mk == (M, K) and Wp.data_ptr() >= bank.arena.data_ptr() and Wp.data_ptr() < bank.arena.data_ptr() + 4 * bank.arena.numel()
        nat = ops.bnn_sample(m.mu_weight.detach().reshape(M, K), m.rho_weight.detach().reshape(M, K), ns, None, seed=SEED, stream_id=P.stream_id(rank, epoch, t))
        got, pad = decode_x6(Wp, M, K)
        assert bits_equal(got, nat), f"segment {t} M={M} K={K}: {int((got != nat).sum())} of {nat.numel()} draws differ"
        assert pad == 0, f"segment {t}: padding limbs are not zero"
