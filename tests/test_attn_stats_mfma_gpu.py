"""bem_attn_stats_f64 on the f64 matrix cores (csrc/chan_attn.hip): S = F1 F2^T and the two channel sums per image against the host.

A workgroup takes a `chunk` of pixels, its four waves 16-pixel groups of it, a lane four pixels of a group; rows are loaded as float4
when L % 4 == 0 and with guarded scalar loads otherwise (for odd L the rows of images b >= 1 are not 16-byte aligned).  The sizes below
sit on every one of those seams.  The chunk is chosen per launch (`chunk_of` restates the launcher's rule): 256 for everything small,
512 / 1024 / 2048 only once B L is large, which the three cases of test_exact_integers_large_chunks reach.

Three kinds of check:
  * float64 parity at the tolerance of tests/test_ops_gpu.py::test_attn_stats_f64 (rtol 1e-12, atol 1e-10, unit-scale inputs);
  * integer-valued inputs: every product and every partial sum is an integer far below 2^53, so the result must EQUAL the integer
    reference whatever the order of the sums -- a pixel counted twice or left out at a chunk, group or tail seam cannot hide here;
  * cancellation: f1 = 1e4 + randn, f2 = -1e4 + randn.  Sums of ~1e8-sized products: an f32 accumulation anywhere would be off by
    ~6e-8 of sum |f1 f2|, the bound is 1e-12 of it."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 32
CHUNK = 256                                                      # what every B in {1, 3} launch below this file's large cases gets


def chunk_of(B, L):
    chunk = 2048
    while chunk > 256 and B * ((L + chunk - 1) // chunk) < 512:
        chunk //= 2
    return chunk


def stats_gpu(f1, f2):
    from bem import native
    B, L = f1.shape[0], f1.shape[2]
    d1, d2 = f1.cuda().contiguous(), f2.cuda().contiguous()
    out = torch.full((B, C * C + 2 * C), float("nan"), device="cuda", dtype=torch.float64)     # the call zeroes it itself
    native.check(native.lib().bem_attn_stats_f64(ctypes.c_void_p(d1.data_ptr()), ctypes.c_void_p(d2.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, L,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "attn_stats")
    return out.cpu()


def stats_ref(a, b):
    """a, b (B, 32, L) in float64 or int64 -> (B, 1088) like the kernel's stats."""
    S = torch.einsum("bip,bjp->bij", a, b) if a.dtype == torch.int64 else a @ b.transpose(1, 2)
    return torch.cat([S.reshape(a.shape[0], -1), a.sum(-1), b.sum(-1)], 1)


LS = (1, 3, 4, 15, 16, 17, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", LS)
def test_float64_parity(B, L):
    assert chunk_of(B, L) == CHUNK
    g = torch.Generator().manual_seed(1000 * L + B)
    f1, f2 = torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g) * 0.5 + 0.1
    got, want = stats_gpu(f1, f2), stats_ref(f1.double(), f2.double())
    err = float((got - want).abs().max())
    print(f"B={B} L={L}: max |diff| = {err:.3e}")
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-10), err


@pytest.mark.parametrize("B,L", [(1, 4099), (3, 4099), (3, 4096), (3, 2 * CHUNK + 5), (3, 65), (1, 3)])
def test_exact_integers(B, L):
    """|v| <= 1024, L <= 4099: sums below 2^20 2^13 = 2^33.  F1 and F2 are drawn independently, so S is not symmetric and a swap of the
    two operands or of rows and columns shows."""
    assert chunk_of(B, L) == CHUNK
    g = torch.Generator().manual_seed(77 * L + B)
    i1, i2 = torch.randint(-1024, 1025, (B, C, L), generator=g), torch.randint(-1024, 1025, (B, C, L), generator=g)
    got, want = stats_gpu(i1.float(), i2.float()), stats_ref(i1, i2)
    assert got.abs().max() < 2.0 ** 53
    bad = got.to(torch.int64) != want
    assert torch.equal(got, got.round()) and not bad.any(), f"{int(bad.sum())} of {bad.numel()} statistics differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("B,L,chunk", [(3, 512 * 171 + 1, 512), (3, 1024 * 171 + 3, 1024), (3, 2048 * 171 + 4, 2048)])
def test_exact_integers_large_chunks(B, L, chunk):
    """The launches that get a chunk above 256: scalar loads at 512 and 1024 (L odd), float4 at 2048.  |v| <= 16 keeps every sum below
    2^8 L < 2^27, so the float64 matrix product of the host is exact too and serves as the integer reference."""
    assert chunk_of(B, L) == chunk
    g = torch.Generator().manual_seed(L)
    i1, i2 = torch.randint(-16, 17, (B, C, L), generator=g), torch.randint(-16, 17, (B, C, L), generator=g)
    got, want = stats_gpu(i1.float(), i2.float()), stats_ref(i1.double(), i2.double())
    bad = got != want
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} statistics differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("B,L", [(3, 2 * CHUNK + 5), (3, 4096), (1, 17)])
def test_cancellation(B, L):
    g = torch.Generator().manual_seed(5 * L + B)
    f1, f2 = 1e4 + torch.randn(B, C, L, generator=g), -1e4 + torch.randn(B, C, L, generator=g)
    a, b = f1.double(), f2.double()
    got, want = stats_gpu(f1, f2), stats_ref(a, b)
    scale = stats_ref(a.abs(), b.abs())                                              # sum |f1 f2| per entry, sum |f| for the channel sums
    rel = float(((got - want).abs() / scale).max())
    print(f"B={B} L={L}: max |diff| / sum|f1 f2| = {rel:.3e}")
    assert rel <= 1e-12, rel
