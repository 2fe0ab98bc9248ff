"""The CPU model of the weight sampler (tests/philox_ref.py) against the published Philox4x32-10 known-answer vectors, its statistics
over 2^22 draws, and the host-side stream-id arithmetic (SampleCtx is plain Python) against the documented bit layout.  No GPU."""
import itertools

import numpy as np
import pytest

import philox_ref as P

# Random123 kat_vectors, philox4x32 with 10 rounds:  counter ; key -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_known_answer_vectors(ctr, key, out):
    got = P.philox4x32_10(ctr, key)
    assert got.shape == (4, 1) and got.dtype == np.uint32
    assert tuple(int(v) for v in got[:, 0]) == out, " ".join(f"{int(v):08x}" for v in got[:, 0])


def test_known_answer_vectors_vectorised():
    """The three vectors as one call share a key only pairwise, so: each counter inside an array of other counters."""
    for ctr, key, out in KAT:
        arr = [np.array([1, c, 2], dtype=np.uint64) for c in ctr]
        got = P.philox4x32_10(arr, key)
        assert tuple(int(v) for v in got[:, 1]) == out


def test_normals_index_mapping():
    """normals(n, ., ., first) is a window of the same sequence; element i uses block i >> 2, pair (i & 3) >> 1, cos for even i."""
    z, r = P.normals(24, 0xDEADBEEF00000007, (1 << 62) | (5 << 44) | 9)
    for first, n in ((0, 1), (1, 3), (3, 5), (4, 4), (7, 16), (23, 1)):
        zw, rw = P.normals(n, 0xDEADBEEF00000007, (1 << 62) | (5 << 44) | 9, first=first)
        assert np.array_equal(zw, z[first:first + n]) and np.array_equal(rw, r[first:first + n])
    assert np.array_equal(r[0::2], r[1::2])                          # one radius per pair
    assert np.allclose(z[0::2] ** 2 + z[1::2] ** 2, r[0::2] ** 2, rtol=1e-14, atol=0)
    c = P.philox4x32_10((2, 0, 9, (1 << 30) | (5 << 12)), (7, 0xDEADBEEF))[:, 0]          # block 2 = elements 8 .. 11
    u1, u2 = ((int(c[2]) >> 8) + 1) / 2 ** 24, (int(c[3]) >> 8) / 2 ** 24
    assert z[10] == np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2) and z[11] == np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2)
    assert np.isfinite(z).all() and (r >= 0).all()


def _corr(a, b):
    return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))


def test_model_statistics():
    """n = 2^22 draws, k = 5 sigma sampling bounds (about 6e-7 per check, two-sided, if the draws are iid N(0,1)):
         mean        sd = 1 / sqrt(n)                   -> |m|        <= k / sqrt(n)
         variance    Var(z^2) = 2                       -> |v - 1|    <= k sqrt(2 / n)
         4th moment  Var(z^4) = E z^8 - 9 = 96          -> |m4 - 3|   <= k sqrt(96 / n)
         correlation of two independent unit-variance sequences (lags, streams, seeds):  sd = 1 / sqrt(n) -> |rho| <= k / sqrt(n)
       The 24-bit uniforms cut the radius off at sqrt(2 ln 2^24) = 5.77: the moments lose less than 1e-4, far inside the bounds."""
    n, k = 1 << 22, 5.0
    seed, s = 0x0123456789ABCDEF, P.stream_id(3, 17, 42)
    z, r = P.normals(n, seed, s)
    assert abs(z.mean()) <= k / np.sqrt(n), z.mean()
    assert abs(z.var() - 1) <= k * np.sqrt(2 / n), z.var()
    assert abs((z ** 4).mean() - 3) <= k * np.sqrt(96 / n), (z ** 4).mean()
    assert r.max() <= np.sqrt(2 * np.log(2 ** 24)) + 1e-12
    for lag in (1, 2, 3, 4):
        c = _corr(z[:-lag], z[lag:])
        assert abs(c) <= k / np.sqrt(n - lag), (lag, c)
    for what, other in (("stream s + 1", P.normals(n, seed, s + 1)[0]), ("stream s + 2^20", P.normals(n, seed, s + (1 << 20))[0]),
                        ("stream s + 2^44", P.normals(n, seed, s + (1 << 44))[0]), ("seed k + 2^32", P.normals(n, seed + (1 << 32), s)[0]),
                        ("seed k + 1", P.normals(n, seed + 1, s)[0])):
        c = _corr(z, other)
        assert abs(c) <= k / np.sqrt(n), (what, c)
        assert not np.array_equal(z[:64], other[:64]), what


RANKS, EPOCHS, TENSORS = (0, 1, 65535), (1, 2, (1 << 24) - 1), 1000


def test_stream_id_layout():
    """SampleCtx hands out rank << 44 | epoch << 20 | counter, counter = 1, 2, ...: pairwise distinct over ranks, epochs and tensors, bit
    62 clear, and no condition-noise id (bit 62 | rank << 44 | epoch) among them."""
    from bem.modules import SampleCtx
    ids = {}
    for rank, epoch in itertools.product(RANKS, EPOCHS):
        ctx = SampleCtx(4, None, seed=9, rank=rank, epoch=epoch)
        for t in range(1, TENSORS + 1):
            sid = ctx.next_stream()
            assert sid == P.stream_id(rank, epoch, t), (rank, epoch, t, hex(sid))
            assert 0 <= sid < 1 << 62 and not (sid >> 62) & 1
            assert (sid >> 44, (sid >> 20) & 0xFFFFFF, sid & 0xFFFFF) == (rank, epoch, t)
            ids[sid] = (rank, epoch, t)
    assert len(ids) == len(RANKS) * len(EPOCHS) * TENSORS
    noise = {P.noise_stream_id(rank, epoch) for rank, epoch in itertools.product(RANKS, EPOCHS)}
    assert len(noise) == len(RANKS) * len(EPOCHS) and not noise & set(ids)
    assert all((v >> 62) & 1 and v < 1 << 63 for v in noise)


def test_stream_id_default_epoch_is_a_fresh_forward():
    from bem.modules import SampleCtx
    a, b = SampleCtx(1, None, seed=0, rank=2), SampleCtx(1, None, seed=0, rank=2)
    assert b.epoch == a.epoch + 1 == SampleCtx._epoch
    assert a.next_stream() == P.stream_id(2, a.epoch, 1) and b.next_stream() == P.stream_id(2, b.epoch, 1)


def test_stream_id_exhaustion_raises():
    from bem.modules import SampleCtx
    ctx = SampleCtx(1, None, seed=0, rank=0, epoch=1)
    ctx.counter = (1 << 20) - 2
    assert ctx.next_stream() == P.stream_id(0, 1, (1 << 20) - 1)      # the last id of the forward
    with pytest.raises(RuntimeError):
        ctx.next_stream()                                             # counter 2^20 would carry into the epoch field
    with pytest.raises(RuntimeError):
        SampleCtx(1, None, seed=0, rank=0, epoch=1 << 24).next_stream()   # epoch 2^24 would carry into the rank field
    assert SampleCtx(1, None, seed=0, rank=0, epoch=(1 << 24) - 1).next_stream() == P.stream_id(0, (1 << 24) - 1, 1)


def test_stream_id_with_device_epoch():
    """With ``epoch_dev`` the ids carry epoch 0 and the kernels add the device word ``epoch << 20``: id + (epoch << 20) is the id of the
    same tensor under a host epoch -- the identity a captured step relies on."""
    from bem.modules import SampleCtx
    for rank, epoch in itertools.product(RANKS, EPOCHS):
        dev_word = object()                                           # any non-None stands for the device tensor on the host side
        c0 = SampleCtx(1, None, seed=5, rank=rank, epoch=epoch, epoch_dev=dev_word)
        c1 = SampleCtx(1, None, seed=5, rank=rank, epoch=epoch)
        assert c0.epoch == 0 and c0.epoch_dev is dev_word
        for t in range(1, 65):
            a, b = c0.next_stream(), c1.next_stream()
            assert a == P.stream_id(rank, 0, t) and (a >> 20) & 0xFFFFFF == 0
            assert (a + (epoch << 20)) & (2 ** 64 - 1) == b == P.stream_id(rank, epoch, t)
