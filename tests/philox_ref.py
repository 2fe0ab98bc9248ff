"""Float64 numpy model of the project's N(0,1) draws: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
SC'11) followed by Box-Muller, element for element as csrc/bem_common.h defines them.  Written for the tests from that header and the
published algorithm; it imports nothing of ``bem``.

  draw of element i under (seed, stream):  counter = (lo32(i >> 2), hi32(i >> 2), lo32(stream), hi32(stream)),  key = (lo32(seed), hi32(seed))
  c = philox4x32_10(counter, key);  h = (i & 3) >> 1
  u1 = ((c[2h] >> 8) + 1) / 2^24 in (0, 1],   u2 = (c[2h+1] >> 8) / 2^24 in [0, 1)      (both exact in float32)
  r = sqrt(-2 ln u1);   z = r cos(2 pi u2) for even i,  r sin(2 pi u2) for odd i

The high word of the block counter is reached by element counts >= 2^34 only (64 GB per tensor): no tensor of the model is near that,
so that word is covered by the known-answer vectors of test_philox_cpu.py alone.

The stream-id layout restated here is the documented one (docstring of SampleCtx.next_stream, the noise draw of BEMPipeline.candidates):
  weights:  [ rank : 16 bits | forward epoch : 24 bits | tensor counter : 20 bits ]  =  rank << 44 | epoch << 20 | counter
  noise:    bit 62 | rank << 44 | epoch            (the epoch in the LOW bits)"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)      # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                            # key schedule (Weyl) increments
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (scalars or equal-length arrays, taken modulo 2^32) -> uint32 array (4, n)."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & _LO for v in counter]
    n = max(v.size for v in c)
    c = [np.broadcast_to(v, (n,)).copy() for v in c]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c).astype(np.uint32)


def normals(n, seed, stream_id, first=0):
    """Draws of elements first .. first + n - 1 under (seed, stream_id): (z float64[n], r float64[n]); r = sqrt(-2 ln u1) is the
    Box-Muller radius of the element's pair -- rounding errors of a float32 evaluation scale with it."""
    seed, stream_id = int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1)
    j0, j1 = first >> 2, (first + max(n, 1) - 1) >> 2
    j = np.arange(j0, j1 + 1, dtype=np.uint64)
    c = philox4x32_10((j & _LO, j >> _S32, stream_id & 0xFFFFFFFF, stream_id >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    zz, rr = np.empty((j.size, 4)), np.empty((j.size, 4))
    for h in range(2):
        u1 = ((c[2 * h] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
        u2 = (c[2 * h + 1] >> np.uint32(8)).astype(np.float64) / 16777216.0
        r = np.sqrt(-2.0 * np.log(u1))
        zz[:, 2 * h], zz[:, 2 * h + 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
        rr[:, 2 * h] = rr[:, 2 * h + 1] = r
    lo = first - 4 * j0
    return zz.reshape(-1)[lo:lo + n], rr.reshape(-1)[lo:lo + n]


def stream_id(rank, epoch, counter):
    assert 0 <= rank < 1 << 16 and 0 <= epoch < 1 << 24 and 0 <= counter < 1 << 20
    return rank * 2 ** 44 + epoch * 2 ** 20 + counter


def noise_stream_id(rank, epoch):
    assert 0 <= rank < 1 << 16 and 0 <= epoch < 1 << 24
    return 2 ** 62 + rank * 2 ** 44 + epoch


def softplus64(x):
    x = np.asarray(x, dtype=np.float64)
    return np.logaddexp(0.0, x)
