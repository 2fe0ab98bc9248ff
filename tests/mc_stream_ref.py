"""numpy restatement of the streamed Monte-Carlo statistics (csrc/selection.hip: mc_accum_kernel, mc_std_kernel) -- the checker of
tests/test_sample_chunk_*.py, not the product.  Every operation is rounded to float32 on its own, like the kernel's (contraction off),
so the state is a function of the sample sequence alone and any split into chunks leaves the same bits."""
import numpy as np

F = np.float32


class Stream:
    """sum of the clamped raw crops, and Welford's running mean / m2 of the finished candidates; planes (B,3,h,w) float32."""

    def __init__(self, B, h, w):
        self.sum, self.mean, self.m2 = (np.zeros((B, 3, h, w), F) for _ in range(3))
        self.h, self.w, self.n = h, w, 0

    def accum(self, raw=None, final=None):
        """raw (B,Nc,3,Hp,Wp) and / or final (B,Nc,3,h,w), float32: one chunk, its samples in order."""
        Nc = (raw if raw is not None else final).shape[1]
        for n in range(Nc):
            if raw is not None:
                self.sum = self.sum + np.clip(raw[:, n, :, :self.h, :self.w].astype(F), F(0), F(1))
            if final is not None:
                x, k = final[:, n].astype(F), F(self.n + n + 1)
                d = x - self.mean
                self.mean = self.mean + d / k
                self.m2 = self.m2 + d * (x - self.mean)
                assert d.dtype == F and self.mean.dtype == F and self.m2.dtype == F
        self.n += Nc

    def mc(self):
        return np.clip(self.sum / F(self.n), F(0), F(1))

    def std(self):
        return np.sqrt(self.m2 / F(self.n - 1)) if self.n > 1 else np.zeros_like(self.m2)


def run(final, splits, raw=None):
    """final (B,N,3,h,w) [, raw (B,N,3,Hp,Wp)] accumulated in chunks of the sizes ``splits`` -> Stream."""
    B, N, _, h, w = final.shape
    assert sum(splits) == N
    s, lo = Stream(B, h, w), 0
    for n in splits:
        s.accum(None if raw is None else raw[:, lo:lo + n], final[:, lo:lo + n])
        lo += n
    return s


def std64(final):
    """The unbiased std over the samples in float64 on the same float32 inputs: what the f32 recurrence is measured against."""
    return final.astype(np.float64).std(axis=1, ddof=1)


def kernel_inputs(seed=3, B=2, N=5, Hp=20, Wp=24, h=17, w=21):
    """The kernel-level case of the GPU test: raw values partly outside [0,1]; final = the clamped crop (what candidate_finalize leaves
    without GT-mean)."""
    g = np.random.default_rng(seed)
    raw = (0.5 + 0.45 * g.standard_normal((B, N, 3, Hp, Wp))).astype(F)
    final = np.clip(raw[..., :h, :w], 0, 1).astype(F)
    return raw, final


def cancellation_inputs(seed=5, N=8, h=16, w=16):
    """final = 0.9 + 1e-4 randn: where a sum-of-squares accumulator in f32 loses everything and Welford does not."""
    g = np.random.default_rng(seed)
    return (0.9 + 1e-4 * g.standard_normal((1, N, 3, h, w))).astype(F)


# Worst |f32 recurrence - float64| of the std map on kernel_inputs(), measured on the CPU by test_sample_chunk_cpu.py (which asserts
# the restatement stays under it): the GPU, whose division and square root round like numpy's, is allowed 4x this.
REF_STD_DEV = 5.7e-8          # measured 5.694e-8 (std values between 0.03 and 0.55: about one ulp of the largest)
