"""Score rows and tables shared by tests/test_selection_gpu.py and tests/test_selection_cpu.py for the selection rules' edges (not collected
by pytest).  The references stay in tests/selection_ref.py; here are only inputs, so that the CPU tests can check the conditions the GPU tests
rely on, on the very same tables."""
import torch

import selection_ref as R

NAN = float("nan")
# the rows of test_selection_with_nan_scores: a NaN first, in the middle, last, everywhere, and between two equal maxima
NAN_ROWS = [[NAN, 20.0, 30.0, 25.0], [20.0, NAN, 30.0, 25.0], [30.0, 20.0, 25.0, NAN], [NAN, NAN, NAN, NAN], [20.0, 30.0, NAN, 30.0]]
# + all equal (the first index must hold through every chunk) and strictly decreasing ('min' moves at every sample)
MERGE_ROWS = NAN_ROWS + [[7.0, 7.0, 7.0, 7.0], [4.0, 3.0, 2.0, 1.0]]


def compositions(n):
    """Every way to write n as an ordered sum of positive chunk sizes: 2^(n-1) tuples."""
    if n == 0:
        yield ()
    for k in range(1, n + 1):
        for rest in compositions(n - k):
            yield (k,) + rest


EDGE_B = 65                                   # one image past a 64-thread workgroup
# (rule, with s2, weight)
EDGE_RULES = [("relative", False, 1.0), ("weighted", False, 1.0), ("weighted", True, 0.5), ("max", False, 1.0), ("min", False, 1.0)]
EDGE_GAP = 1e-6                               # relative lead of the float64 winner; the kernels compare the float32 tables exactly, in f64


def edge_tables(N):
    """(s1 (65,N), s2 (65,N), {row: 'tie'}) float32.  At N = 64 the first row and the one past the workgroup carry a bit-equal best score
    twice, for every rule: the largest and the smallest s1, and the largest s2 at the indices of the largest s1."""
    g = R.gen(450 + N)
    s1 = torch.rand(EDGE_B, N, generator=g) * 10 + 15
    s2 = torch.rand(EDGE_B, N, generator=g) * 0.3 + 0.6
    ties = {}
    if N > 1:
        for b in (0, EDGE_B - 1):
            s1[b, 3] = s1[b, 40] = 26.0
            s2[b, 3] = s2[b, 40] = 0.95
            s1[b, 7] = s1[b, 50] = 14.0
            ties[b] = "tie"
    return s1, s2, ties


def edge_scores(rule, s1_row, s2_row, weight):
    """What the rule compares, larger = better, float64 (R.ranked; 'relative' is the weighted rule of one score)."""
    return R.ranked(s1_row, s2_row, weight, "weighted" if rule == "relative" else rule)


def edge_reference(rule, s1_row, s2_row, weight):
    return R.select_best(s1_row) if rule == "relative" else R.select_scores(s1_row, s2_row, weight, rule)
