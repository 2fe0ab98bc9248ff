"""GPU: the launch bracket of bem.ops (ops._bracket, profile_start / profile_stop), one case per profile key.

Each case issues a few calls at the smallest shapes on both sides of the key's predicate, once plainly and once inside the bracket, and
holds profile_stop()'s launches / bytes / flops to literal numbers (host arithmetic on the shapes; x6-packed weights hold
ceil(M / 32) * ceil(K / 16) * 768 floats).  Every tensor an op returns must be bit-equal with the bracket on and off.
(conv2d's key: test_derived_cache_gpu.py::test_profiled_conv_takes_a_prepared_weight.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as _ops
    return _ops


def rnd(seed, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).cuda()


def pw_calls(ops):
    """pw_gemm on an (1,8,4,6) plane with W (16,8); the same summing a second input (in_mode 1); an odd plane (1,8,3,5) with a residual."""
    W = ops.pack_pw_weight(rnd(1, 16, 8))
    x, x2, xo = rnd(2, 1, 8, 4, 6), rnd(3, 1, 8, 4, 6), rnd(4, 1, 8, 3, 5)
    return [ops.pw_gemm(x, W, 16), ops.pw_gemm(x, W, 16, x2=x2, in_mode=1), ops.pw_gemm(xo, W, 16, res=rnd(5, 1, 16, 3, 5))]


def stream_calls(ops):
    """K = 56 > 48: W (40,56) plain; the same behind a LayerNorm; W (32,56), M no more than 32."""
    x = rnd(6, 1, 56, 4, 6)
    W40, W32 = ops.pack_pw_weight(rnd(7, 40, 56, scale=0.1)), ops.pack_pw_weight(rnd(8, 32, 56, scale=0.1))
    ln = (rnd(9, 56, scale=0.2, shift=1.0), rnd(10, 56, scale=0.1))
    return [ops.pw_gemm(x, W40, 40), ops.pw_gemm(x, W40, 40, ln=ln), ops.pw_gemm(x, W32, 32)]


def gdmlp_calls(ops, widths):
    """The fused gdMlp branch with Hd = 16 on a 5 x 33 plane, once per width C."""
    out, Hd = [], 16
    perm = ops.gate_interleave(Hd, "cuda")
    for C in widths:
        wi, wd, wo = rnd(C, 2 * Hd, C, scale=C ** -0.5), rnd(C + 1, 2 * Hd, 1, 3, 3, scale=1 / 3), rnd(C + 2, C, Hd, scale=0.25)
        out.append(ops.gdmlp_x6(rnd(C + 3, 1, C, 5, 33), rnd(C + 4, C, scale=0.2, shift=1.0), rnd(C + 5, C, scale=0.1), 1e-6,
                                ops.pack_pw_weight(wi[perm].contiguous()), torch.zeros(2 * Hd, device="cuda"), ops.dw_gate_params10(wd, None, Hd),
                                ops.pack_pw_weight(wo), None, Hd))
    return out


def dwconv_calls(ops):
    return [ops.dwconv3x3(rnd(11, 1, 8, 5, 7), rnd(12, 8, 1, 3, 3), rnd(13, 8), mode=2)]


def scan_operands(B, C, L, R, N, seed, flat_A):
    x0, x1 = rnd(seed, B, C, L), rnd(seed + 1, B, C, L)
    xd0, xd1 = rnd(seed + 2, B, 2, R + 2 * N, L), rnd(seed + 3, B, 2, R + 2 * N, L)
    dtw, dtb = rnd(seed + 4, 4, C, R, scale=0.3), rnd(seed + 5, 4, C, shift=-2.0)
    A = -torch.rand(4 * C, N, generator=torch.Generator().manual_seed(seed + 6)).cuda()
    return x0, x1, xd0, xd1, dtw, dtb, (A.view(-1) if flat_A else A), rnd(seed + 7, 4 * C)


def scan_calls(ops):
    """ss2d_scan at B = 1, C = 8, a 5 x 7 plane, R = 1; ss2d_scan_n (d_state 2) on the same plane belongs to no key."""
    y = ops.ss2d_scan(*scan_operands(1, 8, 35, 1, 1, 20, True))
    return list(y) + list(ops.ss2d_scan_n(*scan_operands(1, 8, 35, 1, 2, 30, False)))


def transpose_calls(ops):
    """Only the whole-tensor form counts: the slice and the into form launch the same kernel outside the key."""
    x = rnd(40, 1, 3, 5, 7)
    return [ops.transpose_planes(x), ops.transpose_plane_slice(x, 1, 2), ops.transpose_planes_into(x, torch.zeros(1, 4, 7, 5, device="cuda"), 1)]


def up_fuse_calls(ops):
    folded = ops.UpFuseWeights(ops.pack_pw_weight(rnd(41, 4, 2, 4, scale=0.5)), ops.pack_pw_weight(rnd(42, 2, 2, scale=0.5)), rnd(43, 2), 4)
    return [ops.up_fuse(rnd(44, 1, 4, 3, 5), rnd(45, 1, 2, 6, 10), folded)]


# The backward cases keep to one workgroup per accumulated address (one 32-pixel tile for the weight gradients, four channels of a
# 6 x 8 plane for the scan), where the float atomics of these kernels add in one order and the results are reproducible bit for bit.
def pw_wgrad_calls(ops):
    """dw (16, 8) from a 4 x 6 plane, then dw (16, 12) from two inputs (8 + 4 channels) with a bias gradient."""
    dy, x1, x2 = rnd(50, 1, 16, 24), rnd(51, 1, 8, 24), rnd(52, 1, 4, 24)
    return [ops.pw_wgrad_(dy, x1, torch.zeros(16, 8, device="cuda")),
            ops.pw_wgrad_(dy, x1, torch.zeros(16, 12, device="cuda"), x2=x2, dbias=torch.zeros(16, device="cuda"))]


def conv_wgrad_calls(ops):
    return [ops.conv_wgrad_(rnd(53, 1, 16, 4, 6), rnd(54, 1, 8, 4, 6), torch.zeros(16, 8, 3, 3, device="cuda"), torch.zeros(16, device="cuda"), stride=1, pad=1)]


def scan_bwd_calls(ops):
    """ss2d_scan_bwd at B = 1, C = 4, a 6 x 8 plane, R = 2; ss2d_scan_n_bwd (d_state 2) belongs to no key (and adds its x_dbl gradient
    from several workgroups: only its dx0, dx1 are compared)."""
    B, C, L, R = 1, 4, 48, 2
    z = lambda *s: torch.zeros(*s, device="cuda")
    a = scan_operands(B, C, L, R, 1, 60, True)
    out = list(ops.ss2d_scan_bwd(*a[:4], rnd(68, B, C, L), rnd(69, B, C, L), *a[4:], z(4 * C), z(4 * C), z(4, C, R), z(4, C)))
    a = scan_operands(B, C, L, R, 2, 70, False)
    return out + list(ops.ss2d_scan_n_bwd(*a[:4], rnd(78, B, C, L), rnd(79, B, C, L), *a[4:], z(4 * C, 2), z(4 * C), z(4, C, R), z(4, C)))[:2]


def dwact_bwd_calls(ops):
    return [ops.dwact_bwd(rnd(80, 1, 8, 5, 7), rnd(81, 8, 1, 3, 3), rnd(82, 8), rnd(83, 1, 4, 5, 7), torch.zeros(8, 1, 3, 3, device="cuda"),
                          torch.zeros(8, device="cuda"), 2)]


def ln_bwd_calls(ops):
    """LayerNorm2d backward on (1,8,5,7): with a residual gradient and n wanted; then of x1 + x2 without either."""
    x1, x2, dn, dres = rnd(84, 1, 8, 5, 7), rnd(85, 1, 8, 5, 7), rnd(86, 1, 8, 5, 7), rnd(87, 1, 8, 5, 7)
    gam, bet = rnd(88, 8, shift=1.0), rnd(89, 8)
    z = lambda: torch.zeros(8, device="cuda")
    a = ops.ln_bwd(x1, dn, gam, bet, 1e-5, z(), z(), dres=dres)
    b = ops.ln_bwd(x1, dn, gam, bet, 1e-5, z(), z(), x2=x2, want_n=False)
    return [a[0], a[1], b[0]]


# key -> (calls, launches, bytes, flops) as the commit before the bracket became one decorator reported them for these calls; beside each
# the formula that gives the number.  768 and 6144 are the x6-packed floats of a (16, 8) and a (40, 56) weight.
CASES = {
    # bytes = 4 B L (cin + M + M [res]) + 4 packed floats, flops = 2 M K L B, summed over the calls the key counts
    "pw_gemm": (pw_calls, 3, 16992.0,           # 4 * 24 * (8 + 16) + 4 * 24 * (16 + 16) + 4 * 15 * (8 + 16 + 16) + 3 * 4 * 768
                16128.0),                       # 2 * 16 * 8 * 24 + 2 * 16 * 8 * 24 + 2 * 16 * 8 * 15
    "pw_x6_res<3,2,1>": (pw_calls, 1, 5376.0,   # 4 * 24 * (8 + 16) + 4 * 768
                         6144.0),               # 2 * 16 * 8 * 24
    "pw_x6_stream<2>": (stream_calls, 1, 33792.0,        # 4 * 24 * (56 + 40) + 4 * 6144
                        107520.0),                       # 2 * 40 * 56 * 24
    # bytes = 8 numel(x), flops = 6 * 2 B H W (2 Hd C + Hd C)
    "gdmlp_x6<3>": (lambda ops: gdmlp_calls(ops, (40, 8)), 1, 52800.0,       # 8 * 40 * 5 * 33
                    3801600.0),                                              # 12 * 165 * 3 * 16 * 40
    "gdmlp_x6<5>": (lambda ops: gdmlp_calls(ops, (72, 40)), 1, 95040.0,      # 8 * 72 * 5 * 33
                    6842880.0),                                              # 12 * 165 * 3 * 16 * 72
    "dwconv3x3": (dwconv_calls, 1, 1680.0,      # 4 B H W (Cin + Cout) = 4 * 35 * (8 + 4)
                  5040.0),                      # 18 B Cin H W = 18 * 8 * 35
    "ss2d_scan": (scan_calls, 1, 6160.0, 0.0),  # 4 numel(x0, x1, xd0, xd1, y0, y1) = 4 * (4 * 8 * 35 + 2 * 2 * 3 * 35)
    "transpose_planes": (transpose_calls, 1, 840.0, 0.0),        # 8 numel(x) = 8 * 3 * 35
    "up_fuse": (up_fuse_calls, 1, 16560.0,      # 4 (numel f + 2 numel skip + numel Wc + numel Wf2) = 4 * (60 + 2 * 120 + 4 * 768 + 768)
                1440.0),                        # 2 numel(skip) (Cin + Cin / 2) = 2 * 120 * (4 + 2)
    "pw_wgrad": (pw_wgrad_calls, 2, 6272.0,     # 4 B L (M + K) + 4 M K = 4 * 24 * (16 + 8) + 4 * 16 * 8 + 4 * 24 * (16 + 12) + 4 * 16 * 12
                 15360.0),                      # 2 M K B L = 2 * 16 * 8 * 24 + 2 * 16 * 12 * 24
    "conv_wgrad": (conv_wgrad_calls, 1, 6912.0,     # 4 (numel dy + B Cin H W) + 4 numel dw = 4 * (16 * 24 + 8 * 24) + 4 * 16 * 8 * 9
                   55296.0),                        # 2 numel(dy) Cin KH KW = 2 * 16 * 24 * 8 * 9
    "ss2d_scan_bwd": (scan_bwd_calls, 1, 10752.0, 0.0),          # 4 (6 numel x0 + 4 numel xd0) = 4 * (6 * 4 * 48 + 4 * 2 * 4 * 48)
    "dwact_bwd": (dwact_bwd_calls, 1, 2800.0,   # 4 (2 numel t + numel dout) = 4 * (2 * 280 + 140)
                  11200.0),                     # 40 numel t = 40 * 280
    "ln_bwd": (ln_bwd_calls, 2, 10080.0, 0.0),  # 4 numel(x1) (3 + [x2] + [dres] + [n wanted]) = 4 * 280 * (3 + 1 + 1) + 4 * 280 * (3 + 1)
}


def test_every_key_but_conv2d_has_a_case(ops):
    assert set(CASES) == set(ops._KEYS) - {"conv2d"}


@pytest.mark.parametrize("key", sorted(CASES))
def test_bracket_counts_and_leaves_results_alone(ops, key):
    calls, launches, nbytes, nflops = CASES[key]
    plain = calls(ops)
    ops.profile_start(key)
    try:
        timed = calls(ops)
    finally:
        rec = ops.profile_stop()
    assert ops._PROF is None
    assert (rec["launches"], rec["bytes"], rec["flops"]) == (launches, nbytes, nflops)
    assert rec["kernel"] == ops._KEYS[key][2] and rec["bound"] == ops._KEYS[key][1]
    assert len(plain) == len(timed) and all(torch.equal(a, b) for a, b in zip(plain, timed))
