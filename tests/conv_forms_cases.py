"""Case tables, float64 reference, f32 yardstick and mutant references shared by tests/test_conv_forms_gpu.py and tests/test_conv_forms_cpu.py
(not collected by pytest): the dense convolution's kernel forms at the instantiations no other test runs by value.  The CPU tests check, on
these very tables, what the GPU tests rely on: that every case is routed to the form it names, that the tables together reach every
instantiation of the two dispatch ladders, and that the per-element bound of the GPU tests would notice each of the mutants below.

A case is (B, Cin, Cout, H, W, K, stride, pad, dilation, switches, want_form, extras):
  switches   (USE_CONV_X6, USE_CONV_MFMA), the values the GPU test puts on bem.ops before it asks for the route
  want_form  "taps", "mfma" or "direct"
  extras     {"relu": True, "bias": False, "res1": True, "res2": True, "res1_rep": n, "cin_slice": (c0, Ct)}, each optional; the bias is there unless
             "bias" is False; cin_slice = (first channel, channels of the wider tensor the Cin channels are a slice of)"""
import zlib

import torch
import torch.nn.functional as F

RTOL, ATOL = 1e-4, 2e-5      # tests/test_stage2_entry.py::conv_close, the bound the suite holds all four forms to against float64
ON, NO_X6, OFF = (True, True), (False, True), (False, False)
RR = {"relu": True, "res1": True, "res2": True}


def _c(shape, ksp, switches, form, **extras):
    return tuple(shape) + tuple(ksp) + (switches, form, extras)


S1D2, S2P1 = (3, 1, 2, 2), (3, 2, 1, 1)
# (B, Cin, Cout, H, W) and the edge the case exists for
FAMILIES = {
    # conv_taps_x6_kernel<*, 3, 3, 1> with dilation 2 (QD model2's branch_q1 / q2[2]): W even, Cin % 8 == 0
    "taps_dil2": [
        _c((2, 32, 32, 16, 16), S1D2, ON, "taps", res1=True),                    # model2's branch call: one M-tile, Lo = 256 = one workgroup
        _c((1, 8, 7, 2, 4), S1D2, ON, "taps"),                                   # plane smaller than the 5x5 window, one partly live wave, half k-block, odd Cout
        _c((1, 24, 70, 17, 20), S1D2, ON, "taps", **RR),                         # Cin % 16 == 8 in two k-blocks, 3 M-tiles on MTW 2 (last masked), Lo = 340
        _c((6, 16, 40, 1, 6), S1D2, ON, "taps", res1=True, res1_rep=3),          # H = 1: both outer tap rows outside for every pixel
        _c((1, 16, 33, 5, 130), S1D2, ON, "taps", bias=False),                   # rows longer than two waves: pixel pairs across wave boundaries
        _c((1, 16, 40, 6, 10), S1D2, ON, "taps", cin_slice=(8, 32)),
    ],
    # conv_taps_x6_kernel<*, 3, 3, 2> (model2's down_conv): Wo even
    "taps_s2": [
        _c((2, 32, 32, 16, 16), S2P1, ON, "taps"),                               # down_conv
        _c((1, 8, 33, 5, 7), S2P1, ON, "taps"),                                  # odd H and W: the last tap column on / past the edge
        _c((1, 24, 70, 9, 12), S2P1, ON, "taps", **RR),
        _c((1, 16, 16, 2, 3), S2P1, ON, "taps", bias=False),                     # 1x2 output
        _c((1, 40, 96, 33, 64), S2P1, ON, "taps", res1=True),                    # 17x32 outputs, three workgroups
        _c((4, 16, 40, 6, 8), S2P1, ON, "taps", res1=True, res1_rep=2, cin_slice=(8, 32)),
    ],
    # conv2d_mfma_pipe_kernel<3,3,1,1|2>, conv2d_mfma_kernel<3,3,1,3|5> and <4,4,2,1|2|3|5>: 8 x 32 output tiles, chunks of 8 input channels.
    # Odd W or Cin % 8 != 0 keeps the x6 forms away, else USE_CONV_X6 = False.  Output planes of 9x33 (two tiles each way, the second one row /
    # column wide) and of 8x32 exactly; M-tiles 1, 2, 3, 4, 4, 5 (4 M-tiles run on the MTW = 5 instantiation)
    "mfma": [
        _c((1, 3, 16, 9, 33), (3, 1, 1, 1), ON, "mfma", **RR),                   # Cin 3: K = 27, the last k-step half empty
        _c((1, 16, 16, 10, 34), (3, 1, 0, 1), NO_X6, "mfma"),                    # pad 0 -> 8x32
        _c((2, 16, 16, 5, 9), (3, 1, 2, 1), ON, "mfma", bias=False),             # pad 2 -> 7x11
        _c((1, 11, 40, 8, 32), (3, 1, 1, 1), ON, "mfma", **RR),                  # Cin 11: the second chunk partial
        _c((1, 3, 40, 11, 35), (3, 1, 0, 1), ON, "mfma"),                        # pad 0 -> 9x33
        _c((6, 11, 40, 5, 33), (3, 1, 1, 1), ON, "mfma", res1=True, res1_rep=3),
        _c((1, 16, 70, 9, 33), (3, 1, 1, 1), ON, "mfma", **RR),
        _c((1, 11, 70, 7, 31), (3, 1, 2, 1), ON, "mfma"),                        # pad 2 -> 9x33
        _c((1, 11, 100, 9, 33), (3, 1, 1, 1), ON, "mfma", **RR),                 # 4 M-tiles on MTW 5
        _c((1, 16, 128, 8, 32), (3, 1, 1, 1), NO_X6, "mfma"),                    # 4 full M-tiles
        _c((1, 3, 130, 9, 33), (3, 1, 1, 1), ON, "mfma", cin_slice=(2, 6)),      # 5 M-tiles, the last two rows high
        _c((1, 8, 24, 18, 66), (4, 2, 1, 1), ON, "mfma"),                        # 9x33 outputs (Wo no power of two: not the row form)
        _c((1, 3, 24, 18, 66), (4, 2, 0, 1), ON, "mfma", **RR),                  # pad 0 -> 8x32
        _c((1, 24, 48, 19, 67), (4, 2, 0, 1), ON, "mfma", **RR),                 # pad 0, last row and column of the plane unread -> 8x32
        _c((4, 8, 48, 6, 10), (4, 2, 1, 1), ON, "mfma", res1=True, res1_rep=2),
        _c((2, 11, 80, 9, 13), (4, 2, 1, 1), ON, "mfma", **RR),
        _c((1, 16, 128, 14, 62), (4, 2, 2, 1), ON, "mfma", **RR),                # pad 2 -> 8x32, 4 M-tiles on MTW 5
        _c((1, 8, 160, 17, 65), (4, 2, 2, 1), ON, "mfma", bias=False),           # pad 2 -> 9x33, 5 M-tiles
    ],
    # conv2d_kernel<3,3,1>, <4,4,2>, <5,5,1>: 16 output channels per workgroup; both switches off, or Cout > 160, or 5x5 at an odd width
    "direct": [
        _c((1, 11, 7, 9, 33), (3, 1, 1, 1), OFF, "direct"),
        _c((1, 16, 16, 8, 32), (3, 1, 1, 1), OFF, "direct", bias=False),
        _c((1, 3, 17, 10, 34), (3, 1, 0, 1), OFF, "direct", **RR),               # pad 0 -> 8x32
        _c((1, 8, 168, 7, 31), (3, 1, 2, 1), ON, "direct"),                      # pad 2 -> 9x33; Cout > 160
        _c((1, 8, 7, 18, 66), (4, 2, 1, 1), OFF, "direct"),                      # 9x33
        _c((1, 11, 16, 18, 66), (4, 2, 0, 1), OFF, "direct"),                    # pad 0 -> 8x32
        _c((4, 16, 17, 14, 62), (4, 2, 2, 1), OFF, "direct", relu=True, res1=True, res2=True, res1_rep=2),      # pad 2 -> 8x32
        _c((1, 3, 168, 17, 65), (4, 2, 2, 1), ON, "direct", cin_slice=(1, 5)),   # pad 2 -> 9x33; Cout > 160
        _c((2, 8, 20, 7, 7), (5, 1, 2, 1), ON, "direct", **RR),
        _c((1, 24, 33, 3, 3), (5, 1, 2, 1), ON, "direct"),                       # plane smaller than the window
    ],
}
CASES = [(fam, i) for fam, cs in FAMILIES.items() for i in range(len(cs))]
MAX_OUT_ELEMS = 72000


def case_id(fam, i):
    B, Ci, Co, H, W, K, s, p, d, sw, form, ex = FAMILIES[fam][i]
    return f"{fam}-{B}x{Ci}x{Co}x{H}x{W}-k{K}s{s}p{p}d{d}" + "".join(f"-{'nobias' if k == 'bias' else k}" for k in sorted(ex))


def out_hw(case):
    B, Ci, Co, H, W, K, s, p, d = case[:9]
    return (H + 2 * p - d * (K - 1) - 1) // s + 1, (W + 2 * p - d * (K - 1) - 1) // s + 1


def reads_last(n, K, s, p, d):
    """Whether some output position's window holds input index n - 1 of an axis of n."""
    no = (n + 2 * p - d * (K - 1) - 1) // s + 1
    return any(o * s - p + k * d == n - 1 for o in range(no) for k in range(K))


def inputs(case):
    """The existing convention (tests/test_ops_gpu.py::test_conv2d): randn x, w * (Cin K K)^-1/2, randn bias and residuals, one seeded
    generator per case.  x has the channels of the wider tensor where the case has a cin_slice."""
    B, Ci, Co, H, W, K, s, p, d, sw, form, ex = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case[:9]).encode()))
    Ho, Wo = out_hw(case)
    rep = ex.get("res1_rep", 1)
    return {
        "x": torch.randn(B, ex["cin_slice"][1] if "cin_slice" in ex else Ci, H, W, generator=g),
        "w": torch.randn(Co, Ci, K, K, generator=g) * (Ci * K * K) ** -0.5,
        "bias": torch.randn(Co, generator=g) if ex.get("bias", True) else None,
        "res1": torch.randn(B // rep, Co, Ho, Wo, generator=g) if ex.get("res1") else None,
        "res2": torch.randn(B, Co, Ho, Wo, generator=g) if ex.get("res2") else None,
    }


# mutant -> what a kernel with that mistake would compute
MUTANTS = ["dilation_one_axis", "pad_off_by_one", "last_col_zero", "last_row_zero", "kykx_swapped", "res1_row_b", "bias_last_dropped"]


def mutant_applies(mutant, case):
    B, Ci, Co, H, W, K, s, p, d, sw, form, ex = case
    return {"dilation_one_axis": d != 1, "last_col_zero": reads_last(W, K, s, p, d), "last_row_zero": reads_last(H, K, s, p, d),
            "res1_row_b": ex.get("res1_rep", 1) > 1, "bias_last_dropped": ex.get("bias", True)}.get(mutant, True)


def reference(case, inp, dtype=torch.float64, mutant=None):
    """relu?(conv2d(x[:, slice], w) + bias) + res1[b // rep] + res2 by F.conv2d in `dtype`: float64 is the reference, float32 the yardstick."""
    B, Ci, Co, H, W, K, s, p, d, sw, form, ex = case
    c0 = ex["cin_slice"][0] if "cin_slice" in ex else 0
    x, w = inp["x"][:, c0:c0 + Ci].to(dtype), inp["w"].to(dtype)
    bias = None if inp["bias"] is None else inp["bias"].to(dtype)
    pad, dil = (p, p), (d, d)
    if mutant == "dilation_one_axis":
        pad, dil = (p, p - (d - 1) * (K - 1) // 2), (d, 1)        # the same output size
    elif mutant == "pad_off_by_one":
        x, pad = F.pad(x, (p + 1, p - 1, p + 1, p - 1)), (0, 0)    # the windows one up and one left
    elif mutant == "last_col_zero":
        x = x.clone()
        x[..., -1] = 0
    elif mutant == "last_row_zero":
        x = x.clone()
        x[..., -1, :] = 0
    elif mutant == "kykx_swapped":
        w = w.transpose(2, 3)
    elif mutant == "bias_last_dropped":
        bias = bias.clone()
        bias[-1] = 0
    y = F.conv2d(x, w, bias, stride=s, padding=pad, dilation=dil)
    if ex.get("relu"):
        y = F.relu(y)
    if inp["res1"] is not None:
        rep, r1 = ex.get("res1_rep", 1), inp["res1"].to(dtype)
        y = y + (r1[torch.arange(B) % (B // rep)] if mutant == "res1_row_b" else r1.repeat_interleave(rep, 0))
    if inp["res2"] is not None:
        y = y + inp["res2"].to(dtype)
    return y


def excess(a, ref):
    """max over the elements of |a - ref| / (ATOL + RTOL |ref|): above 1 breaks the per-element bound."""
    return float(((a.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max())


# --- the two dispatch ladders of csrc (conv_patch_launch in conv.hip, conv_taps_launch in conv_x6.hip), restated ---
def instantiation(case):
    B, Ci, Co, H, W, K, s, p, d, sw, form, ex = case
    MT = -(-Co // 32)
    if form == "direct":
        return f"conv2d_kernel<{K},{K},{s}>"
    if form == "mfma":
        if (K, s) == (3, 1) and MT <= 2:
            return f"conv2d_mfma_pipe_kernel<3,3,1,{MT}>"
        return f"conv2d_mfma_kernel<{K},{K},{s},{MT if MT <= 3 else 5}>"
    assert form == "taps"
    return f"conv_taps_x6_kernel<{1 if MT == 1 else 2},{K},{K},{s}>" + (" dilation 2" if d == 2 else "")


# every instantiation the two ladders dispatch, but the dilation-1 3x3 and the 5x5 taps (tests/test_ops_gpu.py::test_conv3x3_x6_taps, tests/test_lpips_gpu.py)
INSTANTIATIONS = ({f"conv2d_kernel<{k},{k},{s}>" for k, s in ((3, 1), (4, 2), (5, 1))} |
                  {f"conv2d_mfma_pipe_kernel<3,3,1,{m}>" for m in (1, 2)} | {f"conv2d_mfma_kernel<3,3,1,{m}>" for m in (3, 5)} |
                  {f"conv2d_mfma_kernel<4,4,2,{m}>" for m in (1, 2, 3, 5)} |
                  {f"conv_taps_x6_kernel<{m},3,3,1> dilation 2" for m in (1, 2)} | {f"conv_taps_x6_kernel<{m},3,3,2>" for m in (1, 2)})
