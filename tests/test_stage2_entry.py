"""GPU: how the candidates enter the two Stage-II U-Nets of DecompDualBranchDDWavelet.

* ``ops.conv2d(..., res1_rep=n)``: one residual row shared by n output rows, in the row-form, tap-form, f32-MFMA and direct kernels.
* ``forward_decomposed``: first_conv as the per-image half (once per image) plus the per-sample half with the former as its residual,
  against the concatenated form (explicit q by cat / repeat_interleave) in float64.
* ``ops.cond_dwt``: quat_dwt(bilinear_up(conds, s)) in one kernel, bit for bit.
* ``BEMPipeline.enhance`` with the per-image work on the side stream and on the launch stream.

Tolerances are the ones the suite already holds these kernels to; each is quoted where it is used."""
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

import stage2_yardstick as Y
from oracle import bem_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as _ops
    return _ops


def dev(t):
    return t.cuda().contiguous()


def conv_close(a, b, what):
    """rtol 1e-4 / atol 2e-5: the bound of tests/test_ops_gpu.py::test_conv3x3_row_form (and test_conv2d, test_conv3x3_x6_taps) on the dense
    convolutions, here against the float64 result."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    print(f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})")
    assert torch.allclose(a, b, rtol=1e-4, atol=2e-5), f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})"


# ----------------------------------------------------------------------------- res1_rep ---
def _res1_rep_case(ops, H, W, what, route):
    B, rep, Ci, Co = 6, 3, 16, 40
    g = torch.Generator().manual_seed(H * W)
    x, w, b = torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, 3, 3, generator=g) * (Ci * 9) ** -0.5, torch.randn(Co, generator=g)
    r1, r2 = torch.randn(B // rep, Co, H, W, generator=g), torch.randn(B, Co, H, W, generator=g)
    y64 = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    r1x = r1.double().repeat_interleave(rep, 0)
    xd, wd, bd, r1d, r2d = dev(x), dev(w), dev(b), dev(r1), dev(r2)
    assert ops.conv2d_route(xd, wd, pad=1, res1=r1d, res1_rep=rep) == route
    conv_close(ops.conv2d(xd, wd, bd, pad=1, res1=r1d, res1_rep=rep), y64 + r1x, f"{what}: res1_rep {rep}")
    conv_close(ops.conv2d(xd, wd, bd, pad=1, relu=True, res1=r1d, res2=r2d, res1_rep=rep), F.relu(y64) + r1x + r2.double(),
               f"{what}: relu + res1_rep {rep} + res2")
    conv_close(ops.conv2d(xd, wd, None, pad=1, res1=r1d, res1_rep=rep), F.conv2d(x.double(), w.double(), None, padding=1) + r1x,
               f"{what}: no bias, res1_rep {rep}")
    # res1_rep = 1 is the call without the argument, to the bit
    full = dev(r1x.float())
    for kw in (dict(), dict(relu=True, res2=r2d)):
        assert torch.equal(ops.conv2d(xd, wd, bd, pad=1, res1=full, res1_rep=1, **kw), ops.conv2d(xd, wd, bd, pad=1, res1=full, **kw)), what
    with pytest.raises(ValueError):
        ops.conv2d(xd, wd, bd, pad=1, res1=r1d)                       # B / 3 rows without res1_rep
    with pytest.raises(ValueError):
        ops.conv2d(xd, wd, bd, pad=1, res1=r1d, res1_rep=2)           # 6 / 2 != 2 rows


def test_res1_rep_row_form(ops):
    """B = 6 rows share 2 residual rows (res1_rep = 3), 16 -> 40 channels at 32x32: the row-form kernel (one k-block, two row blocks of
    output channels)."""
    _res1_rep_case(ops, 32, 32, "row form 32x32", "rows")


@pytest.mark.parametrize("kernel", ["taps", "mfma", "direct"])
def test_res1_rep_other_kernels(ops, kernel, monkeypatch):
    """24x40 is outside the row form (W no power of two): the nine-tap x6 kernel takes it; with that switched off the f32-MFMA
    implicit GEMM, and with both off the direct kernel."""
    if kernel != "taps":
        monkeypatch.setattr(ops, "USE_CONV_X6", False)
    if kernel == "direct":
        monkeypatch.setattr(ops, "USE_CONV_MFMA", False)
    _res1_rep_case(ops, 24, 40, f"{kernel} 24x40", kernel)


# ----------------------------------------------------------------------------- split first_conv ---
NAME = "DecompDualBranchDDWavelet"


def _yardstick(out, r32, r64, what):
    """tests/test_modules_gpu.py::_yardstick, the Stage-II float64 parity bound of the suite: HIP no further from float64 than 2x the f32
    oracle, mean and max."""
    (rm, rM), (hm, hM) = Y.errors(r32, r64), Y.errors(out, r64)
    print(f"{what} vs float64: f32 oracle mean {rm:.3e} max {rM:.3e} | HIP mean {hm:.3e} max {hM:.3e} ({hm / rm:.2f}x, {hM / rM:.2f}x)")
    assert torch.isfinite(out).all()
    assert hm <= 2 * rm and hM <= 2 * rM, (what, hm, rm, hM, rM)


def _oracle_from_decomposed(sd, d_img_rows, d_cond, dtype):
    """The oracle's DecompDualBranchDDWavelet forward (q = cat(Q_img, Q_cond) per branch, first_conv on it) on given decompositions:
    decomp_wavelet_ref is answered with the halves [Q1_w | Q2_w] of d_img_rows (already one row per sample), then of d_cond."""
    halves = iter([(d_img_rows[:, :16].to(dtype), d_img_rows[:, 16:].to(dtype)), (d_cond[:, :16].to(dtype), d_cond[:, 16:].to(dtype))])
    x = torch.zeros(d_cond.shape[0], 6, 2 * d_cond.shape[2], 2 * d_cond.shape[3])
    with mock.patch.object(O, "decomp_wavelet_ref", lambda *a, **k: next(halves)):
        if dtype == torch.float64:
            return Y.float64_ref(NAME, sd, x)
        return Y.oracle(NAME, sd, x, O.selective_scan_c)


@pytest.fixture(scope="module")
def split_case(ops):
    """The net (n_feat 8, [1,1,1]), the decompositions of Bi = 2 images and of 6 conditions at 64x64 (32x32 wavelet planes), made once."""
    net = Y.build_arch(NAME, n_feat=8, num_blocks=(1, 1, 1), seed=3).cuda().eval()
    g = torch.Generator().manual_seed(17)
    img, cond = 0.25 * torch.rand(2, 3, 64, 64, generator=g), torch.rand(6, 3, 64, 64, generator=g)
    with torch.no_grad():
        d_img, d_cond = net.decompose(dev(img), 0), net.decompose(dev(cond), 0)
    return net, d_img, d_cond


def _run_split(net, d_img, d_cond, spi):
    """forward_decomposed and what its two first_conv modules returned."""
    taps, hooks = {}, []
    for br in ("_Q1", "_Q2"):
        hooks.append(getattr(net, "first_conv" + br).register_forward_hook(lambda m, a, o, br=br: taps.__setitem__(br, o.detach().cpu())))
    try:
        with torch.no_grad():
            out = net.forward_decomposed(d_img, d_cond, None if spi == 1 else spi)
    finally:
        for h in hooks:
            h.remove()
    return out.cpu(), taps


def _check_split(net, d_img, d_cond, spi, what, end_to_end=True):
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    rows = d_img.cpu().repeat_interleave(spi, 0)
    out, taps = _run_split(net, d_img, d_cond, spi)
    for bi, br in enumerate(("_Q1", "_Q2")):
        q = torch.cat([rows[:, 16 * bi:16 * bi + 16], d_cond.cpu()[:, 16 * bi:16 * bi + 16]], 1)          # the concatenated input, explicitly
        ref = F.conv2d(q.double(), sd[f"first_conv{br}.weight"].double(), sd[f"first_conv{br}.bias"].double(), padding=1)
        conv_close(taps[br], ref, f"{what}: first_conv{br}")
    if end_to_end:
        _yardstick(out, _oracle_from_decomposed(sd, rows, d_cond.cpu(), torch.float32), _oracle_from_decomposed(sd, rows, d_cond.cpu(), torch.float64), what)
    return out


def test_split_first_conv_three_samples_per_image(split_case):
    """Bi = 2 images x 3 samples (no power of two): at the first_conv outputs against the concatenated form in float64 (dense-conv bound),
    end to end against the float64 oracle on the same decompositions (Stage-II parity bound)."""
    net, d_img, d_cond = split_case
    _check_split(net, d_img, d_cond, 3, "2 images x 3 samples")


def test_split_first_conv_one_sample_per_image(split_case):
    """img_index=None: one image row per condition row (res1_rep = 1)."""
    net, d_img, d_cond = split_case
    _check_split(net, d_img.repeat_interleave(3, 0).contiguous(), d_cond, 1, "6 images x 1 sample")


def test_split_first_conv_follows_a_weight_update(split_case):
    """The sliced and packed halves of first_conv are cached per weight version: after an in-place change of the weight (both halves) and
    of the bias the first_conv output is the new layer's."""
    net, d_img, d_cond = split_case
    before = _check_split(net, d_img, d_cond, 3, "before the update", end_to_end=False)
    with torch.no_grad():
        net.first_conv_Q1.weight.mul_(1.5)
        net.first_conv_Q1.weight[:, :16].add_(0.01)
        net.first_conv_Q1.bias.add_(0.1)
    try:
        after = _check_split(net, d_img, d_cond, 3, "after the update", end_to_end=False)
        assert float((after - before).abs().max()) > 1e-3
    finally:
        with torch.no_grad():
            net.first_conv_Q1.bias.sub_(0.1)
            net.first_conv_Q1.weight[:, :16].sub_(0.01)
            net.first_conv_Q1.weight.div_(1.5)


# ----------------------------------------------------------------------------- cond_dwt ---
@pytest.mark.parametrize("shape,s", [((5, 3, 4, 4), 16), ((2, 3, 16, 16), 16), ((3, 3, 6, 10), 2)])
def test_cond_dwt_is_the_chain_bit_for_bit(ops, shape, s):
    """ops.cond_dwt against quat_dwt(bilinear_up(conds, s)): 16-byte stores (output rows of 32 / 128 pixels) and the scalar form (10), every
    edge clamp of the interpolation in the s = 2 case; values around 0 .. 1 like the conditions, with negative ones (noise) among them."""
    g = torch.Generator().manual_seed(shape[0] * 100 + s)
    conds = dev(torch.rand(shape, generator=g) * 1.2 - 0.1)
    want = ops.quat_dwt(ops.bilinear_up(conds, s))
    got = ops.cond_dwt(conds, s)
    assert got.shape == want.shape == (shape[0], 32, shape[2] * s // 2, shape[3] * s // 2)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), float((got - want).abs().max())


def test_cond_dwt_rejects_odd_sizes(ops):
    with pytest.raises(ValueError):
        ops.cond_dwt(dev(torch.rand(1, 3, 3, 4)), 1)
    with pytest.raises(ValueError):
        ops.cond_dwt(dev(torch.rand(1, 4, 4, 4)), 2)


# ----------------------------------------------------------------------------- pipeline ---
def test_pipeline_same_result_on_one_and_two_streams(monkeypatch):
    """BEMPipeline.enhance, 2 images x 3 samples at 64x64, fixed seed: the per-image work (decomp(image), the image halves of the two first
    convs) on the side stream and on the launch stream.  The same selection; PSNRs within 1e-4 dB, the bound of
    tests/test_modules_gpu.py::test_bench_step_reproducible_under_full_load between runs of one step."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem.modules import SampleCtx
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, net2 = build_nets(n_feat=16, num_blocks=(1, 1, 1), device="cuda")
    pipe = BEMPipeline(net1, net2, 16, 0.1)
    lq, gt = synthetic_pair((2, 3, 64, 64), seed=21, device="cuda")
    runs = {}
    for mode in ("1", "0", "1"):
        monkeypatch.setenv("BEM_DECOMP_OVERLAP", mode)
        SampleCtx._epoch = 91000                       # the forward counter keys the Philox streams: the runs draw the same weights and noise
        r = pipe.enhance(lq, gt, 3, gt_mean=True, seed=77)
        runs.setdefault(mode, []).append((r["best"], r["psnr"].cpu(), r["final"].cpu()))
    (b1, p1, f1), (b0, p0, f0) = runs["1"][0], runs["0"][0]
    assert torch.isfinite(f1).all() and p1.shape == (6,)
    assert b1 == b0 == runs["1"][1][0]
    for p, f in ((p0, f0), runs["1"][1][1:]):
        print(f"max |d psnr| {float((p - p1).abs().max()):.2e} dB, max |d final| {float((f - f1).abs().max()):.2e}")
        assert float((p - p1).abs().max()) <= 1e-4
