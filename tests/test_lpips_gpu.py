"""LPIPS (v0.1, AlexNet) on the GPU against the float64 torch-CPU restatement tests/lpips_ref.py on seeded weights: each kernel of
csrc/lpips.hip, every convolution route the metric takes (even and odd widths), the whole metric, and the two drivers.

Bounds.  Convolutions: 1e-5 of the output's maximum, the bound of the VGG19 feature pass, same kernels.  Head: 1e-6
relative (it computes in f64 from f32 features; what is left is the f32 rounding of the result).  Whole metric: 1e-5 relative to the
float64 value; the f32 torch evaluation of the restatement is within 7e-7 on these cases, so the inputs leave more than 10x headroom."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sds():
    return R.seeded_state_dicts(0)


@pytest.fixture(scope="module")
def metric(sds):
    from bem.lpips import LPIPS
    return LPIPS(state_dict=sds[0], lin_state_dict=sds[1]).cuda()


def unblock(xs, H, W):
    """(R,48,Hb,Wb) block form of ops.lpips_prep -> the planar (R,3,H,W) image it holds, and whether everything around it is zero."""
    Rn, _, Hb, Wb = xs.shape
    full = xs.reshape(Rn, 3, 4, 4, Hb, Wb).permute(0, 1, 4, 2, 5, 3).reshape(Rn, 3, 4 * Hb, 4 * Wb)
    inner = full[:, :, 2:2 + H, 2:2 + W]
    return inner, float(full.abs().sum()) == float(inner.abs().sum())


# ------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("H,W", [(31, 31), (37, 53)])
def test_prep(H, W):
    from bem import ops
    rng = np.random.default_rng(H)
    x = rng.uniform(-0.2, 1.2, (2, 2, 3, H, W)).astype(np.float32)                 # values below 0 and above 1
    ks = np.array([k for k in range(255) if float(np.float32((k + 0.5) / 255) * np.float32(255)) == k + 0.5])
    assert ks.size > 20                                                             # x * 255 exactly at .5: half goes to even
    halves, n = ((ks + 0.5) / 255).astype(np.float32), min(ks.size, W)
    x[0, 0, 0, 0, :n], x[1, 1, 2, H - 1, :n] = halves[:n], halves[-n:]
    xs = ops.lpips_prep(torch.from_numpy(x[0]).cuda(), torch.from_numpy(x[1]).cuda()).cpu()
    Ho, Wo = R.sizes(H)[0], R.sizes(W)[0]
    assert xs.shape == (4, 48, Ho + 2, (Wo + 3) // 2 * 2)
    got, rest_zero = unblock(xs, H, W)
    assert rest_zero
    got = got.numpy()
    u = np.rint(np.clip(x.reshape(4, 3, H, W), 0, 1) * np.float32(255))
    shift, scale = np.float32(R.SHIFT).reshape(1, 3, 1, 1), np.float32(R.SCALE).reshape(1, 3, 1, 1)
    want = ((u / np.float32(127.5) - np.float32(1)) - shift) / scale
    assert want.dtype == np.float32
    back = np.rint((got.astype(np.float64) * scale + shift + 1) * 127.5)            # the integers the kernel quantised to
    assert np.array_equal(back, u)
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))
    # the unquantised modes: [-1,1] as given, and 2 x - 1
    t = torch.from_numpy(x[0] * 2 - 1).cuda()
    a, _ = unblock(ops.lpips_prep(t, t, quantise=False).cpu(), H, W)
    b, _ = unblock(ops.lpips_prep(torch.from_numpy(x[0]).cuda(), torch.from_numpy(x[0]).cuda(), quantise=False, normalize=True).cpu(), H, W)
    want = (np.concatenate([x[0], x[0]]) * 2 - 1 - shift) / scale
    assert np.all(np.abs(a.numpy() - want) <= np.spacing(np.abs(want))) and torch.equal(a, b)


@pytest.mark.parametrize("H,W", [(3, 3), (7, 7), (8, 12), (9, 10), (49, 74)])
def test_maxpool3s2(H, W):
    from bem import ops
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, 3, H, W, generator=g)
    x[1, 1, H // 2, W // 2] = float("nan")
    want = F.max_pool2d(x, 3, 2)
    got = ops.maxpool3s2(x.cuda()).cpu()
    assert got.shape == want.shape and bool(torch.isnan(want).any())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # a crop of a wider tensor, as conv1's output is read
    big = torch.randn(2, 3, H + 3, W + 5, generator=g)
    crop = big.cuda()[:, :, 1:1 + H, 2:2 + W]
    assert torch.equal(ops.maxpool3s2(crop).cpu(), F.max_pool2d(big[:, :, 1:1 + H, 2:2 + W], 3, 2))


def _conv_check(got, x64, w, b, **kw):
    want = torch.relu(F.conv2d(x64, w.double(), b.double(), **kw))
    assert got.shape == want.shape
    err, top = float((got.cpu().double() - want).abs().max()), float(want.max())
    print(f"conv {tuple(w.shape)} on {tuple(x64.shape)}: max err {err:.3e}, max {top:.3e}, ratio {err / top:.2e}")
    assert top > 0 and err <= 1e-5 * top


@pytest.mark.parametrize("H,W", [(31, 31), (37, 53), (37, 57), (64, 66)])
def test_conv1(sds, H, W):
    """11x11 stride 4 pad 2 as the 3x3 block convolution on the x6 path; output widths 7, 12, 13, 15."""
    from bem import ops
    from bem.lpips import conv1_block_weight
    w, b = sds[0]["features.0.weight"], sds[0]["features.0.bias"]
    g = torch.Generator().manual_seed(H + W)
    x = (torch.rand(2, 3, H, W, generator=g) * 2 - 1).cuda()
    xs = ops.lpips_prep(x[:1].contiguous(), x[1:].contiguous(), quantise=False)
    planar, _ = unblock(xs.cpu(), H, W)                                              # the f32 scaled image the convolution reads
    Ho, Wo = R.sizes(H)[0], R.sizes(W)[0]
    got = ops.conv2d(xs, ops.ConvWeight(conv1_block_weight(w.cuda())), b.cuda(), pad=1, relu=True)[:, :, 1:1 + Ho, 1:1 + Wo]
    _conv_check(got, planar.double(), w, b, stride=4, padding=2)


@pytest.mark.parametrize("H,W", [(3, 3), (7, 7), (8, 13), (12, 74), (4, 6)])
def test_conv2(sds, H, W):
    """5x5 pad 2, 64 -> 192: 25 shifted taps on the x6 path at even widths, the direct kernel at odd ones; 3x3 is smaller than the window."""
    from bem import ops
    w, b = sds[0]["features.3.weight"], sds[0]["features.3.bias"]
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.relu(torch.randn(2, 64, H, W, generator=g))
    _conv_check(ops.conv2d(x.cuda(), w.cuda(), b.cuda(), pad=2, relu=True), x.double(), w, b, padding=2)


@pytest.mark.parametrize("idx", [6, 8, 10])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (3, 5), (6, 8)])
def test_conv3_to_5(sds, idx, H, W):
    from bem import ops
    w, b = sds[0][f"features.{idx}.weight"], sds[0][f"features.{idx}.bias"]
    g = torch.Generator().manual_seed(idx * 1000 + H * 10 + W)
    x = torch.relu(torch.randn(2, w.shape[1], H, W, generator=g))
    _conv_check(ops.conv2d(x.cuda(), w.cuda(), b.cuda(), pad=1, relu=True), x.double(), w, b, padding=1)


@pytest.mark.parametrize("C", [64, 192, 384, 256])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7)])
def test_head(C, h, w):
    from bem import ops
    g = torch.Generator().manual_seed(C + h)
    f = torch.relu(torch.randn(4, C, h, w, generator=g))
    f[0, :, 0, 0] = 0                                      # a pixel whose features are all zero in one image: yhat = 0 / 1e-10 = 0
    f[1, :, h - 1, w - 1] = 0                              # and in both
    f[3, :, h - 1, w - 1] = 0
    lin = torch.rand(C, generator=g) * 2 / C
    want = R.head(f[:2].double(), f[2:].double(), lin.double())
    got, ws = ops.lpips_layer(f.cuda(), lin.cuda())
    err = (got.cpu().double() - want).abs()
    print(f"head C={C} {h}x{w}: f64 {want.tolist()}, abs err {err.tolist()}")
    assert float(want.max()) > 0 and bool((err <= 1e-6 * want).all())          # a pair of two all-zero pixels (1x1 planes) is exactly 0
    # a second layer adds to the first; a crop of a wider tensor gives the same bits
    big = torch.zeros(4, C, h + 2, w + 3)
    big[:, :, 1:1 + h, 2:2 + w] = f
    got2, _ = ops.lpips_layer(big.cuda()[:, :, 1:1 + h, 2:2 + w], lin.cuda(), ws=ws, out=got.clone(), first=False)
    assert bool(((got2.cpu().double() - 2 * want).abs() <= 2e-6 * want).all())
    again, _ = ops.lpips_layer(big.cuda()[:, :, 1:1 + h, 2:2 + w], lin.cuda())
    assert torch.equal(again, got)


# ------------------------------------------------------------------------------ the whole metric
SHAPES = [(31, 31), (37, 53), (64, 64), (100, 152)]


def _pairs(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    a = torch.rand(2, 3, H, W, generator=g)
    return {"independent": (a, torch.rand(2, 3, H, W, generator=g)), "close": (a, a + 0.02 * torch.randn(2, 3, H, W, generator=g)), "same": (a, a)}


@pytest.fixture(scope="module")
def refs(sds):
    """float64 values of every case, computed once."""
    return {(H, W, kind): R.lpips01(sds[0], sds[1], a, b) for H, W in SHAPES for kind, (a, b) in _pairs(H, W).items()}


@pytest.mark.parametrize("H,W", SHAPES)
def test_metric(metric, refs, sds, H, W):
    for kind, (a, b) in _pairs(H, W).items():
        want = refs[(H, W, kind)]
        got = metric.distance01(a.cuda(), b.cuda())
        assert got.shape == (2,) and got.dtype == torch.float32
        assert torch.equal(metric.distance01(a.cuda(), b.cuda()), got)              # bit-identical on a second call
        got = got.cpu().double()
        if kind == "same":
            assert torch.equal(want, torch.zeros(2, dtype=torch.float64)) and torch.equal(got, torch.zeros(2, dtype=torch.float64))
            continue
        rel = float(((got - want).abs() / want).max())
        print(f"lpips {H}x{W} {kind}: f64 {want.tolist()}, HIP rel err {rel:.3e}")
        assert rel <= 1e-5
        # forward on the [-1,1] tensors im2tensor makes of the quantised images, and on [0,1] tensors with normalize
        t0 = torch.cat([R.im2tensor(R.img_as_ubyte(a[i].permute(1, 2, 0).numpy()), torch.float32) for i in range(2)])
        t1 = torch.cat([R.im2tensor(R.img_as_ubyte(b[i].permute(1, 2, 0).numpy()), torch.float32) for i in range(2)])
        fw = metric(t0.cuda(), t1.cuda())
        assert fw.shape == (2, 1, 1, 1)
        assert float(((fw.cpu().double().view(-1) - R.lpips(sds[0], sds[1], t0, t1)).abs() / want).max()) <= 1e-5
        assert float(((fw.cpu().double().view(-1) - got).abs() / want).max()) <= 2e-5
        fn = metric((t0.cuda() + 1) / 2, (t1.cuda() + 1) / 2, normalize=True)
        assert float(((fn.cpu().double().view(-1) - got).abs() / want).max()) <= 2e-5


# ------------------------------------------------------------------------------ the drivers
def _script(name):
    spec = importlib.util.spec_from_file_location("bem_" + name + "_lpips_gpu", os.path.join(PKG, "Enhancement", name + ".py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_eval_driver_and_cal_metrics(tmp_path, sds, capsys):
    from PIL import Image
    from bem.pipeline import build_nets, synthetic_pair
    drv = _script("eval")
    net1, net2 = build_nets(device="cpu")
    torch.save({"params": net1.state_dict()}, tmp_path / "cg.pth")
    torch.save({"params": net2.state_dict()}, tmp_path / "s2.pth")
    (tmp_path / "w").mkdir()
    torch.save(sds[0], tmp_path / "w" / R.ALEXNET_FILE)
    torch.save(sds[1], tmp_path / "w" / R.LIN_FILE)
    (tmp_path / "in").mkdir(); (tmp_path / "gt").mkdir()
    lq, gt = synthetic_pair((2, 3, 64, 64))
    for i in range(2):
        for d, t in (("in", lq), ("gt", gt)):
            Image.fromarray(np.rint(t[i].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(tmp_path / d / f"{i}.png")
    out = drv.main(["--opt", os.path.join(PKG, "Options", "CG_UNet_LOLv1.yml"), "--cond_opt", os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml"),
                    "--weights", str(tmp_path / "cg.pth"), "--cond_weights", str(tmp_path / "s2.pth"), "--input_dir", str(tmp_path / "in"),
                    "--target_dir", str(tmp_path / "gt"), "--result_dir", str(tmp_path / "res"), "--dataset", "synthetic", "--num_samples", "2",
                    "--seed", "11", "--GT_mean", "--lpips", "--lpips_weights", str(tmp_path / "w")])
    assert sorted(os.listdir(out["result_dir"])) == ["0.png", "1.png", "result.txt"]
    assert len(out["lpips"]) == 2
    lines = open(os.path.join(out["result_dir"], "result.txt")).read().splitlines()
    want_line = f"Best_lpips: {np.mean(out['lpips']):.4f} "
    assert [ln for ln in lines if ln.startswith("Best_lpips")] == [want_line]
    assert [ln.split(":")[0] for ln in lines[:3]] == ["Best_PSNR", "Best_SSIM", "Best_lpips"]
    # the driver's value is the metric of the image it saved: its quantisation is save_rgb's
    u8 = lambda p: np.asarray(Image.open(p).convert("RGB"))
    for i in range(2):
        want = float(R.lpips(sds[0], sds[1], R.im2tensor(u8(tmp_path / "gt" / f"{i}.png")), R.im2tensor(u8(os.path.join(out["result_dir"], f"{i}.png"))))[0])
        print(f"driver image {i}: f64 {want:.6e}, driver {out['lpips'][i]:.6e}")
        assert want > 0 and abs(out["lpips"][i] - want) <= 1e-5 * want
    capsys.readouterr()
    m = _script("cal_metrics_with_imgs").main(["--pred_dir", out["result_dir"], "--target_dir", str(tmp_path / "gt"), "--psnr", "--ssim", "--lpips",
                                               "--lpips_weights", str(tmp_path / "w")])
    printed = capsys.readouterr().out.splitlines()
    assert want_line.strip() in printed and m["lpips"] == out["lpips"]
    assert [ln.split(":")[0] for ln in printed] == ["Best_PSNR", "Best_SSIM", "Best_lpips"]
    assert abs(np.mean(m["ssim"]) - np.mean(out["ssim"])) < 1e-6
