"""The three kernels on the shared 4 x 32 pixel tile (bem_ss2d_front_x6_f32, bem_gdmlp_x6_f32, bem_vss_back_x6_f32) at the smallest shapes
that reach every address and mask path of their loads and stores: ragged last tile row and column with the halo clamped at all four image
borders, one exact tile, two tiles across, a second k-block that is not full (C = 24), the C = 80 form, C % 8 != 0, with and without biases.
Each output is compared with torch in float64 (the reference and the bounds of tests/test_ops_gpu.py and tests/test_vss_back_gpu.py for the
same op) and is allocated inside a larger buffer of canary values, so that a store through a wrong or clamped address shows."""
import pytest
import torch
import torch.nn.functional as F

from large_rows import canaries

pytestmark = pytest.mark.gpu

# (B, C, H, W)
TILE_CASES = [(2, 40, 6, 34), (1, 48, 4, 32), (2, 24, 5, 33), (1, 40, 9, 64)]
GDMLP_ONLY = [(1, 80, 8, 36), (1, 36, 5, 33)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as o
    return o


def dev(t):
    return t.cuda().contiguous()


def close(a, b, rtol, atol, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    print(f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})")
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})"


def ln64(v, w, b, eps):
    mu, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
    return (v - mu) / (var + eps).sqrt() * w.double()[None, :, None, None] + b.double()[None, :, None, None]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cfg", TILE_CASES)
def test_ss2d_front_edges(ops, monkeypatch, cfg, bias):
    B, C, H, W = cfg
    Mx = 20 if C >= 40 else 16                                             # 4 (R + 2) with the shipped dt ranks 3 and 2
    g = torch.Generator().manual_seed(C * Mx + H)
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.3
    lw, lb = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    wi = torch.randn(C, C, generator=g) * C ** -0.5
    bi = 0.3 * torch.randn(C, generator=g) if bias else None
    wd = torch.randn(C, 1, 3, 3, generator=g) / 3
    bd = 0.2 * torch.randn(C, generator=g) if bias else None
    wx = torch.randn(Mx, C, generator=g) * C ** -0.5
    Wpi, Wpx = ops.pack_pw_weight(dev(wi), x6=True), ops.pack_pw_weight(dev(wx), x6=True)
    args = (dev(x), dev(lw), dev(lb), 1e-6, Wpi, None if bi is None else dev(bi), dev(wd), None if bd is None else dev(bd), Wpx, Mx)
    with canaries(monkeypatch):
        xc, xd = ops.ss2d_front(*args)
    tt = F.conv2d(ln64(x.double(), lw, lb, 1e-6), wi.double()[:, :, None, None], None if bi is None else bi.double())
    c64 = F.silu(F.conv2d(tt, wd.double(), None if bd is None else bd.double(), padding=1, groups=C))
    close(xc, c64.float(), 1e-4, 4e-5, f"ss2d_front xc vs torch f64 {cfg} bias={bias}")
    close(xd, F.conv2d(c64, wx.double()[:, :, None, None]).float(), 1e-4, 4e-5, f"ss2d_front xd vs torch f64 {cfg} bias={bias}")


def _gd_case(cfg, bias):
    B, C, H, W = cfg
    Hd = 320 if C == 80 else 48                                            # three chunks: both parameter buffers and a reused one
    g = torch.Generator().manual_seed(C * Hd + H + 7 * W)
    t = dict(x=torch.randn(B, C, H, W, generator=g) * 2 + 0.3, y0=torch.randn(B, C, H, W, generator=g) + 0.2,
             y1=torch.randn(B, C, H, W, generator=g) * 1.5 - 0.1,
             onw=1 + 0.2 * torch.randn(C, generator=g), onb=0.1 * torch.randn(C, generator=g),
             wop=torch.randn(C, C, generator=g) * C ** -0.5, bop=0.3 * torch.randn(C, generator=g) if bias else None,
             lw=1 + 0.2 * torch.randn(C, generator=g), lb=0.1 * torch.randn(C, generator=g),
             wi=torch.randn(2 * Hd, C, generator=g) * C ** -0.5, bi=0.3 * torch.randn(2 * Hd, generator=g) if bias else None,
             wd=torch.randn(2 * Hd, 1, 3, 3, generator=g) / 3, bd=0.2 * torch.randn(2 * Hd, generator=g) if bias else None,
             wo=torch.randn(C, Hd, generator=g) * Hd ** -0.5, bo=0.3 * torch.randn(C, generator=g) if bias else None)
    return Hd, t


def _gd_run(ops, monkeypatch, Hd, t, fused):
    d = {k: (None if v is None else dev(v)) for k, v in t.items()}
    perm = ops.gate_interleave(Hd, "cpu")
    Wg = ops.pack_pw_weight(dev(t["wi"][perm]), x6=True)
    bg = dev(t["bi"][perm]) if t["bi"] is not None else torch.zeros(2 * Hd, device="cuda")
    w10 = ops.dw_gate_params10(d["wd"], d["bd"], Hd)
    Wo = ops.pack_pw_weight(d["wo"], x6=True)
    pre = (d["y0"], d["y1"], d["onw"], d["onb"], 1e-5, ops.pack_vss_back_outproj(d["wop"]), d["bop"]) if fused else None
    with canaries(monkeypatch):
        return ops.gdmlp_x6(d["x"], d["lw"], d["lb"], 1e-6, Wg, bg, w10, Wo, d["bo"], Hd, pre=pre)


def _gd_ref64(Hd, t, fused):
    o = lambda v: None if v is None else v.double()
    x1 = t["x"].double()
    if fused:
        x1 = x1 + F.conv2d(ln64(t["y0"].double() + t["y1"].double(), t["onw"], t["onb"], 1e-5), t["wop"].double()[:, :, None, None], o(t["bop"]))
    tt = F.conv2d(ln64(x1, t["lw"], t["lb"], 1e-6), t["wi"].double()[:, :, None, None], o(t["bi"]))
    hh = F.conv2d(tt, t["wd"].double(), o(t["bd"]), padding=1, groups=2 * Hd)
    return (x1 + F.conv2d(F.gelu(hh[:, :Hd]) * hh[:, Hd:], t["wo"].double()[:, :, None, None], o(t["bo"]))).float()


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cfg", TILE_CASES + GDMLP_ONLY)
def test_gdmlp_x6_edges(ops, monkeypatch, cfg, bias):
    Hd, t = _gd_case(cfg, bias)
    y = _gd_run(ops, monkeypatch, Hd, t, False)
    close(y, _gd_ref64(Hd, t, False), 1e-4, 4e-5, f"gdmlp_x6 vs torch f64 {cfg} bias={bias}")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cfg", TILE_CASES)
def test_gdmlp_x6_pre_edges(ops, monkeypatch, cfg, bias):
    Hd, t = _gd_case(cfg, bias)
    y = _gd_run(ops, monkeypatch, Hd, t, True)
    close(y, _gd_ref64(Hd, t, True), 1e-4, 4e-5, f"gdmlp_x6 with pre vs torch f64 {cfg} bias={bias}")
