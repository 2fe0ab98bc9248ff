"""GPU: the folded decoder level -- fuse(cat(up(pre(f)), skip)) as one kernel (csrc/upfuse_x6.hip, ops.up_fuse, modules.fold_up_fuse).

* the op against float64, held to the error of torch's own f32 evaluation of the chain;
* exact placement: with f = 0 and Wf2 = I every skip value arrives at its own (channel, row, column) bit for bit;
* the nets with the folded path on and off against the oracle (the Stage-II float64 parity bound of the suite);
* the cached folded weights follow an in-place weight update;
* training records the layers as before and gives the same loss to the bit."""
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


# ----------------------------------------------------------------------------- the op ---
SHAPES = [(2, 80, 8, 8),        # one partial tile
          (2, 80, 5, 33),       # odd width, tiles wrap row ends
          (2, 160, 4, 6),       # K streamed over ten k-blocks, three M-tiles
          (2, 14, 3, 5),        # Cin no multiple of 16, C/2 = 7
          (1, 80, 16, 80),      # the config-5 level-1 width
          (3, 80, 7, 160)]      # the config-5 level-0 low-res width, batch stride


def _level(c, seed, pre):
    from bem.modules import ConvT2x2, PwConv2d
    torch.manual_seed(seed)
    return ConvT2x2(c, c // 2), PwConv2d(c, c // 2, bias=False), (PwConv2d(c, c, bias=False) if pre else None)


def _chain(f, skip, up, fuse, pre, dtype):
    """conv_transpose2d -> cat -> conv2d from the f32 weights, evaluated in ``dtype`` by torch on the CPU."""
    c = lambda t: t.detach().to(dtype)
    x = F.conv2d(c(f), c(pre.weight)) if pre is not None else c(f)
    return F.conv2d(torch.cat([F.conv_transpose2d(x, c(up.weight), c(up.bias), stride=2), c(skip)], 1), c(fuse.weight))


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "pre"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_up_fuse_vs_float64(ops, shape, pre):
    """ops.up_fuse is no further from the float64 chain than torch's f32 evaluation of the same chain is, in mean and in max absolute
    error, with no margin: the folded form rounds the composed weights once and the x6 products add less than one f32 GEMM's error."""
    from bem.modules import fold_up_fuse
    B, C, h, w = shape
    up, fuse, prel = _level(C, 1000 * C + 10 * h + w, pre)
    g = torch.Generator().manual_seed(h * w + C)
    f, skip = torch.randn(B, C, h, w, generator=g), torch.randn(B, C // 2, 2 * h, 2 * w, generator=g)
    r64, r32 = _chain(f, skip, up, fuse, prel, torch.float64), _chain(f, skip, up, fuse, prel, torch.float32)
    for m in (up, fuse) + ((prel,) if pre else ()):
        m.cuda()
    got = ops.up_fuse(f.cuda(), skip.cuda(), fold_up_fuse(up, fuse, prel))
    assert got.shape == r64.shape and torch.isfinite(got).all()
    (rm, rM), (hm, hM) = Y.errors(r32, r64), Y.errors(got.cpu(), r64)
    print(f"PARITY up_fuse {shape} pre={pre}: f32 chain mean {rm:.3e} max {rM:.3e} | up_fuse mean {hm:.3e} max {hM:.3e}")
    assert hm <= rm and hM <= rM, (shape, pre, hm, rm, hM, rM)


@pytest.mark.parametrize("shape", [(2, 14, 3, 5), (2, 80, 5, 33), (1, 160, 4, 6)], ids=lambda s: "x".join(map(str, s)))
def test_up_fuse_places_every_skip_pixel_exactly(ops, shape):
    """f = 0, Wc = 0, bias = 0, Wf2 = I: out is skip, bit for bit -- one-hot planes (a single 1 whose position depends on the row and the
    channel) and a plane set of distinct values."""
    B, C, h, w = shape
    Co = C // 2
    folded = ops.UpFuseWeights(ops.pack_pw_weight(torch.zeros(4, Co, C, device="cuda")), ops.pack_pw_weight(torch.eye(Co, device="cuda")),
                               torch.zeros(Co, device="cuda"), C)
    f = torch.zeros(B, C, h, w, device="cuda")
    onehot = torch.zeros(B, Co, 4 * h * w)
    for b in range(B):
        for c in range(Co):
            onehot[b, c, (7 * c + 3 * b) % (4 * h * w)] = 1.0
    g = torch.Generator().manual_seed(5)
    for skip in (onehot.view(B, Co, 2 * h, 2 * w), torch.randn(B, Co, 2 * h, 2 * w, generator=g)):
        skip = skip.cuda().contiguous()
        out = ops.up_fuse(f, skip, folded)
        assert torch.equal(out, skip), float((out - skip).abs().max())


def test_up_fuse_rejects_bad_operands(ops):
    from bem.modules import fold_up_fuse
    up, fuse, _ = _level(16, 1, False)
    up.cuda(), fuse.cuda()
    folded = fold_up_fuse(up, fuse)
    f, skip = torch.zeros(2, 16, 4, 6, device="cuda"), torch.zeros(2, 8, 8, 12, device="cuda")
    assert ops.up_fuse(f, skip, folded).shape == skip.shape
    with pytest.raises(ValueError):
        ops.up_fuse(f, torch.zeros(2, 8, 8, 10, device="cuda"), folded)                     # skip not (B, C/2, 2h, 2w)
    with pytest.raises(ValueError):
        ops.up_fuse(f, skip[:, :, :, ::2], folded)                                          # not contiguous
    with pytest.raises(ValueError):
        ops.up_fuse(torch.zeros(2, 32, 4, 6, device="cuda"), torch.zeros(2, 16, 8, 12, device="cuda"), folded)      # weights made for C = 16
    with pytest.raises(TypeError):
        ops.up_fuse(f.double(), skip, folded)


# ----------------------------------------------------------------------------- the nets ---
def _yardstick(out, r32, r64, what):
    """tests/test_modules_gpu.py::_yardstick, the Stage-II float64 parity bound of the suite (test_stage2_config5_vs_float64, Stage II in
    isolation): HIP no further from float64 than 2x the f32 oracle, mean and max."""
    (rm, rM), (hm, hM) = Y.errors(r32, r64), Y.errors(out, r64)
    print(f"{what} vs float64: f32 oracle mean {rm:.3e} max {rM:.3e} | HIP mean {hm:.3e} max {hM:.3e} ({hm / rm:.2f}x, {hM / rM:.2f}x)")
    assert torch.isfinite(out).all()
    assert hm <= 2 * rm and hM <= 2 * rM, (what, hm, rm, hM, rM)


def _net_input():
    g = torch.Generator().manual_seed(11)
    return torch.cat([0.25 * torch.rand(2, 3, 64, 64, generator=g), torch.rand(2, 3, 64, 64, generator=g)], 1)


def _run(ops, net, x, folded):
    """Eval forward with the folded path on / off; returns the output and how many times ops.up_fuse ran."""
    calls, real = [], ops.up_fuse
    with mock.patch.object(ops, "USE_UPFUSE", folded), mock.patch.object(ops, "up_fuse", lambda *a: (calls.append(1), real(*a))[1]):
        with torch.no_grad():
            out = net(x.cuda())[-1].cpu()
    return out, len(calls)


def _refs(name, net, x):
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    return Y.oracle(name, sd, x, O.selective_scan_c), Y.float64_ref(name, sd, x)


@pytest.fixture(scope="module")
def ddw(ops):
    """DecompDualBranchDDWavelet at n_feat 16, [1,1,1], 2 rows of 64x64, with its oracle results (made once)."""
    name = "DecompDualBranchDDWavelet"
    net = Y.build_arch(name, n_feat=16, num_blocks=(1, 1, 1), seed=100).cuda().eval()
    x = _net_input()
    return name, net, x, _refs(name, net, x)


def test_dual_branch_net_folded_and_unfolded_vs_oracle(ops, ddw):
    """Both forms against O.ddwavelet_ref (f32) and its float64 evaluation; the folded one launches four up_fuse kernels (two branches x two
    levels, bottleneck_to_Q* folded into the first) and none of the layers it replaces."""
    name, net, x, (r32, r64) = ddw
    launched = []
    hooks = [m.register_forward_hook(lambda m, a, o, n=n: launched.append(n)) for n, m in net.named_modules()
             if n.startswith("bottleneck_to") or n.endswith((".up", ".fuse"))]
    try:
        out, n = _run(ops, net, x, True)
        assert n == 4 and launched == [], (n, launched)
        _yardstick(out, r32, r64, f"{name} folded")
        out0, n0 = _run(ops, net, x, False)
        assert n0 == 0 and len(launched) == 10, (n0, launched)
        _yardstick(out0, r32, r64, f"{name} unfolded")
    finally:
        for h in hooks:
            h.remove()
    print(f"folded vs unfolded: max |d| {float((out - out0).abs().max()):.3e}")


def test_single_branch_net_folded_and_unfolded_vs_oracle(ops):
    """DecompSingleBranch: the folded path without a layer ahead of the first level (pre=None)."""
    name = "DecompSingleBranch"
    net = Y.build_arch(name, n_feat=16, num_blocks=(1, 1, 1), seed=100).cuda().eval()
    x = _net_input()
    r32, r64 = _refs(name, net, x)
    out, n = _run(ops, net, x, True)
    assert n == 2, n
    _yardstick(out, r32, r64, f"{name} folded")
    out0, n0 = _run(ops, net, x, False)
    assert n0 == 0
    _yardstick(out0, r32, r64, f"{name} unfolded")


def test_folded_weights_follow_a_weight_update(ops, ddw):
    """The folded operands are cached per weight version and weight epoch: after an in-place change of up.weight (and of the layer folded
    in ahead of it) and ops.bump_weight_epoch() the next forward is the changed net's -- both forms against the changed net's oracle."""
    name, net, x, _ = ddw
    before, _ = _run(ops, net, x, True)
    ups = [net.decoders_Q1[0]["up"].weight, net.decoders_Q2[1]["up"].weight, net.bottleneck_to_Q2.weight]
    with torch.no_grad():
        for t in ups:
            t.mul_(1.25)
    ops.bump_weight_epoch()
    try:
        r32, r64 = _refs(name, net, x)
        after, n = _run(ops, net, x, True)
        assert n == 4
        assert float((after - before).abs().max()) > 1e-3
        _yardstick(after, r32, r64, "after the update, folded")
        _yardstick(_run(ops, net, x, False)[0], r32, r64, "after the update, unfolded")
    finally:
        with torch.no_grad():
            for t in ups:
                t.div_(1.25)
        ops.bump_weight_epoch()


# ----------------------------------------------------------------------------- training ---
def _unfolded_decode(self, sfx, f, skips, pre=None):
    """The decoder walk as it was before the folded kernel existed: every layer its own call."""
    if pre is not None:
        f = pre(f)
    for dec, skip in zip(getattr(self, "decoders" + sfx), reversed(skips)):
        f = dec["block"](dec["fuse"](dec["up"](f), x2=skip, in_mode=2))
    return getattr(self, "proj" + sfx)(f)


def _node_types(t):
    """Names of the autograd nodes reachable from t, in depth-first order."""
    seen, order, stack = set(), [], [t.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        order.append(type(fn).__name__)
        stack.extend(nf for nf, _ in reversed(fn.next_functions))
    return order


def _train_step(patch):
    """One ImageEnhancer.optimize_parameters step of the small DDWavelet net from seeded weights -> (l_pix, gradient norm, node types)."""
    import contextlib
    import bem.archs as A
    from basicsr.models import build_model
    from bem import autograd as ag
    opt = dict(model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, condition=dict(type="mean", scale_down=16, noise_level=0.0),
               network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                              mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model="model4"),
               path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None),
               train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                          scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                          optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                          pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))
    g = torch.Generator().manual_seed(33)
    lq, gt = 0.25 * torch.rand(1, 3, 32, 32, generator=g), torch.rand(1, 3, 32, 32, generator=g)
    gt_down = F.interpolate(gt, scale_factor=1 / 16, mode="bilinear")
    with (mock.patch.object(A._Stage2, "_decode", _unfolded_decode) if patch else contextlib.nullcontext()):
        torch.manual_seed(100)
        model = build_model(opt)
        x = torch.cat([lq, F.interpolate(gt_down, scale_factor=16, mode="bilinear", align_corners=False)], 1).cuda()
        model.net_g.train()
        nodes = _node_types(ag.l1_loss(model.net_g(x)[-1], gt.cuda()))
        model.feed_train_data(dict(lq=lq, gt=gt, gt_down=gt_down))
        tn = model.optimize_parameters(1)
        return float(model.log_dict["l_pix"]), float(tn), nodes


def test_training_step_is_unchanged(ops):
    """In train() mode the decoder runs its layers as autograd nodes, bottleneck_to_Q* first: the same node types in the same order and
    bit-identical loss and gradient norm as with the former decoder walk."""
    loss, tn, nodes = _train_step(False)
    loss0, tn0, nodes0 = _train_step(True)
    assert nodes == nodes0 and {"ConvT2x2FnBackward", "PwFnBackward"} <= set(nodes), sorted(set(nodes))
    print(f"training step: loss {loss!r} / {loss0!r}, gradient norm {tn!r} / {tn0!r}, {len(nodes)} nodes")
    assert loss == loss0 and tn == tn0
