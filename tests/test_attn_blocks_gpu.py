"""Every kernel of csrc/attn_blocks.hip (and the plane means under the SE gate) at op level against the float64 references of
tests/attn_blocks_ref.py, on the shape grid R.SHAPES: the shipped width C = 160 / Cr = 10 on its three plane sizes, the fixtures' width,
and the ragged / degenerate / narrow planes where the lane-, wave- and thread-strided loops stop being single passes.

Bounds.  Each is relative to the error of the float32 CPU evaluation of the same formula against float64 (the reference's own error):
  * per-pixel outputs (out, dx, chan_scale, row_scale, gates): mean and max |err| <= 2x the f32 reference's (the convention of
    test_modules_gpu.py::_yardstick), with a floor of one f32 ulp (2^-23) of the output's mean / max magnitude where the reference is exact;
  * reductions (chan_dot, plane means, dw, dW1, dW2, dmean): |err| / (float64 sum of the absolute terms, plus |fill| for accumulated
    outputs), worst element, <= MARGIN x the f32 reference's worst for that case, floor 2^-23.  MARGIN is set from the measured ratios in
    profiles/attn_blocks_parity.txt; one dropped block of 256 terms (profiles/attn_blocks_fault_injection.txt, fault e) is a normalised
    error of 4e-3 .. 7e-2 on the shipped planes and fails at any margin below 3e4.
Accumulated outputs (dw, dW1, dW2, chan_dot's parameter mode) start from a random fill and are called twice: fill + g, then fill + 2 g.
Float atomics across workgroups make them order-dependent, so they are held to the bound both times, not compared bit for bit."""
import pytest
import torch

import attn_blocks_ref as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
MARGIN = 4.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import native
    native.lib()


def dev(t):
    return t.cuda().contiguous()


def _err(a, r64):
    e = (a.detach().cpu().double() - r64).abs()
    return float(e.mean()), float(e.max())


def per_pixel(got, r32, r64, what):
    """got no further from float64 than 2x the f32 reference, mean and max; floor one f32 ulp of the output's magnitude."""
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    (rm, rM), (hm, hM) = _err(r32, r64), _err(got, r64)
    fm, fM = ULP * float(r64.abs().mean()), ULP * float(r64.abs().max())
    print(f"PARITY pixel {what}: f32 ref mean {rm:.3e} max {rM:.3e} | HIP mean {hm:.3e} max {hM:.3e} | ratio {hm / max(rm, fm, 1e-300):.2f} {hM / max(rM, fM, 1e-300):.2f}")
    assert hm <= max(2 * rm, fm) and hM <= max(2 * rM, fM), (what, hm, rm, hM, rM, fm, fM)


def reduction(got, r32, r64, scale, what):
    """Worst |err| / scale over the elements (scale: float64 sum of absolute terms) against MARGIN x the f32 reference's, floor 2^-23."""
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    scale = scale.clamp_min(1e-300)
    rn = float(((r32.double() - r64).abs() / scale).max())
    hn = float(((got.detach().cpu().double() - r64).abs() / scale).max())
    print(f"PARITY sum {what}: f32 ref {rn:.3e} | HIP {hn:.3e} | ratio {hn / max(rn, ULP):.2f}")
    assert hn <= max(MARGIN * rn, ULP), (what, hn, rn)


def both(fn, *args, **kw):
    """fn on the float32 values and on their float64 copies."""
    cast = lambda t, d: t.to(d) if torch.is_tensor(t) else t
    return tuple(fn(*[cast(a, d) for a in args], **{k: cast(v, d) for k, v in kw.items()}) for d in (torch.float32, torch.float64))


def _inputs(name, seed):
    B, C, Cr, H, W = R.SHAPES[name]
    g = R.gen(seed)
    x = R.randn(g, B, C, H, W) + R.randn(g, 1, C, 1, 1)                 # channel offsets: the plane means are O(1)
    return g, (B, C, Cr, H, W), x


CASES = list(R.SHAPES)


# ---------------------------------------------------------------------------------------------------------------- forwards
@pytest.mark.parametrize("name", CASES)
def test_forward_kernels(name):
    from bem import ops
    g, (B, C, Cr, H, W), x = _inputs(name, 11)
    tag = f"{name} {R.SHAPES[name]}"
    x_d = dev(x)
    (m32, _), (m64, mabs) = both(R.plane_mean, x)
    reduction(ops.plane_mean(x_d), m32, m64, mabs, f"plane_mean {tag}")
    w1, w2 = R.randn(g, Cr, C, scale=0.5), R.randn(g, C, Cr, scale=0.5)
    y_d, mean_d = ops.se_gate(x_d, dev(w1), dev(w2), want_mean=True)
    y32, y64 = both(lambda x_, a, b: R.se_gate(R.plane_mean(x_)[0], a, b), x, w1, w2)
    per_pixel(y_d, y32, y64, f"se_gate {tag}")
    reduction(mean_d, m32, m64, mabs, f"se_gate's means {tag}")
    # row_scale: a (C,C,1,1) weight and its bias, as CrossFusionBlock folds its gate
    gate = 1 + 0.3 * R.randn(g, C)
    for wt in (R.randn(g, C, C, 1, 1), R.randn(g, C)):
        per_pixel(ops.row_scale(dev(wt), dev(gate)), *both(R.row_scale, wt, gate), f"row_scale {tuple(wt.shape)} {tag}")
    # chan_scale: every combination
    add, bc, sb = R.randn(g, B, C, H, W), R.randn(g, B, C), R.randn(g, B, C)
    for scale, sname in ((gate, "parameter"), (gate.reshape(1, C, 1, 1), "parameter (1,C,1,1)"), (sb, "per image")):
        for a in (None, add):
            for b_ in (None, bc):
                r32, r64 = both(R.chan_scale, x, scale, a, b_, 1.0 / (H * W))
                got = ops.chan_scale(x_d, dev(scale), None if a is None else dev(a), None if b_ is None else dev(b_), 1.0 / (H * W))
                per_pixel(got, r32, r64, f"chan_scale {sname} add={a is not None} add_bc={b_ is not None} {tag}")
    # chan_dot: per image, and accumulated into a parameter's gradient from a non-zero fill, twice
    (d32, _), (d64, dabs) = both(R.chan_dot, x, add)
    reduction(ops.chan_dot(x_d, dev(add)), d32, d64, dabs, f"chan_dot per image {tag}")
    (p32, _), (p64, pabs) = both(R.chan_dot, x, add, per_image=False)
    fill = R.randn(g, C)
    out_d = dev(fill.clone())
    for n in (1, 2):
        assert ops.chan_dot(x_d, dev(add), out_d) is out_d
        r32 = fill + p32 if n == 1 else fill + p32 + p32
        reduction(out_d, r32, fill.double() + n * p64, fill.double().abs() + n * pabs, f"chan_dot parameter, call {n} {tag}")
    # spatial attention: both kernel sizes, with and without the SE gate as the per-image channel factor
    for k in (3, 7):
        w = R.randn(g, 1, 2, k, k, scale=0.3)
        for cs in (None, y_d.cpu()):
            r32, r64 = both(R.spatial_attention, x, w, cs)
            got = ops.spatial_attention(x_d, dev(w), None if cs is None else dev(cs))
            per_pixel(got, r32, r64, f"spatial_attention k={k} gate={cs is not None} {tag}")


# ---------------------------------------------------------------------------------------------------------------- backwards
def _se_backward(name, x, w1, w2, dy, fills, tag):
    from bem import ops
    x_d, w1_d, w2_d = dev(x), dev(w1), dev(w2)
    y_d, mean_d = ops.se_gate(x_d, w1_d, w2_d, want_mean=True)
    r32, r64 = both(lambda x_, a, b, d: R.se_gate_bwd(R.plane_mean(x_)[0], a, b, d), x, w1, w2, dy)
    dw1_d, dw2_d = dev(fills[0].clone()), dev(fills[1].clone())
    for n in (1, 2):
        dmean = ops.se_gate_bwd(mean_d, w1_d, w2_d, y_d, dev(dy), dw1_d, dw2_d)
        reduction(dmean, r32["dmean"], r64["dmean"], r64["dmean_abs"], f"se_gate_bwd dmean, call {n} {tag}")
        for key, got, fill in (("dw1", dw1_d, fills[0]), ("dw2", dw2_d, fills[1])):
            want32 = fill + r32[key] if n == 1 else fill + r32[key] + r32[key]
            reduction(got, want32, fill.double() + n * r64[key], fill.double().abs() + n * r64[key + "_abs"], f"se_gate_bwd {key}, call {n} {tag}")


def _sa_backward(x, w, dout, fill, tag):
    from bem import ops
    x_d, w_d = dev(x), dev(w)
    r32, r64 = both(R.spatial_attention_bwd, x, w, dout)
    out_d, amap = ops.spatial_attention(x_d, w_d, want_map=True)
    per_pixel(out_d, r32["out"], r64["out"], f"spatial_attention out {tag}")
    dw_d = dev(fill.clone())
    for n in (1, 2):
        dx = ops.spatial_attention_bwd(x_d, dev(dout), amap, w_d, dw_d)
        per_pixel(dx, r32["dx"], r64["dx"], f"spatial_attention_bwd dx, call {n} {tag}")
        want32 = fill + r32["dw"] if n == 1 else fill + r32["dw"] + r32["dw"]
        reduction(dw_d, want32, fill.double() + n * r64["dw"], fill.double().abs() + n * r64["dw_abs"], f"spatial_attention_bwd dw, call {n} {tag}")


@pytest.mark.parametrize("name", CASES)
def test_backward_kernels(name):
    g, (B, C, Cr, H, W), x = _inputs(name, 12)
    tag = f"{name} {R.SHAPES[name]}"
    w1, w2 = R.randn(g, Cr, C, scale=0.5), R.randn(g, C, Cr, scale=0.5)
    _se_backward(name, x, w1, w2, R.randn(g, B, C), (R.randn(g, Cr, C), R.randn(g, C, Cr)), tag)
    dout = R.randn(g, B, C, H, W)
    for k in (3, 7):
        _sa_backward(x, R.randn(g, 1, 2, k, k, scale=0.3), dout, R.randn(g, 1, 2, k, k), f"k={k} {tag}")


@pytest.mark.parametrize("name", CASES)
def test_saturated_attention(name):
    """Attention weights scaled so that the pre-sigmoid plane reaches about +-100: finite, and equal to float64 at both saturated ends."""
    from bem import ops
    g, (B, C, Cr, H, W), x = _inputs(name, 13)
    tag = f"{name} {R.SHAPES[name]}"
    dout, cs = R.randn(g, B, C, H, W), torch.sigmoid(R.randn(g, B, C))
    for k in (3, 7):
        w0 = R.randn(g, 1, 2, k, k, scale=0.3)
        w = R.saturating_weight(x, w0)
        pre = R.spatial_attention(x.double(), w.double(), parts=True)[2]
        assert 99 <= float(pre.abs().max()) <= 101
        _sa_backward(x, w, dout, R.randn(g, 1, 2, k, k), f"saturated k={k} {tag}")
        wg = R.saturating_weight(x, w0, chan_scale=cs)
        per_pixel(ops.spatial_attention(dev(x), dev(wg), dev(cs)), *both(R.spatial_attention, x, wg, cs), f"saturated, gated k={k} {tag}")


@pytest.mark.parametrize("name", CASES)
def test_argmax_ties_route_to_the_first_maximum(name):
    """Inputs on multiples of 1/4 (exact in f32 and f64): the channel maximum is tied at most pixels, and dx must carry the max branch's
    gradient on the first maximal channel, as torch.max(dim) and hence the float64 autograd reference do."""
    B, C, Cr, H, W = R.SHAPES[name]
    g = R.gen(14)
    x = R.quantised(g, B, C, H, W)
    assert R.tie_fraction(x) >= 0.5, (name, R.tie_fraction(x))
    dout = R.randn(g, B, C, H, W)
    for k in (3, 7):
        w = R.randn(g, 1, 2, k, k, scale=0.3)
        w[:, 1] += 0.5 * torch.sign(w[:, 1])                           # the max branch's taps are not small
        _sa_backward(x, w, dout, R.randn(g, 1, 2, k, k), f"ties k={k} {name} {R.SHAPES[name]}")


# ---------------------------------------------------------------------------------------------------------------- host checks
class _NoLaunch:
    """Stands in for the library while malformed calls are made: reaching it means a host check is missing."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: the wrapper would have launched")


def _bad_calls():
    B, C, Cr, H, W = 2, 6, 3, 4, 5
    z = lambda *s: torch.zeros(*s, device="cuda")
    x, w7, w3 = (B, C, H, W), (1, 2, 7, 7), (1, 2, 3, 3)
    sab = lambda x_=x, dout=x, amap=(B, 2, H, W), w=w7, dw=w7: (lambda ops: ops.spatial_attention_bwd(z(*x_), z(*dout), z(*amap), z(*w), z(*dw)))
    seb = lambda mean=(B, C), w1=(Cr, C), w2=(C, Cr), y=(B, C), dy=(B, C), dw1=(Cr, C), dw2=(C, Cr): (
        lambda ops: ops.se_gate_bwd(z(*mean), z(*w1), z(*w2), z(*y), z(*dy), z(*dw1), z(*dw2)))
    return {
        "sa_bwd: dout is not x's shape": sab(dout=(B, C, H, W + 1)),
        "sa_bwd: dout misses a batch": sab(dout=(B - 1, C, H, W)),
        "sa_bwd: map of another plane": sab(amap=(B, 2, H, W - 1)),
        "sa_bwd: map with one channel": sab(amap=(B, 1, H, W)),
        "sa_bwd: 5x5 kernel": sab(w=(1, 2, 5, 5), dw=(1, 2, 5, 5)),
        "sa_bwd: w with two outputs": sab(w=(2, 2, 3, 3), dw=(2, 2, 3, 3)),
        "sa_bwd: w not square": sab(w=(1, 2, 3, 7)),
        "sa_bwd: dw of the 3x3 size under a 7x7 w": sab(dw=w3),
        "sa_bwd: x is 3-D": sab(x_=(C, H, W), dout=(C, H, W)),
        "se_gate_bwd: mean is flat": seb(mean=(B * C,)),
        "se_gate_bwd: y of another width": seb(y=(B, C - 1)),
        "se_gate_bwd: dy of another batch": seb(dy=(B + 1, C)),
        "se_gate_bwd: dy is flat": seb(dy=(B * C,)),
        "se_gate_bwd: w1 of another width": seb(w1=(Cr, C + 1), dw1=(Cr, C + 1)),
        "se_gate_bwd: w2 transposed": seb(w2=(Cr, C), dw2=(Cr, C)),
        "se_gate_bwd: dw1 is not w1's shape": seb(dw1=(Cr - 1, C)),
        "se_gate_bwd: dw2 is not w2's shape": seb(dw2=(Cr, C)),
        "chan_scale: flat B*C scale with B > 1": lambda ops: ops.chan_scale(z(*x), z(B * C)),
        "chan_scale: C + 1 factors": lambda ops: ops.chan_scale(z(*x), z(C + 1)),
        "chan_scale: (C, B) scale": lambda ops: ops.chan_scale(z(*x), z(C, B)),
        "chan_scale: C factors folded as (2, C / 2)": lambda ops: ops.chan_scale(z(*x), z(2, C // 2)),
        "chan_scale: (B, C, 1, 1) scale": lambda ops: ops.chan_scale(z(*x), z(B, C, 1, 1)),
        "chan_scale: flat add_bc": lambda ops: ops.chan_scale(z(*x), z(C), add_bc=z(B * C)),
        "chan_scale: add_bc for one image": lambda ops: ops.chan_scale(z(*x), z(C), add_bc=z(1, C)),
        "chan_scale: add of another plane": lambda ops: ops.chan_scale(z(*x), z(C), add=z(B, C, H, W + 1)),
        "chan_dot: parameter out with B*C elements": lambda ops: ops.chan_dot(z(*x), z(*x), z(B * C)),
        "chan_dot: parameter out with C + 1 elements": lambda ops: ops.chan_dot(z(*x), z(*x), z(C + 1)),
        "chan_dot: operands differ": lambda ops: ops.chan_dot(z(*x), z(B, C, H, W + 1)),
        "se_gate: x is 3-D": lambda ops: ops.se_gate(z(C, H, W), z(Cr, C), z(C, Cr)),
        "se_gate: x is 2-D": lambda ops: ops.se_gate(z(B, C), z(Cr, C), z(C, Cr)),
        "se_gate: w2 transposed": lambda ops: ops.se_gate(z(*x), z(Cr, C), z(Cr, C)),
        "spatial_attention: x is 3-D": lambda ops: ops.spatial_attention(z(C, H, W), z(*w7)),
        "spatial_attention: x is 5-D": lambda ops: ops.spatial_attention(z(1, B, C, H, W), z(*w7)),
        "spatial_attention: 5x5 kernel": lambda ops: ops.spatial_attention(z(*x), z(1, 2, 5, 5)),
        "spatial_attention: flat gate": lambda ops: ops.spatial_attention(z(*x), z(*w7), z(B * C)),
    }


@pytest.mark.parametrize("what", list(_bad_calls()))
def test_malformed_calls_are_rejected_before_any_launch(what, monkeypatch):
    from bem import ops
    monkeypatch.setattr(ops, "lib", lambda: _NoLaunch())
    with pytest.raises(ValueError):
        _bad_calls()[what](ops)


def test_no_launch_stub_is_what_a_missing_check_would_hit(monkeypatch):
    """The stub does stand between the wrappers and the library: a well-formed call reaches it."""
    from bem import ops
    monkeypatch.setattr(ops, "lib", lambda: _NoLaunch())
    with pytest.raises(AssertionError, match="was reached"):
        ops.chan_scale(torch.zeros(2, 6, 4, 5, device="cuda"), torch.zeros(6, device="cuda"))


def test_training_forms_pass_the_checks_and_match_float64():
    """The callers in bem/autograd.py and bem/archs.py (GateAddFn, SEBlock, SpatialAttention; training and inference forms) at B = 2,
    where a per-parameter and a per-image scale differ: outputs and gradients against float64 autograd through the oracle."""
    import bem.archs as A
    from bem import autograd as ag
    from oracle import bem_oracle as O
    torch.manual_seed(15)
    g = R.gen(15)
    B, C, H, W = 2, 160, 8, 6
    x, dout = R.randn(g, B, C, H, W) + R.randn(g, 1, C, 1, 1), R.randn(g, B, C, H, W)

    def grads(fn, leaves, dt):
        leaves = [t.detach().clone().to(dt).requires_grad_() for t in leaves]
        out = fn(*leaves)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, dout.to(dt)))

    # x_tgt + gate * t
    t_, gate = R.randn(g, B, C, H, W), torch.nn.Parameter(dev(1 + 0.3 * R.randn(g, 1, C, 1, 1)))
    x_d, t_d = dev(x).requires_grad_(), dev(t_).requires_grad_()
    out = ag.GateAddFn.apply(t_d, gate, x_d)
    out.backward(dev(dout))
    r32, r64 = (grads(lambda t, gt, xt: xt + gt * t, [t_, gate.detach().cpu(), x], dt) for dt in (torch.float32, torch.float64))
    for i, (what, got) in enumerate((("out", out), ("dt", t_d.grad), ("dx_tgt", x_d.grad))):
        per_pixel(got, r32[(0, 1, 3)[i]], r64[(0, 1, 3)[i]], f"GateAddFn {what}")
    reduction(gate.grad, r32[2], r64[2], (dout.double() * t_.double()).abs().sum((0, 2, 3)).reshape(1, C, 1, 1), "GateAddFn dgate")
    # SE block, training form and inference gate
    se = A.SEBlock(C).cuda().train()
    with torch.no_grad():
        for p_ in se.parameters():
            p_.add_(dev(0.5 * R.randn(g, *p_.shape)))
    w1, w2 = se.fc[0].weight.detach().cpu(), se.fc[2].weight.detach().cpu()
    x_d = dev(x).requires_grad_()
    out = se(x_d)
    out.backward(dev(dout))
    fn = lambda x_, a, b: O.se_block_ref({"fc.0.weight": a, "fc.2.weight": b}, "", x_)
    r32, r64 = (grads(fn, [x, w1, w2], dt) for dt in (torch.float32, torch.float64))
    per_pixel(out, r32[0], r64[0], "SEBlock out")
    per_pixel(x_d.grad, r32[1], r64[1], "SEBlock dx")
    sab = R.se_gate_bwd(R.plane_mean(x.double())[0], w1.double(), w2.double(), R.chan_dot(dout.double(), x.double())[0])
    reduction(se.fc[0].weight.grad, r32[2], r64[2], sab["dw1_abs"], "SEBlock dW1")
    reduction(se.fc[2].weight.grad, r32[3], r64[3], sab["dw2_abs"], "SEBlock dW2")
    with torch.no_grad():
        per_pixel(se.eval()(dev(x)), r32[0], r64[0], "SEBlock out, inference form")
    # spatial attention
    sa = A.SpatialAttention(7).cuda().train()
    w = sa.conv.weight.detach().cpu()
    x_d = dev(x).requires_grad_()
    out = sa(x_d)
    out.backward(dev(dout))
    r32, r64 = both(R.spatial_attention_bwd, x, w, dout)
    per_pixel(out, r32["out"], r64["out"], "SpatialAttention out")
    per_pixel(x_d.grad, r32["dx"], r64["dx"], "SpatialAttention dx")
    reduction(sa.conv.weight.grad, r32["dw"], r64["dw"], r64["dw_abs"], "SpatialAttention dw")


# ---------------------------------------------------------------------------------------------------------------- module path
def test_dualbranch_gradients_at_shipped_width_vs_float64():
    """DecompDualBranch(n_feat=40, num_blocks=[1,1,1]) in train mode on 64x64: a 16x16 bottleneck with C = 160, Cr = 10.  The gradients of
    every cross_fusion_* / bottleneck_se* / spatial_attention* parameter against float64 autograd through O.dualbranch_ref (the float64
    patches of tests/stage2_yardstick.py), bound 2x the same oracle's f32 run, mean and max.  The net's input carries no gradient on either
    side of the comparison that the product defines (the frozen decomposition runs without a graph), so the first convolutions' weights
    stand in for it: their gradients are reached only through the dx of every block between them and the output."""
    import stage2_yardstick as Y
    from bem import ops
    from oracle import bem_oracle as O
    name = "DecompDualBranch"
    net = Y.build_arch(name, n_feat=40, num_blocks=(1, 1, 1))
    g = R.gen(16)
    with torch.no_grad():
        for k, p_ in net.named_parameters():
            if k.startswith("bottleneck_se"):
                p_.add_(0.3 * R.randn(g, *p_.shape))                  # gates away from sigmoid(~0)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    keys = [k for k in sd if k.startswith(("cross_fusion_", "bottleneck_se", "spatial_attention"))]
    assert len(keys) == 12 and sd["bottleneck_se.fc.0.weight"].shape == (10, 160)
    keys += ["first_conv.weight", "first_conv2.weight"]
    x = torch.cat([0.25 * torch.rand(1, 3, 64, 64, generator=g), torch.rand(1, 3, 64, 64, generator=g)], 1)
    dout = R.randn(g, 1, 3, 64, 64)

    def oracle_grads(dt, run):
        s = {k: v.to(dt) for k, v in sd.items()}
        for k in keys:
            s[k].requires_grad_()
        out = run(s, x.to(dt))
        return out.detach(), dict(zip(keys, torch.autograd.grad(out, [s[k] for k in keys], dout.to(dt))))

    o64, g64 = oracle_grads(torch.float64, lambda s, x_: Y.float64_ref(name, s, x_))
    o32, g32 = oracle_grads(torch.float32, lambda s, x_: Y.oracle(name, s, x_, O.selective_scan_ref))
    assert o64.dtype == torch.float64 and all(v.dtype == torch.float64 for v in g64.values())
    ops.bump_weight_epoch()
    net.cuda().train()
    out = net(dev(x))[-1]
    out.backward(dev(dout))
    named = dict(net.named_parameters())
    per_pixel(out, o32, o64, f"{name} n_feat 40 train-mode forward")
    for k in keys:
        per_pixel(named[k].grad, g32[k], g64[k], f"{name} n_feat 40 d {k}")
