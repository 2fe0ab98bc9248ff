"""QD model3's attention dropout (QD/model3.py:98,124-131) as the fold kernel applies it, on the host: the fold identity the GPU test
checks the kernel against, the CPU model of the in-kernel keep flags, and the stream-id key space of the draws."""
import numpy as np
import torch

import model3_train_ref as R
import philox_ref as P


def test_masked_fold_identity_float64():
    """Dropout on the softmaxed maps commutes with the fold: everything behind the softmax is linear in the map.  The module written out
    (model3.py:100-142 + the fuse conv) against W_b [f1; f2] + bias_b with the mask applied at the softmax, both float64."""
    f1, f2, w, fw, fb, mask = R.random_case(3, 6, 10, seed=0)
    assert 0 < float(mask.mean()) < 1
    want = R.direct(f1, f2, w, fw, fb, mask, 0.1)
    Wb, bias = R.folded(f1, f2, w, fw, fb, mask, 0.1)
    got = R.apply_folded(Wb, bias, f1, f2)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the mask matters, and an all-ones mask with p = 0 is the eval form
    plain = R.direct(f1, f2, w, fw, fb)
    assert float((plain - want).abs().max()) > 1e-3 * float(want.abs().max())
    ones = R.folded(f1, f2, w, fw, fb, torch.ones_like(mask), 0.0)
    none = R.folded(f1, f2, w, fw, fb)
    assert torch.equal(ones[0], none[0]) and torch.equal(ones[1], none[1])


SEED, STREAM = R.SEED, R.STREAM                 # the GPU test draws with these; the bound below is what they were chosen against


def test_keep_mask_model():
    """The CPU model of the in-kernel keep flags: 16 384 draws at p = 0.1 keep 0.9 +- 5 sigma, sigma = sqrt(0.09 / 16384); the layout
    (element e -> word e & 3 of block e >> 2) restated element by element; images are consecutive element ranges."""
    m = R.keep_mask(8, 0.1, SEED, STREAM)
    assert m.shape == (8, 2, 32, 32) and m.dtype == np.float32 and set(np.unique(m)) == {0.0, 1.0}
    assert abs(float(m.mean()) - 0.9) <= 5 * (0.09 / 16384) ** 0.5, float(m.mean())
    flat = m.reshape(-1)
    for e in (0, 1, 2, 3, 4, 1023, 1024, 2047, 2048, 16383):
        c = P.philox4x32_10((e >> 2, 0, STREAM & 0xFFFFFFFF, STREAM >> 32), (SEED & 0xFFFFFFFF, SEED >> 32))[:, 0]
        u = np.float32(int(c[e & 3]) >> 8) * np.float32(2.0 ** -24)
        assert flat[e] == float(u >= np.float32(0.1)), e
    assert np.array_equal(R.keep_mask(1, 0.1, SEED, STREAM, b0=2), m[2:3])
    assert np.array_equal(R.keep_mask(8, 0.0, SEED, STREAM), np.ones_like(m))               # u >= 0 always
    assert not np.array_equal(R.keep_mask(8, 0.1, SEED, STREAM + 1), m) and not np.array_equal(R.keep_mask(8, 0.1, SEED + 1, STREAM), m)


def test_stream_id_layout():
    """bit 61 | rank << 44 | iteration << 8 | call: iterations, ranks and calls never share an id, and the ids meet neither the weight
    samples' (SampleCtx.next_stream: rank << 44 | epoch << 20 | counter, below bit 60) nor the condition noise's (bit 62)."""
    from bem.archs import attn_drop_stream_id
    from bem.bayes import SampleCtx
    ids = {(r, it, c): attn_drop_stream_id(r, it, c) for r in (0, 1, 65535) for it in (0, 1, 2, 300000, (1 << 36) - 1) for c in (0, 1, 255)}
    assert len(set(ids.values())) == len(ids)
    for (r, it, c), v in ids.items():
        assert v == R.stream_id(r, it, c) and v < 1 << 62 and v >> 61 == 1 and not v & (1 << 62)
        assert (v >> 44) & 0xFFFF == r and (v >> 8) & ((1 << 36) - 1) == it and v & 255 == c
    assert attn_drop_stream_id(0, 5) != attn_drop_stream_id(0, 6) != attn_drop_stream_id(1, 6)
    assert attn_drop_stream_id(0, 5, 0) != attn_drop_stream_id(0, 5, 1)
    weight_ids = []
    for rank in (0, 65535):
        for epoch in (1, (1 << 24) - 1):
            ctx = SampleCtx(1, seed=0, rank=rank, epoch=epoch)
            weight_ids += [ctx.next_stream(), ctx.next_stream()]
            ctx.counter = (1 << 20) - 2
            weight_ids.append(ctx.next_stream())
    assert max(weight_ids) < 1 << 60 and all(P.stream_id(0, 1, 1) != v for v in ids.values())
    assert not set(weight_ids) & set(ids.values())
    assert all(v != P.noise_stream_id(r, e) for v in ids.values() for r in (0, 65535) for e in (0, 1, (1 << 24) - 1))
    for bad in ((1 << 16, 0, 0), (0, 1 << 36, 0), (0, 0, 256), (-1, 0, 0)):
        try:
            attn_drop_stream_id(*bad)
        except ValueError:
            continue
        raise AssertionError(f"attn_drop_stream_id{bad} was accepted")


def test_decomp_passes_drop_only_in_train_mode():
    """The host-side decision, without a device: cross_attn.p is 0.1 for model3 alone and adds nothing to the state dict; drop is handed
    to the fold iff the module is in train() mode, for both output domains; the record counts the calls of one forward."""
    from bem.archs import AttnDrop, Decomp, attn_drop_stream_id
    for model in ("model1", "model2", "model3", "model4"):
        for wav in (True, False):
            d = Decomp(model, wavelet_out=wav)
            assert d.cross_attn.p == (0.1 if model == "model3" else 0.0)
            assert not any("attn_drop" in k or k.endswith(".p") for k in d.state_dict())
            d.eval()
            assert d._next_drop() is None
            d.train()
            with torch.no_grad():
                first = d._next_drop()
            if model != "model3":
                assert first is None
                continue
            second = d._next_drop()
            assert first[0] == second[0] == 0.1 and first[2] != second[2] and first[2] >> 61 == 1         # no record: fresh stream every call
            d.attn_drop = AttnDrop(5, attn_drop_stream_id(3, 9))
            assert d._next_drop() == (0.1, 5, attn_drop_stream_id(3, 9, 0)) and d._next_drop() == (0.1, 5, attn_drop_stream_id(3, 9, 1))
            masks = [torch.ones(1, 2, 32, 32), torch.zeros(1, 2, 32, 32)]
            d.attn_drop = AttnDrop(masks=masks)
            assert d._next_drop()[1] is masks[0] and d._next_drop()[1] is masks[1]
