"""Writes tests/golden/g15_twobranch_*.npz from the reference, on CPU: the Stage-II archs without a decomposition.

  python tests/golden/make_golden_twobranch.py

Per arch (VMUNet, NaiveVMUNetTwoBranch, TunedModel, FusedTunedModel) at reduced width (n_feat 16, num_blocks [1,1,1]), built under
a fixed seed with perturbed norms / biases / Ds: the state dict, a seeded (2,6,32,32) input and the output.  For the two tuned archs
also the operand (cat(out_1, out_2)) and the result of ``fusion``, recorded with a forward hook.  Plus the full-width (n_feat 40,
[2,2,2]) key / shape contract of all four, and one reduced-width TunedModel with d_state [1, 4, 16].

Every parameter is rounded to float16 BEFORE the reference runs and is stored as float16 (exact), one file per case: that keeps each
file under 1 MiB.  The tests widen them back to float32.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

ARCHS = (("vmunet", "VMUnet_arch", "VMUNet"), ("naive", "TwoBranchNaive_arch", "NaiveVMUNetTwoBranch"),
         ("tuned", "TunedModel_arch", "TunedModel"), ("fused", "FusedModel_arch", "FusedTunedModel"))


def _kw(n_feat, num_blocks, d_state):
    return dict(in_channels=6, out_channels=3, n_feat=n_feat, stage=1, num_blocks=num_blocks, d_state=d_state, ssm_ratio=1, mlp_ratio=4,
                mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False)


def _case(cls, tag, seed, d_state):
    torch.manual_seed(seed)
    with rh.ref_ctor_env():
        net = cls(**_kw(16, [1, 1, 1], d_state)).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p_ in net.named_parameters():
            if "norm" in n or n.endswith("bias") or n.endswith("Ds"):
                p_.add_(0.1 * torch.randn(p_.shape, generator=g))
        for t in net.state_dict().values():
            if t.is_floating_point():
                t.copy_(t.half().float())
    x = torch.rand(2, 6, 32, 32, generator=g)
    rec = {}
    if hasattr(net, "fusion"):
        net.fusion.register_forward_hook(lambda m, i, o: rec.update(fin=i[0].detach().clone(), fout=o.detach().clone()))
    with torch.no_grad(), rh._quiet():
        y = net(x)[-1]
    case = {"sd": {k: v.half() if v.is_floating_point() else v for k, v in net.state_dict().items()}, "x": x, "y": y}
    if rec:
        case["fusion_in"], case["fusion_out"] = rec["fin"], rec["fout"]
    _save(f"g15_twobranch_{tag}", case)


def _save(name, arrs):
    flat = {}
    for k, v in arrs.items():
        if isinstance(v, dict):
            flat.update({f"{k}/{kk}": vv.detach().cpu().numpy() for kk, vv in v.items()})
        else:
            flat[k] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **flat)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    rh.load()
    contract = {}
    for i, (tag, mod, name) in enumerate(ARCHS):
        cls = getattr(importlib.import_module(f"basicsr.archs.{mod}"), name)
        _case(cls, tag, 200 + 10 * i, [1, 1, 1])
        torch.manual_seed(100)
        with rh.ref_ctor_env():
            net = cls(**_kw(40, [2, 2, 2], [1, 1, 1]))
        contract[tag] = np.array([f"{k}|{','.join(map(str, v.shape))}" for k, v in net.state_dict().items()])
    _case(getattr(importlib.import_module("basicsr.archs.TunedModel_arch"), "TunedModel"), "tuned_n1_4_16", 300, [1, 4, 16])
    _save("g15_twobranch_contract", contract)


if __name__ == "__main__":
    main()
