"""Writes tests/golden/g14_dstate.npz from the reference (VMamba SS2D with d_state > 1), on CPU.

  python tests/golden/make_golden_dstate.py

Same recipe as G4 of make_golden.py: a reference VSSBlock at C = 40, 16x12, with perturbed norms / biases / Ds, its output, the
input gradient and the parameter gradients for a fixed dout -- here for ssm_d_state = 4 and 16.  Plus the state-dict key / shape
list of a full-width reference DecompDualBranch2DDWavelet built with d_state = [1, 4, 16].
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402
from make_golden import save  # noqa: E402


def main():
    ns = rh.load()
    vm = ns.vmamba
    out = {}
    for N in (4, 16):
        print(f"VSSBlock d_state={N}")
        torch.manual_seed(100 + N)
        blk = vm.VSSBlock(hidden_dim=40, drop_path=0, norm_layer=vm.LayerNorm2d, channel_first=True, ssm_d_state=N,
                          ssm_ratio=1, ssm_dt_rank="auto", ssm_act_layer=torch.nn.SiLU, ssm_conv=3, ssm_conv_bias=False,
                          ssm_drop_rate=0, ssm_init="v0", forward_type="v05_noz", mlp_ratio=4,
                          mlp_act_layer=torch.nn.GELU, mlp_drop_rate=0.0, mlp_type="gdmlp", use_checkpoint=False,
                          post_norm=False)
        g = torch.Generator().manual_seed(30 + N)
        with torch.no_grad():
            for n, p_ in blk.named_parameters():
                if "norm" in n or n.endswith("bias") or n.endswith("Ds"):
                    p_.add_(0.1 * torch.randn(p_.shape, generator=g))
        x = torch.randn(2, 40, 16, 12, generator=g).requires_grad_()
        y = blk(x)
        dout = torch.randn(y.shape, generator=g)
        params = dict(blk.named_parameters())
        pick = ["op.x_proj_weight", "op.A_logs", "op.dt_projs_bias", "op.Ds", "op.in_proj.weight"]
        grads = torch.autograd.grad(y, [x] + [params[k] for k in pick], dout)
        tag = f"n{N}"
        out[f"sd_{tag}"] = blk.state_dict()
        out[f"grads_{tag}"] = {k: v for k, v in zip(pick, grads[1:])}
        out[f"x_{tag}"], out[f"y_{tag}"], out[f"dout_{tag}"], out[f"dx_{tag}"] = x, y, dout, grads[0]
    kw = dict(in_channels=6, out_channels=3, n_feat=40, d_state=[1, 4, 16], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp",
              use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[2, 2, 2])
    torch.manual_seed(100)
    with rh.ref_ctor_env():
        net = ns.ddw.DecompDualBranchDDWavelet(decomp_model="model4", **kw)
    out["contract_ddw_1_4_16"] = np.array([f"{k}|{','.join(map(str, v.shape))}" for k, v in net.state_dict().items()])
    save("g14_dstate", **out)


if __name__ == "__main__":
    main()
