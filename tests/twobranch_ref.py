"""Oracle restatements of the Stage-II archs without a decomposition (not collected by pytest):

  vmunet_ref            basicsr/archs/VMUnet_arch.py:212-240
  naive_twobranch_ref   basicsr/archs/TwoBranchNaive_arch.py:231-271
  tunedmodel_ref        basicsr/archs/TunedModel_arch.py:367-409
  fusedtunedmodel_ref   basicsr/archs/FusedModel_arch.py:281-332

Built from the pieces of oracle.bem_oracle, with its Stage-II signature ``stage2(sd, x, scan)``, so they plug into
oracle.train_step_ref(stage2=...) and oracle.eval_mc_ref(stage2=...) unchanged.
"""
from unittest import mock

import torch
import torch.nn.functional as F

from oracle import bem_oracle as O


def _encode(sd, s_, x, scan):
    nl = O._levels(sd, f"down_layers{s_}.") + 1
    f = F.conv2d(x, sd[f"first_conv{s_}.weight"], sd[f"first_conv{s_}.bias"], padding=1)
    sk = []
    for i in range(nl - 1):
        f = O._blocks(sd, f"encoders{s_}.{i}.", f, None, scan)
        sk.append(f)
        f = F.conv2d(f, sd[f"down_layers{s_}.{i}.weight"], None, stride=2, padding=1)
    return f, sk


def _decode(sd, s_, f, sk, scan):
    nl = len(sk) + 1
    for j in range(nl - 1):
        d = f"decoders{s_}.{j}."
        f = F.conv_transpose2d(f, sd[d + "up.weight"], sd[d + "up.bias"], stride=2)
        f = F.conv2d(torch.cat([f, sk[nl - 2 - j]], 1), sd[d + "fuse.weight"])
        f = O._blocks(sd, d + "block.", f, None, scan)
    return F.conv2d(f, sd[f"proj{s_}.weight"], sd[f"proj{s_}.bias"], padding=1)


def _attn(sd, s_, f, scan):
    """bottleneck, SE block, spatial attention (TunedModel_arch.py:376-378)."""
    f = O._blocks(sd, f"bottleneck{s_}.", f, None, scan)
    return O.spatial_attention_ref(sd, f"spatial_attention{s_}.", O.se_block_ref(sd, f"bottleneck_se{s_}.", f))


def fusion_ref(sd, o1, o2):
    """fusion = Sequential(Conv2d(6,3,3,p=1), ReLU, Conv2d(3,3,3,p=1)) on cat(o1, o2) (TunedModel_arch.py:315-319,406)."""
    h = torch.relu(F.conv2d(torch.cat([o1, o2], 1), sd["fusion.0.weight"], sd["fusion.0.bias"], padding=1))
    return F.conv2d(h, sd["fusion.2.weight"], sd["fusion.2.bias"], padding=1)


def vmunet_ref(sd, x, scan=O.selective_scan_ref):
    f, sk = _encode(sd, "", x, scan)
    return _decode(sd, "", O._blocks(sd, "bottleneck.", f, None, scan), sk, scan)


def naive_twobranch_ref(sd, x, scan=O.selective_scan_ref):
    outs = []
    for s_ in ("", "2"):
        f, sk = _encode(sd, s_, x, scan)
        outs.append(_decode(sd, s_, O._blocks(sd, f"bottleneck{s_}.", f, None, scan), sk, scan))
    return (outs[0] + outs[1]) / 2.0


def tunedmodel_ref(sd, x, scan=O.selective_scan_ref):
    outs = []
    for s_ in ("", "2"):
        f, sk = _encode(sd, s_, x, scan)
        outs.append(_decode(sd, s_, _attn(sd, s_, f, scan), sk, scan))
    return fusion_ref(sd, *outs)


def fusedtunedmodel_ref(sd, x, scan=O.selective_scan_ref):
    f1, sk1 = _encode(sd, "", x, scan)
    f2, sk2 = _encode(sd, "2", x, scan)
    f2 = O.cross_fusion_ref(sd, "cross_fusion_12.", f1, f2)          # branch 2 from branch 1 first (FusedModel_arch.py:299-300)
    f1 = O.cross_fusion_ref(sd, "cross_fusion_21.", f2, f1)
    outs = [_decode(sd, s_, _attn(sd, s_, f, scan), sk, scan) for s_, f, sk in (("", f1, sk1), ("2", f2, sk2))]
    return fusion_ref(sd, *outs)


REFS = {"VMUNet": vmunet_ref, "NaiveVMUNetTwoBranch": naive_twobranch_ref, "TunedModel": tunedmodel_ref, "FusedTunedModel": fusedtunedmodel_ref}
TAGS = {"VMUNet": "vmunet", "NaiveVMUNetTwoBranch": "naive", "TunedModel": "tuned", "FusedTunedModel": "fused"}


def build(name, n_feat=40, num_blocks=(2, 2, 2), d_state=(1, 1, 1), seed=100):
    import bem.archs as A
    torch.manual_seed(seed)
    return getattr(A, name)(in_channels=6, out_channels=3, n_feat=n_feat, d_state=list(d_state), ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp",
                            use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=list(num_blocks))


def float64_ref(name, sd, x):
    """The restatement in float64 (the scans by the blocked closed form of tests/stage2_yardstick.py): the yardstick."""
    import stage2_yardstick as Y
    with mock.patch.object(O, "ss2d_core_ref", Y.ss2d_core64):
        r = REFS[name]({k: v.double() for k, v in sd.items()}, x.double(), None)
    assert r.dtype == torch.float64
    return r
