"""torch-CPU restatement of LPIPS v0.1 with the AlexNet trunk (spatial=False, eval mode), in any dtype: the checker of bem.lpips, written
from the definition (Zhang et al. 2018, "The Unreasonable Effectiveness of Deep Features as a Perceptual Metric"; Krizhevsky 2014 for
the trunk): scaling layer, five convolutions each followed by a ReLU with a 3x3 stride-2 max pool before the second and the third,
unit-normalised features, squared differences weighted by a non-negative 1x1 layer, spatial mean, sum over layers.
The product package never imports it."""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
# (torchvision ``features`` index, cin, cout, kernel, stride, pad, pool before it)
CONVS = ((0, 3, 64, 11, 4, 2, False), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, True), (8, 384, 256, 3, 1, 1, False),
         (10, 256, 256, 3, 1, 1, False))
WIDTHS = tuple(c[2] for c in CONVS)
ALEXNET_FILE, LIN_FILE = "alexnet-owt-7be5be79.pth", "alex.pth"


def seeded_state_dicts(seed=0, dtype=torch.float32):
    """(AlexNet state dict, lin state dict) in the packages' key layout: Kaiming-normal (fan_out, relu) convolutions, biases 0.05 N(0,1),
    lin weights U(0,1) * 2 / C (non-negative, as trained LPIPS weights are)."""
    g = torch.Generator().manual_seed(seed)
    sd, lin = {}, {}
    for i, (idx, cin, cout, k, _, _, _) in enumerate(CONVS):
        sd[f"features.{idx}.weight"] = (torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cout * k * k)) ** 0.5).to(dtype)
        sd[f"features.{idx}.bias"] = (torch.randn(cout, generator=g) * 0.05).to(dtype)
        lin[f"lin{i}.model.1.weight"] = (torch.rand(1, cout, 1, 1, generator=g) * 2.0 / cout).to(dtype)
    return sd, lin


def sizes(n):
    """Extent of the five features along one axis of length n (floor mode throughout)."""
    a = (n + 4 - 11) // 4 + 1
    b = (a - 3) // 2 + 1
    c = (b - 3) // 2 + 1
    return a, b, c, c, c


def img_as_ubyte(x01):
    """skimage.img_as_ubyte of a float32 image in [0,1], as numpy evaluates it: rint(clip(x,0,1) * 255) in float32."""
    return np.rint(np.clip(np.asarray(x01, np.float32), 0, 1) * np.float32(255)).astype(np.uint8)


def im2tensor(u8_hw3, dtype=torch.float64):
    return (torch.from_numpy(np.array(u8_hw3)).to(dtype) / 127.5 - 1).permute(2, 0, 1)[None]


def features(sd, x):
    """The five ReLU outputs for x (B,3,H,W) in [-1,1], in the dtype of x."""
    dt = x.dtype
    x = (x - torch.tensor(SHIFT, dtype=dt).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dt).view(1, 3, 1, 1)
    out = []
    for idx, _, _, _, stride, pad, pool in CONVS:
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = torch.relu(F.conv2d(x, sd[f"features.{idx}.weight"].to(dt), sd[f"features.{idx}.bias"].to(dt), stride=stride, padding=pad))
        out.append(x)
    return out


def head(y0, y1, w):
    """One layer: y0, y1 (B,C,h,w), w (C) -> (B)."""
    n0 = y0 / (y0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = y1 / (y1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((n0 - n1).pow(2) * w.to(y0.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips(sd, lin, in0, in1, dtype=torch.float64):
    """d(in0, in1) for tensors in [-1,1] -> (B) in ``dtype``."""
    f0, f1 = features(sd, in0.to(dtype)), features(sd, in1.to(dtype))
    return sum(head(a, b, lin[f"lin{i}.model.1.weight"].reshape(-1)) for i, (a, b) in enumerate(zip(f0, f1)))


def lpips01(sd, lin, ref01, pred01, dtype=torch.float64):
    """The driver's call: float images (B,3,H,W) in [0,1] through img_as_ubyte and im2tensor."""
    q = lambda t: torch.from_numpy(img_as_ubyte(t.numpy()).astype(np.float64)).to(dtype) / 127.5 - 1
    return lpips(sd, lin, q(ref01), q(pred01), dtype)
