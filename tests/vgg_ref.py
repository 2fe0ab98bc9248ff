"""torch-CPU restatement of the VGG19 feature extractor and the perceptual loss (criterion l1), in any dtype, built from layer
names: the checker of bem.percep, written from the definition of configuration E (Simonyan & Zisserman 2015, table 1: 3x3 pad-1
convolutions 2x64, 2x128, 4x256, 4x512, 4x512, each followed by a ReLU, a 2x2 stride-2 max pool after every block) and of the loss
(sum over layers of layer_weight * mean |f(x) - f(gt)|, times perceptual_weight).  The product package never imports it."""
import torch
import torch.nn.functional as F

WIDTHS = (64, 128, 256, 512, 512)
DEPTHS = (2, 2, 4, 4, 4)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def layer_table():
    """[(name, kind, torchvision ``features`` index, cin, cout)] for the whole net, in order."""
    rows, cin, idx = [], 3, 0
    for b, (width, depth) in enumerate(zip(WIDTHS, DEPTHS), start=1):
        for j in range(1, depth + 1):
            rows.append((f"conv{b}_{j}", "conv", idx, cin, width))
            rows.append((f"relu{b}_{j}", "relu", idx + 1, width, width))
            cin, idx = width, idx + 2
        rows.append((f"pool{b}", "pool", idx, width, width))
        idx += 1
    return rows


def seeded_state_dict(upto, seed=0, dtype=torch.float32):
    """Kaiming-normal (fan_out, relu) weights and small non-zero biases for every convolution up to layer ``upto``, keyed like
    torchvision's state dict."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, kind, idx, cin, cout in layer_table():
        if kind == "conv":
            sd[f"features.{idx}.weight"] = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cout * 9)) ** 0.5).to(dtype)
            sd[f"features.{idx}.bias"] = (torch.randn(cout, generator=g) * 0.05).to(dtype)
        if name == upto:
            return sd
    raise ValueError(upto)


def features(sd, x, wanted, use_input_norm=True, range_norm=False):
    """{name: feature} for the names in ``wanted``; 'conv*' before its ReLU.  x (B,3,H,W) in the dtype of the computation."""
    dt = x.dtype
    if range_norm:
        x = (x + 1) / 2
    if use_input_norm:
        x = (x - torch.tensor(MEAN).view(1, 3, 1, 1).to(dt)) / torch.tensor(STD).view(1, 3, 1, 1).to(dt)
    wanted, out = set(wanted), {}
    for name, kind, idx, _, _ in layer_table():
        if kind == "conv":
            x = F.conv2d(x, sd[f"features.{idx}.weight"].to(dt), sd[f"features.{idx}.bias"].to(dt), padding=1)
        elif kind == "relu":
            x = torch.relu(x)
        else:
            x = F.max_pool2d(x, 2, 2)
        if name in wanted:
            out[name] = x
        if len(out) == len(wanted):
            return out
    raise ValueError(f"unknown layer among {sorted(wanted)}")


def perceptual_loss(sd, x, gt, layer_weights, perceptual_weight=1.0, **norm):
    fx, fg = features(sd, x, layer_weights, **norm), features(sd, gt, layer_weights, **norm)
    total = 0
    for k, w in layer_weights.items():
        total = total + (fx[k] - fg[k]).abs().mean() * w
    return total * perceptual_weight


def loss_and_grad(sd, x, gt, layer_weights, perceptual_weight=1.0, dtype=torch.float64, **norm):
    """(loss, d loss / d x) computed in ``dtype`` on the CPU."""
    x = x.detach().to(dtype).requires_grad_(True)
    loss = perceptual_loss(sd, x, gt.detach().to(dtype), layer_weights, perceptual_weight, **norm)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g
