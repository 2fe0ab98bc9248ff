"""Reference for the averaged weights (train.ema_decay; basicsr/models/base_model.py:77-84):

    net_g_ema_params[k].data.mul_(decay).add_(net_g_params[k].data, alpha=1 - decay)

``constants`` are the two f32 numbers that line hands to torch's kernels; ``update_f64`` is one update in float64 with those constants
taken as given (exact to 1e-16, the yardstick of the kernel test); ``bound`` is the kernel's derived error bound against it;
``torch_update_`` replays the reference line itself on CPU tensors (the yardstick of the model tests)."""
import numpy as np
import torch

EPS = 2.0 ** -23


def constants(decay):
    """((float)decay, (float)(1 - decay)) as Python floats: a Python scalar reaches a float32 tensor op rounded once from the double."""
    return float(np.float32(decay)), float(np.float32(1.0 - float(decay)))


def update_f64(ema, p, decay_f32, one_minus_f32):
    """decay_f32 * ema + one_minus_f32 * p in float64: (result, |decay_f32 * ema| + |one_minus_f32 * p|)."""
    a, b = float(decay_f32) * ema.double(), float(one_minus_f32) * p.double()
    return a + b, a.abs() + b.abs()


def bound(mag):
    """The kernel's bound: |got - update_f64| <= 2^-23 (|decay ema| + |(1 - decay) p|).  It computes fmaf(1 - decay, p, decay * ema): the
    product decay * ema rounded (<= 2^-24 |decay ema|), then the fused multiply-add rounded once (<= 2^-24 |result|, and |result| is at
    most the magnitude sum): two roundings of at most half an ulp of the magnitude sum each."""
    return EPS * mag


def bound_unfused(mag):
    """torch's pair on the CPU may also round the second product: three roundings, each at most 2^-24 of a value that is at most
    (1 + 2^-23) times the magnitude sum."""
    return 3 * 2.0 ** -24 * (1 + 2.0 ** -20) * mag


def torch_update_(ema, p, decay):
    """The reference's in-place pair on CPU float32 tensors."""
    return ema.mul_(decay).add_(p, alpha=1 - decay)


def replay(snapshots, decay, start):
    """The average after ``len(snapshots)`` updates from ``start``: {name: tensor}, and per name max_t |p_t| for the bound."""
    ema = {k: v.clone() for k, v in start.items()}
    peak = {k: torch.zeros_like(v) for k, v in start.items()}
    for snap in snapshots:
        for k in ema:
            torch_update_(ema[k], snap[k], decay)
            peak[k] = torch.maximum(peak[k], snap[k].abs())
    return ema, peak
