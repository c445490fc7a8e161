"""fp64 restatements of the optimiser extras (include/mpgan_hip.h: mpgan_grad_norm, mpgan_adam_step_ex,
mpgan_ema_buffers) for the host and GPU tests.  Plain torch on the CPU, nothing from the library."""
import math

import numpy as np
import torch

import norm_ref as N


def grad_norm(g, grad_scale=1.0):
    """sqrt(sum (double)(fl32(g_i * grad_scale))^2) for an fp32 gradient (the product rounded to fp32 first, as Adam
    loads it); for an fp64 gradient the product stays fp64.  Returns a python float."""
    if g.dtype == torch.float32:
        x = (g * torch.tensor(grad_scale, dtype=torch.float32)).double()
    else:
        x = g.double() * grad_scale
    return math.sqrt(float((x * x).sum()))


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient, in fp64: min(1, max_norm / (norm + 1e-6)); 1 without a bound."""
    if max_norm is None or not max_norm > 0:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def clip_coef_f32(norm_f32, max_norm):
    """The same formula in fp32 arithmetic on an fp32 norm (what the kernel evaluates): a numpy float32."""
    if max_norm is None or not max_norm > 0:
        return np.float32(1.0)
    c = np.float32(max_norm) / (np.float32(norm_f32) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else c


def adam_step_coef(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, coef=1.0):
    """Adam on fp64 copies with the gradient g * grad_scale * coef: returns (p, m, v)."""
    return N.adam_step(p, g * coef, m, v, lr, b1, b2, eps, step, grad_scale)


def lerp(e, p, w):
    """e + w * (p - e), the exact value both of torch's lerp forms round."""
    return e + w * (p - e)


def ema_decay_at(step, decay, warmup):
    if not warmup:
        return decay
    t = step - 1
    return min(decay, (1.0 + t) / (10.0 + t))


def ema_buffers(src, dst, w):
    """The buffer update: floating buffers are lerped towards src, integer ones copied.  Returns the new dst list."""
    return [lerp(d.double(), s.double(), w) if s.dtype.is_floating_point else s.clone() for s, d in zip(src, dst)]


def ulp32(x):
    """One fp32 unit in the last place at |x| (numpy float64)."""
    return float(np.spacing(np.float32(abs(x))))


def ema_bound(e, p, steps=1):
    """|err| <= steps * 6 * 2^-24 * max(|e|, |p|) + 1e-38: three roundings per step (the difference, the product, the
    sum), each of a quantity <= 2 * max; the map contracts, so the errors of chained steps add at most."""
    return steps * 6.0 * 2.0 ** -24 * torch.maximum(e.abs().double(), p.abs().double()) + 1e-38
