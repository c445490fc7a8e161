"""Differentiable augmentation in front of the discriminator (Zhao et al. 2020, "Differentiable Augmentation for
Data-Efficient GAN Training"): the same random transformation T on everything D sees, differentiable so that
the generator's gradient flows back through it.  One channel: brightness and contrast ("color"; the paper's saturation
does not exist), an integer translation and a cut-out box, applied in that order by csrc/diffaug.hip.

    params = sample_params(x.shape[0], x.shape[2:], "color,translation,cutout", device=x.device)
    y = diff_augment(x, params)                     # (B, 1, *S) fp32 on the GPU; dL/dx through the backward kernel
    c = diff_augment(cond, params, color=False)     # the spatial ops alone, the same shift and box
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch
import torch.nn as nn

from . import ops

BRIGHTNESS, CONTRAST, TRANSLATION, CUTOUT = (ops.DIFFAUG_BRIGHTNESS, ops.DIFFAUG_CONTRAST, ops.DIFFAUG_TRANSLATION,
                                             ops.DIFFAUG_CUTOUT)
POLICY_BITS = {"color": BRIGHTNESS | CONTRAST, "translation": TRANSLATION, "cutout": CUTOUT}


class DiffAugParams(NamedTuple):
    """One draw: color (B, 2) float32 = [b, c]; geom (B, 9) int32 = [t_d, t_h, t_w, lo_d, lo_h, lo_w, size_d, size_h,
    size_w] (2-D: the D entries are 0, 0, 1); ops = the bit mask of what the policy enables."""
    color: torch.Tensor
    geom: torch.Tensor
    ops: int


def parse_policy(policy: str) -> int:
    """The ops bit mask of a comma-separated subset of "color", "translation", "cutout" ("" = 0)."""
    mask = 0
    for word in (w.strip() for w in str(policy).split(",")):
        if not word:
            continue
        if word not in POLICY_BITS:
            raise ValueError(f"diff_augment policy: unknown word {word!r} (a comma-separated subset of {sorted(POLICY_BITS)})")
        mask |= POLICY_BITS[word]
    return mask


def translation_range(size: int) -> int:
    return int(size / 8 + 0.5)


def cutout_size(size: int) -> int:
    return int(size / 2 + 0.5)


def sample_params(n: int, spatial: Sequence[int], policy: str, generator: Optional[torch.Generator] = None,
                  device="cpu") -> DiffAugParams:
    """Draw the parameters of `n` samples of extent `spatial` ((H, W) or (D, H, W)) with the paper's formulas, in pure torch
    ops on `device` (no host sync): b = U[0,1) - 0.5, c = U[0,1) + 0.5; t_k = randint(-r_k, r_k + 1) with
    r_k = int(S_k/8 + 0.5); size_k = int(S_k/2 + 0.5), lo_k = randint(0, S_k + (1 - size_k % 2)) - size_k // 2.
    Draw order: one rand(n, 2) for color, then the translation's axes in order, then the cutout's axes in order; a
    disabled op draws nothing and leaves its neutral entries (b = 0, c = 1, t = 0, lo = 0, size = 0; in 2-D size_d is 1 all the same)."""
    spatial = tuple(int(s) for s in spatial)
    if len(spatial) not in (2, 3) or min(spatial) < 1:
        raise ValueError(f"sample_params: spatial must be (H, W) or (D, H, W) with extents >= 1, got {spatial}")
    mask = parse_policy(policy)
    device = torch.device(device)
    kw = dict(generator=generator, device=device)
    if mask & (BRIGHTNESS | CONTRAST):                 # (scalar updates of the columns: nothing is copied from the host)
        color = torch.rand((n, 2), dtype=torch.float32, **kw)
        color[:, 0] -= 0.5
        color[:, 1] += 0.5
    else:
        color = torch.zeros((n, 2), dtype=torch.float32, device=device)
        color[:, 1] = 1.0
    first = 3 - len(spatial)                           # 2-D: the D column keeps t = 0, lo = 0, size = 1
    zero = torch.zeros(n, dtype=torch.int64, device=device)
    cols = [zero] * 9
    if first:
        cols[6] = zero + 1
    if mask & TRANSLATION:
        for k, s in enumerate(spatial, first):
            r = translation_range(s)
            cols[k] = torch.randint(-r, r + 1, (n,), **kw)
    if mask & CUTOUT:
        for k, s in enumerate(spatial, first):
            size = cutout_size(s)
            cols[3 + k] = torch.randint(0, s + (1 - size % 2), (n,), **kw) - size // 2
            cols[6 + k] = zero + size
    return DiffAugParams(color.contiguous(), torch.stack(cols, 1).to(torch.int32).contiguous(), mask)


class _DiffAugFn(torch.autograd.Function):
    """y = T(x) by ops.diffaug_forward; the backward is ops.diffaug_backward on the same tables.  T is affine in x with
    coefficients that depend on the parameters alone, so only the two tables are saved, never x."""

    @staticmethod
    def forward(ctx, x, color, geom, mask, fill):
        x = x.contiguous()
        n, spatial = x.shape[0], tuple(x.shape[2:])
        ws = _workspace(x, n, spatial, mask)
        y = ops.diffaug_forward(x, mask, color, geom, fill, ws, torch.empty_like(x))
        ctx.mask = mask
        ctx.save_for_backward(color, geom)
        return y

    @staticmethod
    def backward(ctx, gy):
        color, geom = ctx.saved_tensors
        gy = gy.contiguous()
        ws = _workspace(gy, gy.shape[0], tuple(gy.shape[2:]), ctx.mask)
        gx = ops.diffaug_backward(gy, ctx.mask, color, geom, ws, torch.empty_like(gy))
        return gx, None, None, None, None


def _workspace(x, n, spatial, mask):
    if not mask & CONTRAST:
        return None
    return torch.empty(ops.diffaug_workspace(n, spatial) // 8, dtype=torch.float64, device=x.device)


def diff_augment(x: torch.Tensor, params: DiffAugParams, *, color: bool = True, fill: float = 0.0) -> torch.Tensor:
    """T(x) for a (B, 1, *S) fp32 GPU tensor under one draw of sample_params; differentiable in x.  color=False applies
    the spatial ops alone (what the condition of a conditional discriminator gets, under its image's parameters)."""
    mask = int(params.ops) if color else int(params.ops) & ~(BRIGHTNESS | CONTRAST)
    return _DiffAugFn.apply(x, params.color, params.geom, mask, float(fill))


class DiffAugment(nn.Module):
    """Draws fresh parameters on every call (`generator`: a torch.Generator on the input's device, or None for torch's
    global one; every rank of a data-parallel run seeds its own) and applies them: forward(x) -> T(x);
    forward(x, cond) -> (T(x), T_spatial(cond)) with the same parameters.  `.last_params` is the last draw.  The module
    has no parameters and no buffers."""

    def __init__(self, policy: str, fill: float = 0.0, generator: Optional[torch.Generator] = None):
        super().__init__()
        self.ops = parse_policy(policy)
        self.policy = str(policy)
        self.fill = float(fill)
        self.generator = generator
        self.last_params: Optional[DiffAugParams] = None

    def extra_repr(self):
        return f"policy={self.policy!r}, fill={self.fill}"

    def forward(self, x, cond=None):
        params = sample_params(x.shape[0], tuple(x.shape[2:]), self.policy, generator=self.generator, device=x.device)
        self.last_params = params
        y = diff_augment(x, params, fill=self.fill)
        if cond is None:
            return y
        return y, diff_augment(cond, params, color=False, fill=self.fill)
