"""Differentiable augmentation in front of the discriminator (Zhao et al. 2020, "Differentiable Augmentation for
Data-Efficient GAN Training"): the same random transformation T on everything D sees, differentiable so that
the generator's gradient flows back through it.  One channel: brightness and contrast ("color"; the paper's saturation
does not exist), an integer translation and a cut-out box, applied in that order by csrc/diffaug.hip.  The policy word
"affine" (Karras et al. 2020 found rotation and isotropic scaling the most effective augmentations for
small data sets) puts a random rotation, scale, shift and flip in front of those: diff_affine_warp, the trilinear warp
of csrc/pair_augment.hip with its exact adjoint as the backward.

    params = sample_params(x.shape[0], x.shape[2:], "color,affine,translation,cutout", device=x.device)
    y = diff_augment(x, params)                     # (B, 1, *S) fp32 on the GPU; dL/dx through the backward kernels
    c = diff_augment(cond, params, color=False)     # the spatial ops alone, the same map, shift and box
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch
import torch.nn as nn

from . import ops

BRIGHTNESS, CONTRAST, TRANSLATION, CUTOUT = (ops.DIFFAUG_BRIGHTNESS, ops.DIFFAUG_CONTRAST, ops.DIFFAUG_TRANSLATION,
                                             ops.DIFFAUG_CUTOUT)
AFFINE = 16                                           # this module's own bit: diff_augment warps, then strips it
POLICY_BITS = {"color": BRIGHTNESS | CONTRAST, "translation": TRANSLATION, "cutout": CUTOUT, "affine": AFFINE}
AFFINE_KEYS = ("rotate", "scale", "shift", "flip", "prob")       # the sample_affine_params keywords "affine" may set
DEFAULT_AFFINE = dict(rotate=0.26, scale=0.1)         # +-15 degrees about every axis, +-10 % isotropic zoom


class DiffAugParams(NamedTuple):
    """One draw: color (B, 2) float32 = [b, c]; geom (B, 9) int32 = [t_d, t_h, t_w, lo_d, lo_h, lo_w, size_d, size_h,
    size_w] (2-D: the D entries are 0, 0, 1); ops = the bit mask of what the policy enables; theta (B, 12) float64, the
    (A | t) of AffineParams, with the policy word "affine" and None without it."""
    color: torch.Tensor
    geom: torch.Tensor
    ops: int
    theta: Optional[torch.Tensor] = None


def parse_policy(policy: str) -> int:
    """The ops bit mask of a comma-separated subset of "color", "affine", "translation", "cutout" ("" = 0)."""
    mask = 0
    for word in (w.strip() for w in str(policy).split(",")):
        if not word:
            continue
        if word not in POLICY_BITS:
            raise ValueError(f"diff_augment policy: unknown word {word!r} (a comma-separated subset of {sorted(POLICY_BITS)})")
        mask |= POLICY_BITS[word]
    return mask


def affine_options(policy: str, affine: Optional[dict] = None) -> Optional[dict]:
    """The sample_affine_params keywords behind the policy word "affine": None without the word (options given all the
    same are a ValueError), DEFAULT_AFFINE when `affine` is None, else a copy of `affine`, whose keys must come from
    AFFINE_KEYS and whose values some image must be able to take."""
    if not parse_policy(policy) & AFFINE:
        if affine is not None:
            raise ValueError(f"diff_augment policy: affine options {affine!r} without the word 'affine' in {str(policy)!r}")
        return None
    if affine is None:
        return dict(DEFAULT_AFFINE)
    unknown = sorted(set(affine) - set(AFFINE_KEYS)) if isinstance(affine, dict) else None
    if unknown is None or unknown:
        raise ValueError(f"diff_augment policy: the affine options are a dict of the keywords {AFFINE_KEYS}, got {affine!r}")
    _check_some_image(**affine)
    return dict(affine)


def _spatial(what: str, spatial) -> tuple:
    """The samplers' extent: (H, W) or (D, H, W) as a tuple of ints."""
    spatial = tuple(int(s) for s in spatial)
    if len(spatial) not in (2, 3) or min(spatial) < 1:
        raise ValueError(f"{what}: spatial must be (H, W) or (D, H, W) with extents >= 1, got {spatial}")
    return spatial


def translation_range(size: int) -> int:
    return int(size / 8 + 0.5)


def cutout_size(size: int) -> int:
    return int(size / 2 + 0.5)


def sample_params(n: int, spatial: Sequence[int], policy: str, generator: Optional[torch.Generator] = None,
                  device="cpu", affine: Optional[dict] = None) -> DiffAugParams:
    """Draw the parameters of `n` samples of extent `spatial` ((H, W) or (D, H, W)) with the paper's formulas, in pure torch
    ops on `device` (no host sync): b = U[0,1) - 0.5, c = U[0,1) + 0.5; t_k = randint(-r_k, r_k + 1) with
    r_k = int(S_k/8 + 0.5); size_k = int(S_k/2 + 0.5), lo_k = randint(0, S_k + (1 - size_k % 2)) - size_k // 2.
    Draw order: one rand(n, 2) for color, then the translation's axes in order, then the cutout's axes in order; a
    disabled op draws nothing and leaves its neutral entries (b = 0, c = 1, t = 0, lo = 0, size = 0; in 2-D size_d is 1 all the same).
    With the word "affine" theta = sample_affine_params(n, spatial, **affine).theta is drawn last, after the cutout (a
    replay of the other words from the same seed is unchanged); `affine`: keywords from AFFINE_KEYS, by default
    DEFAULT_AFFINE; given without the word it is a ValueError."""
    spatial = _spatial("sample_params", spatial)
    mask = parse_policy(policy)
    affine = affine_options(policy, affine)
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
    theta = None
    if affine is not None:
        theta = sample_affine_params(n, spatial, generator=generator, device=device, **affine).theta
    return DiffAugParams(color.contiguous(), torch.stack(cols, 1).to(torch.int32).contiguous(), mask, theta)


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
    the spatial ops alone (what the condition of a conditional discriminator gets, under its image's parameters).
    With the AFFINE bit x is first warped under params.theta (diff_affine_warp with `fill`), then the other ops run on
    the result; without other ops the warp's output is returned."""
    mask = int(params.ops) if color else int(params.ops) & ~(BRIGHTNESS | CONTRAST)
    if mask & AFFINE:
        if params.theta is None:
            raise ValueError("diff_augment: the AFFINE bit needs params.theta (sample_params with the word 'affine')")
        x = diff_affine_warp(x, params.theta, fill=fill)
        mask &= ~AFFINE
        if not mask:
            return x
    return _DiffAugFn.apply(x, params.color, params.geom, mask, float(fill))


class DiffAugment(nn.Module):
    """Draws fresh parameters on every call (`generator`: a torch.Generator on the input's device, or None for torch's
    global one; every rank of a data-parallel run seeds its own) and applies them: forward(x) -> T(x);
    forward(x, cond) -> (T(x), T_spatial(cond)) with the same parameters.  `.last_params` is the last draw.  The module
    has no parameters and no buffers.  `affine`: the options of the policy word "affine" (affine_options)."""

    def __init__(self, policy: str, fill: float = 0.0, generator: Optional[torch.Generator] = None,
                 affine: Optional[dict] = None):
        super().__init__()
        self.ops = parse_policy(policy)
        self.affine = affine_options(policy, affine)
        self.policy = str(policy)
        self.fill = float(fill)
        self.generator = generator
        self.last_params: Optional[DiffAugParams] = None

    def extra_repr(self):
        return f"policy={self.policy!r}, fill={self.fill}" + (f", affine={self.affine!r}" if self.affine is not None else "")

    def forward(self, x, cond=None):
        params = sample_params(x.shape[0], tuple(x.shape[2:]), self.policy, generator=self.generator, device=x.device,
                               affine=self.affine)
        self.last_params = params
        y = diff_augment(x, params, fill=self.fill)
        if cond is None:
            return y
        return y, diff_augment(cond, params, color=False, fill=self.fill)


# ---- paired affine augmentation of the training pair itself (csrc/pair_augment.hip) --------------------
# Not in front of D but on the data: the same random rotation, scale, shift and flips on t1w and t2w, Gaussian noise on
# the input, so that every term of the generator loss sees a new pair.  Runs under no_grad; there is no backward.
#
#     p = sample_affine_params(B, S, rotate=0.3, scale=0.1, shift=0.05, flip=(2,), noise_std=0.05, device=x.device)
#     t1, t2 = affine_warp(t1w, p.theta, t2w, noise=torch.randn_like(t1w), sigma=p.sigma)
#     batch = PairAugment(rotate=0.3, noise_std=0.05)(batch)        # the module: one draw, one launch, a new dict
WARP_MODES = {"constant": ops.WARP_CONSTANT, "border": ops.WARP_BORDER}
PAIR_KEYS = ("t1w", "t2w")                            # plane 0, plane 1


class AffineParams(NamedTuple):
    """One draw: theta (B, 12) float64, per sample the row-major 3 x 4 (A | t) in (d, h, w) voxel-index order (output
    voxel p samples the input at A p + t); sigma (B, 2) float32, the noise standard deviation of plane 0 and plane 1."""
    theta: torch.Tensor
    sigma: torch.Tensor


def _triple(value, ndim: int, what: str):
    """A number (every axis; for `rotate` in 2-D the in-plane angle) or one entry per axis -> a (d, h, w) triple."""
    if isinstance(value, (int, float)):
        vals = [float(value)] * ndim
    else:
        vals = [float(v) for v in value]
        if len(vals) != ndim:
            raise ValueError(f"{what}: one number or {ndim} of them, got {value!r}")
    if any(not v >= 0 for v in vals):
        raise ValueError(f"{what} must be >= 0, got {value!r}")
    return [0.0] * (3 - ndim) + vals


def _check_affine_options(rotate, scale, shift, flip, prob, noise_std, noise_prob, noise_planes, ndim: int):
    if isinstance(rotate, (int, float)) and ndim == 2:
        rot = [float(rotate), 0.0, 0.0]               # 2-D: the one angle is the in-plane one, about d
        if not rot[0] >= 0:
            raise ValueError(f"rotate must be >= 0, got {rotate!r}")
    elif ndim == 2:
        raise ValueError(f"rotate: a 2-D image has one angle, got {rotate!r}")
    else:
        rot = _triple(rotate, 3, "rotate")
    if not 0.0 <= float(scale) < 1.0:
        raise ValueError(f"scale must be in [0, 1), got {scale!r}")
    sh = _triple(shift, ndim, "shift")
    axes = sorted({int(a) % ndim if -ndim <= int(a) < ndim else -1 for a in flip})
    if axes and axes[0] < 0:
        raise ValueError(f"flip: axes of a {ndim}-D image, got {tuple(flip)!r}")
    for name, v in (("prob", prob), ("noise_prob", noise_prob)):
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"{name} must be in [0, 1], got {v!r}")
    if not float(noise_std) >= 0:
        raise ValueError(f"noise_std must be >= 0, got {noise_std!r}")
    planes = sorted({int(k) for k in noise_planes})
    if any(k not in (0, 1) for k in planes):
        raise ValueError(f"noise_planes: a subset of (0, 1), got {tuple(noise_planes)!r}")
    return rot, float(scale), sh, [a + 3 - ndim for a in axes], planes


def _check_some_image(rotate=0.0, scale=0.0, shift=0.0, flip=(), prob=1.0, noise_std=0.0, noise_prob=1.0, noise_planes=()):
    """ValueError unless some image, 2-D or 3-D, can take these options (the 3-D refusal is the one reported)."""
    try:
        _check_affine_options(rotate, scale, shift, flip, prob, noise_std, noise_prob, noise_planes, 2)
    except ValueError:
        _check_affine_options(rotate, scale, shift, flip, prob, noise_std, noise_prob, noise_planes, 3)


def sample_affine_params(n: int, spatial: Sequence[int], *, rotate=0.0, scale: float = 0.0, shift=0.0,
                         flip: Sequence[int] = (), prob: float = 1.0, noise_std: float = 0.0, noise_prob: float = 1.0,
                         noise_planes: Sequence[int] = (0,), generator: Optional[torch.Generator] = None,
                         device="cpu") -> AffineParams:
    """Draw the parameters of `n` samples of extent `spatial` ((H, W) or (D, H, W)), in pure torch ops on `device` (no host
    sync).  In (d, h, w) index order, with c = (S - 1) / 2 the centre of the extent (input and output alike):
        R = R_d R_h R_w,  R_d = [[1,0,0],[0,c,-s],[0,s,c]],  R_h = [[c,0,s],[0,1,0],[-s,0,c]],  R_w = [[c,-s,0],[s,c,0],[0,0,1]]
        A = F R / s,  t = c - A c + shift
    rotate: the largest |angle| in radians, one number or (about d, about h, about w); each angle is U[-r, r]; a 2-D
            image has the one in-plane angle (about d).
    scale:  a in [0, 1): s = 1 + a U[-1, 1]; s > 1 zooms in.
    shift:  a fraction f of each extent (one number or one per axis): U[-f S, f S] voxels, continuous.
    flip:   axes of `spatial` (0 = the first), each reversed with probability 0.5: F = diag(+-1).
    prob:   a sample keeps its spatial draw with this probability, else it gets exactly (I | 0): a bit copy.
    noise_std, noise_prob, noise_planes: for each listed plane sigma = noise_std U[0, 1) with probability noise_prob,
            else 0 (MONAI 0.4's RandGaussianNoise: the std is itself drawn); the other plane's sigma is 0.
    Draw order, one torch.rand each: rotate (n, 3) (2-D: (n, 1)), scale (n,), shift (n, ndim), flip (n, number of
    axes), the prob gate (n,) when prob < 1, then sigma (n, number of planes) and its gate (n, number of planes) when
    noise_prob < 1.  A disabled op (rotate 0, scale 0, shift 0, no flip axis, prob 1 or 0, noise_std 0, noise_prob 1 or
    0) draws nothing and leaves its neutral entry; with prob 0 no spatial op draws.  In 2-D the d row and column of A are (1, 0, 0) and t_d = 0."""
    return _sample_affine(n, spatial, rotate, scale, shift, flip, prob, noise_std, noise_prob, noise_planes, generator,
                          device)[0]


def _sample_affine(n, spatial, rotate, scale, shift, flip, prob, noise_std, noise_prob, noise_planes, generator, device):
    """sample_affine_params and the boolean (n,) gate of its `prob` draw (None when 0 < prob < 1 does not hold)."""
    spatial = _spatial("sample_affine_params", spatial)
    ndim = len(spatial)
    rot, a, sh, axes, planes = _check_affine_options(rotate, scale, shift, flip, prob, noise_std, noise_prob,
                                                     noise_planes, ndim)
    device = torch.device(device)
    kw = dict(generator=generator, device=device, dtype=torch.float64)
    S = (1,) * (3 - ndim) + spatial
    first = 3 - ndim
    zero, one = torch.zeros(n, dtype=torch.float64, device=device), torch.ones(n, dtype=torch.float64, device=device)
    ang = [zero, zero, zero]
    live = prob > 0.0                                 # prob 0: no spatial op is drawn at all
    if live and any(r > 0 for r in rot):
        u = torch.rand((n, 3 if ndim == 3 else 1), **kw)
        for k in range(u.shape[1]):
            ang[k] = (2.0 * u[:, k] - 1.0) * rot[k]
    s = one
    if live and a > 0:
        s = 1.0 + a * (2.0 * torch.rand((n,), **kw) - 1.0)
    t_shift = [zero, zero, zero]
    if live and any(f > 0 for f in sh):
        u = torch.rand((n, ndim), **kw)
        for k in range(ndim):
            t_shift[first + k] = (2.0 * u[:, k] - 1.0) * (sh[first + k] * S[first + k])
    F = [one, one, one]
    if live and axes:
        u = torch.rand((n, len(axes)), **kw)
        for j, k in enumerate(axes):
            F[k] = torch.where(u[:, j] < 0.5, -one, one)
    (cd, ch, cw), (sd, sh_, sw) = [torch.cos(x) for x in ang], [torch.sin(x) for x in ang]
    R = [[ch * cw, -ch * sw, sh_],
         [cd * sw + sd * sh_ * cw, cd * cw - sd * sh_ * sw, -sd * ch],
         [sd * sw - cd * sh_ * cw, sd * cw + cd * sh_ * sw, cd * ch]]
    A = [[F[i] * R[i][j] / s for j in range(3)] for i in range(3)]
    ctr = [(S[k] - 1) / 2.0 for k in range(3)]
    t = [ctr[i] - (A[i][0] * ctr[0] + A[i][1] * ctr[1] + A[i][2] * ctr[2]) + t_shift[i] for i in range(3)]
    if ndim == 2:
        A[0], t[0] = [one, zero, zero], zero
        A[1][0], A[2][0] = zero, zero
    theta = torch.stack([A[i][j] if j < 3 else t[i] for i in range(3) for j in range(4)], 1)
    gate = None
    if 0.0 < prob < 1.0:
        identity = torch.eye(3, 4, dtype=torch.float64, device=device).reshape(1, 12)
        gate = torch.rand((n,), **kw) < prob
        theta = torch.where(gate[:, None], theta, identity)
    sigma = torch.zeros((n, 2), dtype=torch.float32, device=device)
    if noise_std > 0 and planes and noise_prob > 0.0:
        draw = torch.rand((n, len(planes)), **kw) * float(noise_std)
        if noise_prob < 1.0:
            draw = torch.where(torch.rand((n, len(planes)), **kw) < noise_prob, draw, torch.zeros_like(draw))
        for j, k in enumerate(planes):
            sigma[:, k] = draw[:, j].to(torch.float32)
    return AffineParams(theta.contiguous(), sigma), gate


def affine_warp(x: torch.Tensor, theta: torch.Tensor, x1: Optional[torch.Tensor] = None, *, out_size=None,
                mode: str = "border", fill=-1.0, noise=None, sigma: Optional[torch.Tensor] = None):
    """The trilinear resampling of a (B, 1, *S) fp32 GPU tensor (and of `x1`, under the same map, in the same launch) at
    c = A p + t per sample, theta (B, 12) float64 = (A | t) in (d, h, w) voxel-index order; returns one tensor, or a pair
    with `x1`.  out_size: the output's spatial extent (default: the input's).  mode "border" clamps c to the image,
    "constant" gives a corner outside it the value `fill` (one number, or one per plane).  noise: a field of the
    output's shape for plane 0, or a pair (field or None, field or None); plane k then gets + sigma[:, k] * noise_k
    (sigma (B, 2) float32).  Not differentiable: an input that requires grad is refused."""
    planes, fills, noises, outs = _warp_arguments("affine_warp", x, x1, out_size, mode, fill, noise)
    ops.affine_warp(planes[0], planes[1], theta, WARP_MODES[mode], fills[0], fills[1], noises[0], noises[1], sigma,
                    outs[0], outs[1])
    return _planes_out(outs)


def _warp_io(what, x, x1, out_size, fill, differentiable: bool):
    """What every warp of this module makes of (x, x1, out_size, fill): the contiguous planes [x, x1] (detached unless
    `differentiable`; without it an input that requires grad under grad mode is refused), the two fills, and the new
    outputs [y, y1] of extent out_size.  x1 None stays None in both lists, which is how ops takes a single plane."""
    for t in (x,) if x1 is None else (x, x1):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{what}: every tensor must be on the GPU (there is no CPU path)")
        if not differentiable and t.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"{what}: not differentiable (an input requires grad); call it under torch.no_grad() "
                             "or on detached tensors")
    fills = (float(fill),) * 2 if isinstance(fill, (int, float)) else tuple(float(f) for f in fill)
    if len(fills) != 2:
        raise ValueError(f"{what}: fill is one number or one per plane, got {fill!r}")
    out_size = tuple(x.shape[2:]) if out_size is None else tuple(int(s) for s in out_size)
    if len(out_size) != x.dim() - 2:
        raise ValueError(f"{what}: out_size {out_size} for a {x.dim() - 2}-D image")
    planes = [None if t is None else (t if differentiable else t.detach()).contiguous() for t in (x, x1)]
    outs = [None if t is None else torch.empty((x.shape[0], 1, *out_size), dtype=torch.float32, device=x.device)
            for t in planes]
    return planes, fills, outs


def _planes_out(outs):
    return outs[0] if outs[1] is None else (outs[0], outs[1])


def _warp_arguments(what, x, x1, out_size, mode, fill, noise):
    """The checks affine_warp and deform_warp share: (detached contiguous planes, fills, noises, new outputs)."""
    planes, fills, outs = _warp_io(what, x, x1, out_size, fill, differentiable=False)
    if mode not in WARP_MODES:
        raise ValueError(f"{what}: mode must be one of {sorted(WARP_MODES)}, got {mode!r}")
    noises = [noise, None] if noise is None or isinstance(noise, torch.Tensor) else list(noise)
    if len(noises) != 2:
        raise ValueError(f"{what}: noise is one field (plane 0) or a pair")
    return planes, fills, noises, outs


# ---- the differentiable warp: what the policy word "affine" applies; affine_warp above is untouched ----------
class _AffineWarpFn(torch.autograd.Function):
    """(y, y1) = the CONSTANT warp of (x, x1) in one launch; the map is linear in the images with weights that depend on
    theta alone, so only theta is saved for them.  The backward launches ops.affine_warp_backward once per plane that
    needs a gradient.  A theta that requires grad also keeps the planes and gets ops.affine_warp_backward_theta's (B, 12)
    float64, one call over the planes that have an output gradient."""

    @staticmethod
    def forward(ctx, theta, fills, outs, x, x1):
        """x and x1 (or None): contiguous; outs: diff_affine_warp's new [y, y1 or None], filled and returned here."""
        ops.affine_warp(x, x1, theta, ops.WARP_CONSTANT, fills[0], fills[1], None, None, None, outs[0], outs[1])
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(theta, *((x,) if x1 is None else (x, x1)))
            ctx.fills = fills
        else:
            ctx.save_for_backward(theta)
        ctx.in_shape = tuple(x.shape)
        ctx.set_materialize_grads(False)              # an unused plane's gradient stays None: no launch for it
        return _planes_out(outs)

    @staticmethod
    def backward(ctx, *gys):
        theta, *planes = ctx.saved_tensors
        grads = [None, None]
        for k, gy in enumerate(gys):
            if gy is not None and ctx.needs_input_grad[3 + k]:
                grads[k] = ops.affine_warp_backward(gy.contiguous(), theta, ops.WARP_CONSTANT,
                                                    torch.empty(ctx.in_shape, dtype=torch.float32, device=gy.device))
        gtheta = None
        if ctx.needs_input_grad[0]:
            # only the planes with an output gradient; plane 1 alone goes in as plane 0 with its own fill
            live = [(planes[k], gy.contiguous(), ctx.fills[k]) for k, gy in enumerate(gys) if gy is not None]
            if live:
                (p0, g0, f0), (p1, g1, f1) = live[0], (live[1] if len(live) > 1 else (None, None, live[0][2]))
                gtheta = ops.affine_warp_backward_theta(p0, p1, g0, g1, theta, ops.WARP_CONSTANT, f0, f1)
        return gtheta, None, None, grads[0], grads[1]


def diff_affine_warp(x: torch.Tensor, theta: torch.Tensor, x1: Optional[torch.Tensor] = None, *, out_size=None, fill=0.0,
                     mode: str = "constant"):
    """affine_warp(..., mode="constant") without noise, differentiable in x (and x1): the same one launch forward, its
    bits under no_grad, and the exact adjoint of the trilinear gather as the backward (include/mpgan_hip.h:
    mpgan_affine_warp_backward; deterministic, no atomics), one launch per plane that requires grad.  `fill` (one number,
    or one per plane) is a constant.  A theta that is singular or shrinks by more than MPGAN_WARP_REACH_MAX per axis
    gives x a NaN gradient; none that sample_affine_params draws is.  A theta (B, 12) float64 that requires grad gets its
    own gradient, (B, 12) float64 summed in fp64 (mpgan_affine_warp_backward_theta: two launches, no atomics, the
    right-hand derivative at integer coordinates); the planes are then kept for the backward.  With a theta that
    requires none nothing is kept and nothing more is launched.  `mode` exists to say why "border" is refused: a
    clamped coordinate sends gradient from arbitrarily far away to the faces, and neither that adjoint nor its gradient
    in theta is built."""
    if mode != "constant":
        raise ValueError(f"diff_affine_warp: only mode 'constant' has a backward, got {mode!r}")
    planes, fills, outs = _warp_io("diff_affine_warp", x, x1, out_size, fill, differentiable=True)
    if any(t is not None and (t.dtype != torch.float32 or t.dim() not in (4, 5) or t.shape != x.shape) for t in planes):
        raise ValueError(f"diff_affine_warp: the planes are float32 (B, 1, *S) tensors of one shape, got "
                         f"{[(tuple(p.shape), p.dtype) for p in planes if p is not None]}")
    return _AffineWarpFn.apply(theta, fills, outs, planes[0], planes[1])


# ---- elastic deformation and MRI intensity augmentation of the same pair (the same file's second kernel) ---
# A smooth non-rigid warp on both images, a smooth multiplicative bias field and a gamma change on the input alone:
#
#     q = sample_deform_params(B, S, elastic=0.3, bias_field=0.3, gamma=0.3, device=x.device)
#     t1, t2 = deform_warp(t1w, p.theta, t2w, ctrl=q.ctrl, gain=q.gain, gamma=q.gamma)
#     batch = PairAugment(rotate=0.3, elastic=0.3, bias_field=0.3, gamma=0.3)(batch)
ELASTIC_MAX = 0.4                                     # of the lattice spacing: below it p + u(p) cannot fold
LATTICE_MIN, LATTICE_MAX = 4, 64


class DeformParams(NamedTuple):
    """One draw, each table None when its option is off: ctrl (B, ndim, *grid) float64, the control displacements of the
    (d, h, w) coordinate in voxels; gain (B, *grid) float64, the control values of the log-gain; gamma (B, 2) float64,
    the exponent of plane 0 and plane 1."""
    ctrl: Optional[torch.Tensor]
    gain: Optional[torch.Tensor]
    gamma: Optional[torch.Tensor]


def _lattice(grid, spatial, what: str):
    """One int (every axis of extent > 1; an axis of extent 1 gets 1) or one per axis -> the lattice extents."""
    if isinstance(grid, int):
        if not LATTICE_MIN <= grid <= LATTICE_MAX:
            raise ValueError(f"{what}: a lattice extent is in [{LATTICE_MIN}, {LATTICE_MAX}], got {grid!r}")
        return (grid,) if spatial is None else tuple(grid if s > 1 else 1 for s in spatial)
    grid = tuple(int(g) for g in grid)
    if len(grid) not in ((2, 3) if spatial is None else (len(spatial),)):
        raise ValueError(f"{what}: one int or one per axis, got {grid!r}")
    for k, g in enumerate(grid):                      # (spatial None: the extents are not known yet, 1 may be right)
        if g != 1 if spatial is not None and spatial[k] == 1 else not (LATTICE_MIN <= g <= LATTICE_MAX
                                                                       or (spatial is None and g == 1)):
            raise ValueError(f"{what}: a lattice extent is in [{LATTICE_MIN}, {LATTICE_MAX}] (1 on an axis of extent 1), got {grid!r}")
    return grid


def _check_deform_options(elastic, elastic_grid, bias_field, bias_grid, gamma, intensity_prob, intensity_planes,
                          spatial=None):
    if not 0.0 <= float(elastic) <= ELASTIC_MAX:
        raise ValueError(f"elastic must be in [0, {ELASTIC_MAX}] (a fraction of the lattice spacing; beyond it the map can "
                         f"fold), got {elastic!r}")
    for name, v in (("bias_field", bias_field), ("gamma", gamma)):
        if not float(v) >= 0:
            raise ValueError(f"{name} must be >= 0, got {v!r}")
    if not 0.0 <= float(intensity_prob) <= 1.0:
        raise ValueError(f"intensity_prob must be in [0, 1], got {intensity_prob!r}")
    planes = sorted({int(k) for k in intensity_planes})
    if any(k not in (0, 1) for k in planes):
        raise ValueError(f"intensity_planes: a subset of (0, 1), got {tuple(intensity_planes)!r}")
    return _lattice(elastic_grid, spatial, "elastic_grid"), _lattice(bias_grid, spatial, "bias_grid"), planes


def sample_deform_params(n: int, spatial: Sequence[int], *, elastic: float = 0.0, elastic_grid=6, bias_field: float = 0.0,
                         bias_grid=4, gamma: float = 0.0, intensity_prob: float = 1.0,
                         intensity_planes: Sequence[int] = (0,), spatial_gate: Optional[torch.Tensor] = None,
                         generator: Optional[torch.Generator] = None, device="cpu") -> DeformParams:
    """Draw the lattices of `n` samples of extent `spatial` ((H, W) or (D, H, W)), in pure torch ops on `device`, float64
    (no host sync).  A lattice of extent g_k over S_k voxels has the spacing delta_k = (S_k - 1) / (g_k - 3)
    (include/mpgan_hip.h: mpgan_deform_warp).
    elastic:      in [0, 0.4]: ctrl[:, k] = elastic * delta_k * U[-1, 1].  A B-spline deformation whose control
                  displacements stay below about 0.4 of the spacing cannot fold, hence the cap.
    elastic_grid, bias_grid: one int in [4, 64] or one per axis (an axis of extent 1 has the lattice extent 1).
    bias_field:   >= 0: the control values of the log-gain are bias_field * U[-1, 1] (the gain stays within e^+-bias_field).
    gamma:        >= 0: gamma[s][k] = exp(gamma * U[-1, 1]) for the planes of intensity_planes, exactly 1.0 for the others.
    intensity_prob: one gate per sample for gain and gamma together; a gated-off sample gets an all-zero gain lattice and
                  gamma 1.0, which deform_warp turns into a bit copy of the ungained value.
    spatial_gate: a boolean (n,) tensor (PairAugment passes on the gate of its `prob` draw): a gated-off sample gets a
                  zero ctrl.  It draws nothing.
    Draw order, one torch.rand each: ctrl (n, ndim, *elastic_grid), gain (n, *bias_grid), gamma (n, number of planes),
    then the intensity gate (n,) when 0 < intensity_prob < 1 and gain or gamma is on.  A disabled option (elastic 0;
    bias_field 0, gamma 0, no plane or intensity_prob 0) draws nothing and returns None for its table."""
    spatial = _spatial("sample_deform_params", spatial)
    eg, bg, planes = _check_deform_options(elastic, elastic_grid, bias_field, bias_grid, gamma, intensity_prob,
                                           intensity_planes, spatial)
    device = torch.device(device)
    kw = dict(generator=generator, device=device, dtype=torch.float64)
    ctrl = gain = gam = None
    if elastic > 0:
        delta = torch.tensor([(s - 1) / (g - 3) if g > 1 else 0.0 for s, g in zip(spatial, eg)], dtype=torch.float64)
        delta = (float(elastic) * delta).to(device).view(1, len(spatial), *[1] * len(spatial))
        ctrl = (2.0 * torch.rand((n, len(spatial), *eg), **kw) - 1.0) * delta
        if spatial_gate is not None:
            ctrl = torch.where(spatial_gate.view(n, *[1] * (ctrl.dim() - 1)), ctrl, torch.zeros_like(ctrl))
        ctrl = ctrl.contiguous()
    live = intensity_prob > 0.0 and bool(planes)
    if live and bias_field > 0:
        gain = float(bias_field) * (2.0 * torch.rand((n, *bg), **kw) - 1.0)
    if live and gamma > 0:
        gam = torch.ones((n, 2), dtype=torch.float64, device=device)
        draw = torch.exp(float(gamma) * (2.0 * torch.rand((n, len(planes)), **kw) - 1.0))
        for j, k in enumerate(planes):
            gam[:, k] = draw[:, j]
    if intensity_prob < 1.0 and (gain is not None or gam is not None):
        on = torch.rand((n,), **kw) < intensity_prob
        if gain is not None:
            gain = torch.where(on.view(n, *[1] * len(bg)), gain, torch.zeros_like(gain))
        if gam is not None:
            gam = torch.where(on[:, None], gam, torch.ones_like(gam))
    return DeformParams(ctrl, None if gain is None else gain.contiguous(), gam)


def deform_warp(x: torch.Tensor, theta: torch.Tensor, x1: Optional[torch.Tensor] = None, *, ctrl=None, gain=None,
                gain_planes: Sequence[int] = (0,), gamma=None, value_range=(-1.0, 1.0), out_size=None,
                mode: str = "border", fill=-1.0, noise=None, sigma: Optional[torch.Tensor] = None):
    """affine_warp with an elastic deformation of the map and an intensity change of the values, in the same one launch
    (include/mpgan_hip.h: mpgan_deform_warp):  c = (A p + t) + u(p) with u the cubic B-spline of the control
    displacements ctrl (B, ndim, *grid) float64, in voxels, over the OUTPUT extent; on the planes listed in `gain_planes`
    v += (v - lo) * expm1(b(p)) with b the B-spline of the log-gain lattice gain (B, *grid) float64; then
    v = lo + (hi - lo) * ((v - lo) / (hi - lo)) ** gamma[:, k] with gamma (B, 2) float64 and (lo, hi) = value_range; then
    the noise term.  ctrl, gain and gamma may each be None (that term is absent); zero lattices and gamma 1 give
    affine_warp's bits, and a value of exactly lo stays lo.  The other arguments are affine_warp's.  Not differentiable."""
    planes, fills, noises, outs = _warp_arguments("deform_warp", x, x1, out_size, mode, fill, noise)
    ndim = x.dim() - 2
    for t, lead, name in ((ctrl, 2, "ctrl"), (gain, 1, "gain")):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != lead + ndim or t.dtype != torch.float64
                              or (name == "ctrl" and t.shape[1] != ndim)):
            raise ValueError(f"deform_warp: {name} must be a float64 (B, {'ndim, ' if lead == 2 else ''}*grid) tensor for a "
                             f"{ndim}-D image, got {tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")
    if ndim == 2:                                     # the d channel and the d extent of a 2-D lattice
        if ctrl is not None:
            ctrl = torch.cat([torch.zeros_like(ctrl[:, :1]), ctrl], 1).unsqueeze(2)
        if gain is not None:
            gain = gain.unsqueeze(1)
    mask = 0
    if gain is not None:
        if any(int(k) not in (0, 1) for k in gain_planes):
            raise ValueError(f"deform_warp: gain_planes is a subset of (0, 1), got {tuple(gain_planes)!r}")
        mask = sum(1 << k for k in {int(k) for k in gain_planes})
    lo, hi = (float(v) for v in value_range)
    ops.deform_warp(planes[0], planes[1], theta, None if ctrl is None else ctrl.contiguous(),
                    None if gain is None else gain.contiguous(), mask, gamma, lo, hi, WARP_MODES[mode], fills[0], fills[1],
                    noises[0], noises[1], sigma, outs[0], outs[1])
    return _planes_out(outs)


class PairAugment(nn.Module):
    """Random geometric augmentation of a training pair with noise on the input (the reference imports MONAI's
    RandRotated and RandGaussianNoised, GAN_final.py:35-36, and never wires them in): forward(batch) draws once
    (sample_affine_params; `generator`: a torch.Generator on the batch's device, or None for torch's global one), warps
    batch["t1w"] and batch["t2w"] under the same draw in one launch, adds sigma * N(0, 1) to `noise_keys` (the field: one
    torch.randn of shape (number of noise keys, *t1w.shape) from the same generator, after the parameters; none is
    drawn when noise_std is 0) and returns a new dict; the other entries pass through.  `.last_params` is the last
    draw, `.last_noise` its field (or None).  No parameters, no buffers, no gradient.

    elastic, elastic_grid, bias_field, bias_grid, gamma, intensity_prob (sample_deform_params; kept in
    `.deform_options`), intensity_keys and value_range add an elastic deformation of both images under the same lattice
    and a bias field and gamma change on `intensity_keys`: with any of elastic, bias_field, gamma above 0 the one launch
    is deform_warp's, the lattices are drawn after the affine parameters and before the noise field, a sample that the
    `prob` gate turned off gets no deformation either (with prob 0 none is drawn), and `.last_deform` holds the
    DeformParams.  With all three 0 nothing changes: affine_warp, the same draws, `.last_deform` None."""

    def __init__(self, rotate=0.0, scale: float = 0.0, shift=0.0, flip: Sequence[int] = (), prob: float = 1.0,
                 noise_std: float = 0.0, noise_prob: float = 1.0, noise_keys: Sequence[str] = ("t1w",),
                 mode: str = "border", fill: float = -1.0, generator: Optional[torch.Generator] = None,
                 elastic: float = 0.0, elastic_grid=6, bias_field: float = 0.0, bias_grid=4, gamma: float = 0.0,
                 intensity_prob: float = 1.0, intensity_keys: Sequence[str] = ("t1w",), value_range=(-1.0, 1.0)):
        super().__init__()
        intensity_keys = (intensity_keys,) if isinstance(intensity_keys, str) else tuple(intensity_keys)
        if any(k not in PAIR_KEYS for k in intensity_keys):
            raise ValueError(f"PairAugment: intensity_keys must be a subset of {PAIR_KEYS}, got {intensity_keys!r}")
        self.intensity_planes = sorted({PAIR_KEYS.index(k) for k in intensity_keys})
        _check_deform_options(elastic, elastic_grid, bias_field, bias_grid, gamma, intensity_prob, self.intensity_planes)
        value_range = tuple(float(v) for v in value_range)
        if len(value_range) != 2 or not value_range[1] > value_range[0]:
            raise ValueError(f"PairAugment: value_range is (lo, hi) with hi > lo, got {value_range!r}")
        self.deform_options = dict(elastic=float(elastic), elastic_grid=elastic_grid, bias_field=float(bias_field),
                                   bias_grid=bias_grid, gamma=float(gamma), intensity_prob=float(intensity_prob))
        self.value_range = value_range
        self.last_deform: Optional[DeformParams] = None
        noise_keys = (noise_keys,) if isinstance(noise_keys, str) else tuple(noise_keys)
        if any(k not in PAIR_KEYS for k in noise_keys):
            raise ValueError(f"PairAugment: noise_keys must be a subset of {PAIR_KEYS}, got {noise_keys!r}")
        if mode not in WARP_MODES:
            raise ValueError(f"PairAugment: mode must be one of {sorted(WARP_MODES)}, got {mode!r}")
        self.noise_planes = sorted({PAIR_KEYS.index(k) for k in noise_keys})
        _check_some_image(rotate, scale, shift, flip, prob, noise_std, noise_prob, self.noise_planes)
        self.options = dict(rotate=rotate, scale=float(scale), shift=shift, flip=tuple(flip), prob=float(prob),
                            noise_std=float(noise_std), noise_prob=float(noise_prob))
        self.mode, self.fill = mode, float(fill)
        self.generator = generator
        self.last_params: Optional[AffineParams] = None
        self.last_noise: Optional[torch.Tensor] = None

    def extra_repr(self):
        text = ", ".join(f"{k}={v!r}" for k, v in self.options.items()) + f", mode={self.mode!r}, fill={self.fill}"
        if self.deforms:
            text += ", " + ", ".join(f"{k}={v!r}" for k, v in self.deform_options.items())
        return text

    @property
    def deforms(self) -> bool:
        """Whether forward launches deform_warp (any of elastic, bias_field, gamma is on) or affine_warp."""
        return any(self.deform_options[k] > 0 for k in ("elastic", "bias_field", "gamma"))

    def forward(self, batch):
        t1w, t2w = batch["t1w"], batch["t2w"]
        with torch.no_grad():
            n, spatial = t1w.shape[0], tuple(t1w.shape[2:])
            p, gate = _sample_affine(n, spatial, noise_planes=self.noise_planes, generator=self.generator,
                                     device=t1w.device, **self.options)
            q = None
            if self.deforms:
                q = dict(self.deform_options)
                if self.options["prob"] == 0.0:       # no spatial op draws at all
                    q["elastic"] = 0.0
                q = sample_deform_params(n, spatial, intensity_planes=self.intensity_planes, spatial_gate=gate,
                                         generator=self.generator, device=t1w.device, **q)
            noise = [None, None]
            field = None
            if self.options["noise_std"] > 0 and self.noise_planes:
                field = torch.randn((len(self.noise_planes), *t1w.shape), generator=self.generator, device=t1w.device,
                                    dtype=torch.float32)
                for j, k in enumerate(self.noise_planes):
                    noise[k] = field[j]
            self.last_params, self.last_noise, self.last_deform = p, field, q
            sigma = p.sigma if field is not None else None
            if q is None:
                y1, y2 = affine_warp(t1w, p.theta, t2w, mode=self.mode, fill=self.fill, noise=noise, sigma=sigma)
            else:
                y1, y2 = deform_warp(t1w, p.theta, t2w, ctrl=q.ctrl, gain=q.gain, gain_planes=self.intensity_planes,
                                     gamma=q.gamma, value_range=self.value_range, mode=self.mode, fill=self.fill,
                                     noise=noise, sigma=sigma)
        out = dict(batch)
        out["t1w"], out["t2w"] = y1, y2
        return out
