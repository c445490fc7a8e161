"""Rigid / affine co-registration of a pair on the device by mutual information.

    res = register_affine(moving, fixed)                       # rigid, levels (2, 1), Parzen-window -MI
    aligned = augment.affine_warp(moving, res.theta, mode="constant", fill=-1.0)

The hot path is three fused pieces: the trilinear warp (mpgan_affine_warp), its gradient in theta
(mpgan_affine_warp_backward_theta) and the Parzen-window MI loss with its backward.  Everything else is a few float64
torch ops on (B, P) parameter tensors: the map from parameters to theta, with autograd, and a per-element Adam step.
Iteration counts are fixed and nothing is read back in the loop: no host sync.

theta is (B, 12) float64 = (A | t) in (d, h, w) voxel-index order, as everywhere in augment.py: output voxel p reads
the input at A p + t, so warping `moving` by res.theta lays it on `fixed`'s grid.

Not built: a gradient for the border mode, a gradient of deform_warp (non-rigid registration), any wiring into
GAN.fit_batch or data.py, normalised cross-correlation (pass a callable as `loss` for another metric).
"""
from typing import Callable, NamedTuple, Optional, Sequence

import torch
import torch.nn.functional as F

from . import augment, losses

TRANSFORMS = ("translation", "rigid", "similarity", "affine")
MIN_LEVEL_EXTENT = 8
ADAM_EPS = 1e-8


class RegistrationResult(NamedTuple):
    """theta (B, 12) float64; loss (B,), the loss at theta on the last level; history (sum(iters), B), the loss of every
    iteration before its step.  All on the device."""
    theta: torch.Tensor
    loss: torch.Tensor
    history: torch.Tensor


# ---- theta algebra (float64, on theta's device, no host sync) ---------------------------------------------------------
def _split(theta):
    if theta.dim() != 2 or theta.shape[1] != 12 or theta.dtype != torch.float64:
        raise ValueError(f"theta must be a float64 (B, 12) tensor, got {tuple(theta.shape)} {theta.dtype}")
    m = theta.reshape(-1, 3, 4)
    return m[:, :, :3], m[:, :, 3:]


def _join(A, t):
    return torch.cat([A, t], dim=2).reshape(-1, 12).contiguous()


def compose_theta(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The theta of c = a(b(p)): warping by it equals sampling at b's coordinate first and carrying that through a."""
    Aa, ta = _split(a)
    Ab, tb = _split(b)
    return _join(Aa @ Ab, Aa @ tb + ta)


def invert_theta(theta: torch.Tensor) -> torch.Tensor:
    """The theta of p = A^-1 (c - t), by the adjugate (no pivoting, no error flag to read back: no host sync).  A
    singular A gives inf / NaN."""
    A, t = _split(theta)
    a = [[A[:, i, j] for j in range(3)] for i in range(3)]
    adj = [[a[1][1] * a[2][2] - a[1][2] * a[2][1], a[0][2] * a[2][1] - a[0][1] * a[2][2], a[0][1] * a[1][2] - a[0][2] * a[1][1]],
           [a[1][2] * a[2][0] - a[1][0] * a[2][2], a[0][0] * a[2][2] - a[0][2] * a[2][0], a[0][2] * a[1][0] - a[0][0] * a[1][2]],
           [a[1][0] * a[2][1] - a[1][1] * a[2][0], a[0][1] * a[2][0] - a[0][0] * a[2][1], a[0][0] * a[1][1] - a[0][1] * a[1][0]]]
    det = a[0][0] * adj[0][0] + a[0][1] * adj[1][0] + a[0][2] * adj[2][0]
    Ai = torch.stack([torch.stack(row, dim=1) for row in adj], dim=1) / det[:, None, None]
    return _join(Ai, -(Ai @ t))


def registration_error(theta_a: torch.Tensor, theta_b: torch.Tensor, spatial: Sequence[int]) -> torch.Tensor:
    """Per sample, the largest distance in voxels between theta_a p and theta_b p over the 8 (2-D: 4) corners p of the
    output box of extent `spatial`: (B,) float64."""
    S = (1,) * (3 - len(spatial)) + tuple(int(s) for s in spatial)
    Aa, ta = _split(theta_a)
    Ab, tb = _split(theta_b)
    ends = [torch.arange(2 if s > 1 else 1, dtype=torch.float64, device=theta_a.device) * float(s - 1) for s in S]
    corners = torch.cartesian_prod(*ends).reshape(-1, 3).t()                                # (3, corners)
    gap = (Aa - Ab) @ corners + (ta - tb)                                                   # (B, 3, corners)
    return gap.norm(dim=1).amax(dim=1)


def level_theta(theta: torch.Tensor, level: int, spatial: Sequence[int]) -> torch.Tensor:
    """The full-resolution theta on the grid of the average-pooled images: level voxel q sits at p = L q + o of the full
    grid, o = (L - 1) / 2, so (A | t) becomes (L^-1 A L | (A o + t - o) / L); an axis of extent 1 is not pooled (L = 1,
    o = 0 there)."""
    S = (1,) * (3 - len(spatial)) + tuple(int(s) for s in spatial)
    A, t = _split(theta)
    Ls = [float(level) if s > 1 else 1.0 for s in S]
    one = torch.ones(3, dtype=torch.float64, device=theta.device)
    Lv = torch.stack([one[k] * Ls[k] for k in range(3)])                                    # (no host-to-device copy)
    o = ((Lv - 1.0) / 2.0).reshape(1, 3, 1)
    return _join(A * Lv.reshape(1, 1, 3) / Lv.reshape(1, 3, 1), (A @ o + t - o) / Lv.reshape(1, 3, 1))


# ---- parameters -> theta ----------------------------------------------------------------------------------------------
def num_params(transform: str, ndim: int) -> int:
    if transform not in TRANSFORMS:
        raise ValueError(f"transform must be one of {TRANSFORMS}, got {transform!r}")
    angles = 3 if ndim == 3 else 1
    return {"translation": ndim, "rigid": angles + ndim, "similarity": angles + ndim + 1, "affine": 12}[transform]


def _matmul3(a, b):
    return [[a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def params_to_theta(q: torch.Tensor, transform: str, spatial: Sequence[int]) -> torch.Tensor:
    """q (B, P) float64, zero at the identity -> theta (B, 12), differentiable.  About the image centre c = (S - 1) / 2
    in theta_from_params' convention: A = R / s, R = R_d R_h R_w, t = c - A c + shift.  Columns of q: the angles (3; 2-D:
    the one in-plane angle), then one shift per axis in units of half that axis's extent, then log s.  "affine": q is
    (dA (9, row-major) | dt (3)), A = I + dA about the centre and the shift dt in the same half-extent units; a 2-D
    image keeps its d row and column at (1, 0, 0)."""
    ndim = len(spatial)
    S = (1,) * (3 - ndim) + tuple(int(s) for s in spatial)
    first = 3 - ndim
    if q.dim() != 2 or q.shape[1] != num_params(transform, ndim) or q.dtype != torch.float64:
        raise ValueError(f"params_to_theta: {transform!r} on a {ndim}-D image takes float64 (B, {num_params(transform, ndim)}) "
                         f"parameters, got {tuple(q.shape)} {q.dtype}")
    zero = q[:, 0] * 0.0
    one = zero + 1.0
    c = [(s - 1) / 2.0 for s in S]
    half = [s / 2.0 for s in S]
    if transform == "affine":
        A = [[(one if i == j else zero) + (q[:, 3 * i + j] if i >= first and j >= first else zero) for j in range(3)]
             for i in range(3)]
        shift = [q[:, 9 + k] * half[k] if k >= first else zero for k in range(3)]
    else:
        col = 0
        ang = [zero, zero, zero]
        if transform != "translation":
            for k in range(3 if ndim == 3 else 1):
                ang[k] = q[:, col]
                col += 1
        shift = [zero, zero, zero]
        for k in range(first, 3):
            shift[k] = q[:, col] * half[k]
            col += 1
        inv_s = torch.exp(-q[:, col]) if transform == "similarity" else one
        cd, sd, ch, sh, cw, sw = (f(a) for a in ang for f in (torch.cos, torch.sin))
        Rd = [[one, zero, zero], [zero, cd, -sd], [zero, sd, cd]]
        Rh = [[ch, zero, sh], [zero, one, zero], [-sh, zero, ch]]
        Rw = [[cw, -sw, zero], [sw, cw, zero], [zero, zero, one]]
        R = _matmul3(_matmul3(Rd, Rh), Rw)
        A = [[R[i][j] * inv_s if i >= first and j >= first else R[i][j] for j in range(3)] for i in range(3)]
    t = [c[k] - (A[k][0] * c[0] + A[k][1] * c[1] + A[k][2] * c[2]) + shift[k] for k in range(3)]
    return torch.stack([e for k in range(3) for e in (A[k][0], A[k][1], A[k][2], t[k])], dim=1).contiguous()


# ---- the registration -------------------------------------------------------------------------------------------------
def _pooled(x, level):
    if level == 1:
        return x.contiguous()
    kernel = tuple(level if s > 1 else 1 for s in x.shape[2:])
    return (F.avg_pool3d if x.dim() == 5 else F.avg_pool2d)(x, kernel).contiguous()         # a remainder is dropped


def register_affine(moving: torch.Tensor, fixed: torch.Tensor, *, transform: str = "rigid", levels: Sequence[int] = (2, 1),
                    iters: Sequence[int] = (80, 40), lr: Sequence[float] = (0.02, 0.01), num_bins: int = 23,
                    value_range=(-1.0, 1.0), fill: float = -1.0, init: Optional[torch.Tensor] = None,
                    loss: Optional[Callable] = None, betas=(0.9, 0.999)) -> RegistrationResult:
    """Register `moving` to `fixed`, two (B, 1, *S) fp32 device tensors of one shape (2-D or 3-D), each sample with its own
    transform: at every level of the pyramid a fixed number of Adam steps on the parameters of `transform` (see
    params_to_theta) down the per-sample loss of (diff_affine_warp(moving_level, theta_level, fill=fill), fixed_level).
    loss: None for losses.global_mutual_information_loss(..., num_bins, value_range, reduction="none"), else a callable
          (y, fixed_level) -> (B,) that autograd can differentiate in y.
    levels, iters, lr: one entry per level, coarse to fine; level L average-pools both images by L (level_theta gives
          the conversion).  A level that would leave an axis of extent > 1 under 8 voxels is refused.  Adam's moments
          start from zero at every level.
    init: a (B, 12) float64 start.  "affine": the base that the parameters' (dA | dt) is added to.  The others: composed
          in front, theta = compose_theta(init, theta(params)): the parameters move the output grid about its centre
          and init carries the result into `moving`.
    Fixed iteration counts, no convergence test and no value read back on the host: the call never syncs."""
    if not (isinstance(moving, torch.Tensor) and isinstance(fixed, torch.Tensor) and moving.is_cuda and fixed.is_cuda):
        raise ValueError("register_affine: moving and fixed must be device tensors (there is no CPU path)")
    if moving.shape != fixed.shape or moving.dim() not in (4, 5) or moving.shape[1] != 1:
        raise ValueError(f"register_affine: moving and fixed are (B, 1, *S) tensors of one shape, got {tuple(moving.shape)} "
                         f"and {tuple(fixed.shape)}")
    if moving.dtype != torch.float32 or fixed.dtype != torch.float32:
        raise ValueError("register_affine: moving and fixed must be float32")
    levels, iters, lr = tuple(int(v) for v in levels), tuple(int(v) for v in iters), tuple(float(v) for v in lr)
    if not levels or len(iters) != len(levels) or len(lr) != len(levels) or min(levels) < 1 or min(iters) < 1:
        raise ValueError(f"register_affine: levels, iters and lr have one entry per level (levels >= 1, iters >= 1), got "
                         f"{levels}, {iters}, {lr}")
    spatial = tuple(int(s) for s in moving.shape[2:])
    for L in levels:
        if any(s > 1 and s // L < MIN_LEVEL_EXTENT for s in spatial):
            raise ValueError(f"register_affine: level {L} leaves extent {tuple(s // L if s > 1 else 1 for s in spatial)} of "
                             f"{spatial}: under {MIN_LEVEL_EXTENT} voxels on an axis")
    B, dev = moving.shape[0], moving.device
    P = num_params(transform, len(spatial))
    if init is not None:
        if tuple(init.shape) != (B, 12) or init.dtype != torch.float64 or init.device != dev:
            raise ValueError(f"register_affine: init must be a float64 ({B}, 12) tensor on {dev}, got {tuple(init.shape)} "
                             f"{init.dtype} on {init.device}")
        init = init.detach()
    if loss is None:
        def loss(y, target):
            return losses.global_mutual_information_loss(y, target, num_bins=num_bins, reduction="none",
                                                         value_range=value_range)
    b1, b2 = (float(b) for b in betas)
    moving, fixed = moving.detach(), fixed.detach()
    identity = params_to_theta(torch.zeros((B, P), dtype=torch.float64, device=dev), transform, spatial)

    def theta_of(q):
        th = params_to_theta(q, transform, spatial)
        if init is None:
            return th
        return init + (th - identity) if transform == "affine" else compose_theta(init, th)

    q = torch.zeros((B, P), dtype=torch.float64, device=dev)
    history = []
    for L, steps, rate in zip(levels, iters, lr):
        m_lv, f_lv = _pooled(moving, L), _pooled(fixed, L)
        m, v = torch.zeros_like(q), torch.zeros_like(q)
        for step in range(1, steps + 1):
            q = q.detach().requires_grad_(True)
            th = level_theta(theta_of(q), L, spatial)
            item = loss(augment.diff_affine_warp(m_lv, th, fill=fill), f_lv)
            (g,) = torch.autograd.grad(item.sum(), q)
            history.append(item.detach())
            m = b1 * m + (1.0 - b1) * g
            v = b2 * v + (1.0 - b2) * g * g
            q = q.detach() - (rate / (1.0 - b1 ** step)) * m / ((v / (1.0 - b2 ** step)).sqrt() + ADAM_EPS)
    with torch.no_grad():
        theta = theta_of(q.detach()).contiguous()
        L = levels[-1]
        final = loss(augment.diff_affine_warp(_pooled(moving, L), level_theta(theta, L, spatial), fill=fill),
                     _pooled(fixed, L)).detach()
    return RegistrationResult(theta, final, torch.stack(history))
