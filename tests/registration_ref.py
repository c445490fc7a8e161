"""The registration phantom and a float64 torch restatement of mpgan_amd.registration.register_affine on
the CPU: grid_sample for the warp, mi_loss_ref.loss for -MI, torch.optim.Adam for the step.  Nothing here touches the
package.

Phantom, from a seed alone, at S = (32, 40, 48), normalised coordinates z_k = (i_k - (S_k - 1) / 2) / (S_k / 2):
    tissue = 1 / (1 + exp(12 (r - 1))), r the radius in an ellipsoid of semi-axes (0.8, 0.7, 0.75)
    f      = clip(sum of 10 Gaussian blobs, -1, 1): centres U[-0.5, 0.5]^3, sigma U[0.12, 0.3], amplitude U[-1, 1]
    t2     = -1 + tissue (1 + 0.6 f),   t1 = -1 + tissue (1 - 0.5 f + 0.3 f^2)      (one anatomy, a non-monotone contrast)
    moving = t1 warped by the inverse of a known rigid theta_true, rounded to fp32;  fixed = t2
"""
import functools

import numpy as np
import torch

import affine_ref as R
import mi_loss_ref as M

S = (32, 40, 48)
FILL = -1.0
CASES = {1: ((-0.15, 0.05, 0.1), (-2.5, 1.0, 2.0)), 2: ((0.2, 0.15, -0.2), (3.0, -3.0, 2.0))}     # seed -> angles, shift
CASE_2D = ((0.15, 0.0, 0.0), (0.0, 2.0, -1.5))                                                      # on the slice d = 16 of seed 1
DEFAULTS = dict(levels=(2, 1), iters=(80, 40), lr=(0.02, 0.01))


def phantom(seed, size=S):
    """(t1, t2) float64 (D, H, W)."""
    rng = np.random.default_rng(seed)
    blobs = [(rng.uniform(-0.5, 0.5, 3), rng.uniform(0.12, 0.3), rng.uniform(-1.0, 1.0)) for _ in range(10)]   # drawn blob by blob
    centres, sigma, amp = (np.array(v) for v in zip(*blobs))
    z =np.stack(np.meshgrid(*[(np.arange(s) - (s - 1) / 2.0) / (s / 2.0) for s in size], indexing="ij"))
    r = np.sqrt(sum((z[k] / a) ** 2 for k, a in enumerate((0.8, 0.7, 0.75))))
    tissue = 1.0 / (1.0 + np.exp(12.0 * (r - 1.0)))
    f = sum(amp[i] * np.exp(-sum((z[k] - centres[i, k]) ** 2 for k in range(3)) / (2.0 * sigma[i] ** 2)) for i in range(10))
    f = np.clip(f, -1.0, 1.0)
    return -1.0 + tissue * (1.0 - 0.5 * f + 0.3 * f * f), -1.0 + tissue * (1.0 + 0.6 * f)


def invert(theta):
    m = np.asarray(theta, dtype=np.float64).reshape(3, 4)
    Ai = np.linalg.inv(m[:, :3])
    return np.concatenate([Ai, -(Ai @ m[:, 3:])], axis=1).reshape(12)


def compose(a, b):
    """c = a(b(p))."""
    a, b = np.asarray(a, dtype=np.float64).reshape(3, 4), np.asarray(b, dtype=np.float64).reshape(3, 4)
    return np.concatenate([a[:, :3] @ b[:, :3], a[:, :3] @ b[:, 3:] + a[:, 3:]], axis=1).reshape(12)


def corner_error(theta_a, theta_b, size):
    """The largest distance in voxels between theta_a p and theta_b p over the corners of the box of extent `size`."""
    a, b = np.asarray(theta_a, dtype=np.float64).reshape(3, 4), np.asarray(theta_b, dtype=np.float64).reshape(3, 4)
    size = R._dhw(size)
    worst = 0.0
    for corner in np.ndindex(*[2 if s > 1 else 1 for s in size]):
        p = np.array([c * (s - 1) for c, s in zip(corner, size)] + [1.0])
        worst = max(worst, float(np.linalg.norm(a @ p - b @ p)))
    return worst


@functools.lru_cache(maxsize=None)
def case(seed):
    """(moving fp32 (D, H, W), fixed fp32, theta_true (12,)): warping moving by theta_true gives t1 on fixed's grid."""
    angles, shift = CASES[seed]
    t1, t2 = phantom(seed)
    theta_true = R.theta_from_params(angles, 1.0, shift, in_size=S)
    moving = R.affine_warp_ref(t1[None], invert(theta_true)[None], S, mode=R.CONSTANT, fill=FILL)[0]
    return moving.astype(np.float32), t2.astype(np.float32), theta_true


@functools.lru_cache(maxsize=None)
def case_2d():
    """The same for the slice d = 16 of seed 1's phantom: arrays (1, H, W)."""
    t1, t2 = phantom(1)
    size = (1,) + S[1:]
    theta_true = R.theta_from_params(CASE_2D[0], 1.0, CASE_2D[1], in_size=size)
    moving = R.affine_warp_ref(t1[None, 16:17], invert(theta_true)[None], size, mode=R.CONSTANT, fill=FILL)[0]
    return moving.astype(np.float32), t2[16:17].astype(np.float32), theta_true


# ---- the restatement ----------------------------------------------------------------------------------------------------
def warp(x, theta, fill=FILL):
    """x (B, 1, D, H, W) float64, theta (B, 12): the CONSTANT trilinear warp by grid_sample, differentiable in theta."""
    B, size = x.shape[0], x.shape[2:]
    th = theta.reshape(B, 3, 4)
    p = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in size], indexing="ij")
                    + (torch.ones(tuple(size), dtype=torch.float64),), dim=-1)
    c = torch.einsum("nkj,dhwj->ndhwk", th, p)
    if size[0] == 1:
        norm = torch.tensor([size[2] - 1, size[1] - 1], dtype=torch.float64)
        grid = 2.0 * c[:, 0, :, :, [2, 1]] / norm - 1.0
        y = torch.nn.functional.grid_sample(x[:, :, 0] - fill, grid, mode="bilinear", padding_mode="zeros",
                                            align_corners=True)[:, :, None]
    else:
        norm = torch.tensor([size[2] - 1, size[1] - 1, size[0] - 1], dtype=torch.float64)
        grid = 2.0 * c[..., [2, 1, 0]] / norm - 1.0
        y = torch.nn.functional.grid_sample(x - fill, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return y + fill


def mi_loss(y, target):
    return M.loss(y, target, num_bins=23, reduction="none", value_range=(-1.0, 1.0))


def rigid_theta(q, size, transform="rigid"):
    """q (B, P) -> theta (B, 12): A = R_d R_h R_w (2-D: the in-plane rotation), t = c - A c + shift, the shifts of q in
    units of half the extent.  "translation": shifts alone."""
    B = q.shape[0]
    three_d = size[0] > 1
    axes = [0, 1, 2] if three_d else [1, 2]
    n_ang = 0 if transform == "translation" else (3 if three_d else 1)
    ang = [q[:, k] if k < n_ang else torch.zeros(B, dtype=torch.float64) for k in range(3)]
    planes = [(1, 2), (2, 0), (0, 1)]                                  # R_d turns (h, w), R_h (w, d), R_w (d, h)
    A = torch.eye(3, dtype=torch.float64).expand(B, 3, 3)
    for a, (i, j) in zip(ang, planes):
        G = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
        G[:, i, i], G[:, j, j], G[:, i, j], G[:, j, i] = torch.cos(a), torch.cos(a), -torch.sin(a), torch.sin(a)
        A = A @ G
    shift = torch.zeros(B, 3, dtype=torch.float64)
    shift = torch.stack([q[:, n_ang + axes.index(k)] * (size[k] / 2.0) if k in axes else shift[:, k] for k in range(3)], dim=1)
    c = torch.tensor([(s - 1) / 2.0 for s in size], dtype=torch.float64)
    t = c - A @ c + shift
    return torch.cat([A, t[:, :, None]], dim=2).reshape(B, 12)


def to_level(theta, L, size):
    """(A | t) -> (A | (A o + t - o) / L), o = (L - 1) / 2, on the pooled axes (A couples no pooled axis with an unpooled one)."""
    B = theta.shape[0]
    th = theta.reshape(B, 3, 4)
    Lv = torch.tensor([float(L) if s > 1 else 1.0 for s in size], dtype=torch.float64)
    o = (Lv - 1.0) / 2.0
    t = (th[:, :, :3] @ o + th[:, :, 3] - o) / Lv
    return torch.cat([th[:, :, :3], t[:, :, None]], dim=2).reshape(B, 12)


def pooled(x, L):
    if L == 1:
        return x
    return torch.nn.functional.avg_pool3d(x, tuple(L if s > 1 else 1 for s in x.shape[2:]))


def register_ref(moving, fixed, transform="rigid", levels=DEFAULTS["levels"], iters=DEFAULTS["iters"], lr=DEFAULTS["lr"],
                 loss=mi_loss, fill=FILL):
    """moving, fixed: (B, D, H, W) arrays -> (theta (B, 12) numpy, final loss (B,), history (sum(iters), B))."""
    m = torch.from_numpy(np.asarray(moving, dtype=np.float64))[:, None]
    f = torch.from_numpy(np.asarray(fixed, dtype=np.float64))[:, None]
    size = tuple(m.shape[2:])
    n_par = (0 if transform == "translation" else (3 if size[0] > 1 else 1)) + (3 if size[0] > 1 else 2)
    q = torch.zeros(m.shape[0], n_par, dtype=torch.float64, requires_grad=True)
    history = []
    for L, steps, rate in zip(levels, iters, lr):
        ml, fl = pooled(m, L), pooled(f, L)
        opt = torch.optim.Adam([q], lr=rate)
        for _ in range(steps):
            opt.zero_grad()
            item = loss(warp(ml, to_level(rigid_theta(q, size, transform), L, size), fill), fl)
            item.sum().backward()
            history.append(item.detach().clone())
            opt.step()
    with torch.no_grad():
        theta = rigid_theta(q, size, transform)
        L = levels[-1]
        final = loss(warp(pooled(m, L), to_level(theta, L, size), fill), pooled(f, L))
    return theta.numpy(), final.numpy(), torch.stack(history).numpy()


def loss_at(moving, fixed, theta, loss=mi_loss, fill=FILL):
    m = torch.from_numpy(np.asarray(moving, dtype=np.float64))[:, None]
    f = torch.from_numpy(np.asarray(fixed, dtype=np.float64))[:, None]
    with torch.no_grad():
        return loss(warp(m, torch.from_numpy(np.asarray(theta, dtype=np.float64)).reshape(-1, 12), fill), f).numpy()
