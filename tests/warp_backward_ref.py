"""float64 numpy restatement of the affine warp's backward (include/mpgan_hip.h: mpgan_affine_warp_backward)
and the cases of its host and GPU tests.

    c(p)    = A p + t, by the forward's own expression: A[k][0]*d + (A[k][1]*h + A[k][2]*w + A[k][3])
    tent(u) = 1 - |u| if |u| < 1, else 0 (also 0 for NaN)
    g_x[q]  = sum over output voxels p of g_y[p] * tent(c_d(p) - q_d) * tent(c_h(p) - q_h) * tent(c_w(p) - q_w)

with dense per-axis tent weights (an (N_out, S_k) table per axis: no candidate search, nothing of the kernel's
mechanism).  A sample is supported when det A is finite and non-zero and every r_k = sum_j |A^-1[k][j]| <= REACH_MAX; an
unsupported sample is NaN everywhere.
"""
import numpy as np

import affine_ref as R

REACH_MAX = 4.0                                       # MPGAN_WARP_REACH_MAX


def coords(theta, out_size):
    """c = A p + t for every output voxel in the forward kernel's order of operations: (3, oD, oH, oW) float64."""
    A = np.asarray(theta, dtype=np.float64).reshape(3, 4)
    d, h, w = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in R._dhw(out_size)], indexing="ij")
    return np.stack([A[k, 0] * d + (A[k, 1] * h + A[k, 2] * w + A[k, 3]) for k in range(3)])


def tent(u):
    a = np.abs(u)
    with np.errstate(invalid="ignore"):
        return np.where(a < 1.0, 1.0 - a, 0.0)


def reach(theta):
    """(det A, (r_d, r_h, r_w)) of one theta; r is NaN where A has no inverse."""
    A = np.asarray(theta, dtype=np.float64).reshape(3, 4)[:, :3]
    with np.errstate(all="ignore"):
        det = float(np.linalg.det(A)) if np.isfinite(A).all() else float("nan")
        if not np.isfinite(det) or det == 0.0:
            return det, (float("nan"),) * 3
        return det, tuple(float(v) for v in np.abs(np.linalg.inv(A)).sum(axis=1))


def supported(theta):
    det, r = reach(theta)
    return bool(np.isfinite(det) and det != 0.0 and all(v <= REACH_MAX for v in r))


def affine_warp_backward_ref(gy, theta, in_size):
    """gy: (n, oD, oH, oW) (or (n, oH, oW)); theta: (n, 12); returns g_x (n, D, H, W) float64."""
    gy = np.asarray(gy, dtype=np.float64)
    if gy.ndim == 3:
        gy = gy[:, None]
    n, out_size = gy.shape[0], gy.shape[1:]
    S = R._dhw(in_size)
    theta = np.asarray(theta, dtype=np.float64).reshape(n, 12)
    gx = np.empty((n,) + S, dtype=np.float64)
    for s in range(n):
        if not supported(theta[s]):
            gx[s] = np.nan
            continue
        c = coords(theta[s], out_size).reshape(3, -1)
        wd, wh, ww = (tent(c[k][:, None] - np.arange(S[k], dtype=np.float64)[None, :]) for k in range(3))
        gx[s] = np.einsum("p,pa,pb,pc->abc", gy[s].reshape(-1), wd, wh, ww, optimize=True)
    return gx


def make_grad(n, size, seed=1):
    """The output gradient of the tests: uniform in [-1, 1), fp32 values, (n, oD, oH, oW)."""
    return R.make_input(n, size, seed=seed)


# name -> (n, in size (D, H, W), out size, theta (n, 12)): affine_ref's rotated cases and three of this file's own
_ANGLES, _SHIFT = (0.3, -0.5, 0.7), (0.2, -0.1, 0.3)
_wide0 = R.theta_from_params((0.2, 0.1, -0.3), 1.1, (0.3, 0.2, -1.7), in_size=(5, 9, 35))
CASES = dict(R.CASES)
CASES.update({
    "zoom2": R._case(1, (5, 6, 7), (9, 11, 13), [_ANGLES], [2.0], [_SHIFT]),        # the largest supported reach: 3.44
    "mini": R._case(1, (9, 11, 13), (5, 6, 7), [_ANGLES], [0.5], [_SHIFT]),          # many q without any contributor
    "wide": (2, (5, 9, 35), (5, 9, 35), np.stack([_wide0, np.eye(3, 4).reshape(12)])),    # W % 4 != 0, two tiles along w
})
