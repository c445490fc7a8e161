"""float64 numpy restatement of the affine warp's gradient in theta (include/mpgan_hip.h:
mpgan_affine_warp_backward_theta) and the cases of its host and GPU tests.

Per sample and output voxel p = (d, h, w), with P = (d, h, w, 1):

    c      = A p + t by the forward's own expression (warp_backward_ref.coords)
    dead   any c_k NaN or outside [-1, S_k]: all three derivatives are 0
    b, f   = floor(c), c - floor(c)
    v_ijl  = x[b + (i, j, l)] inside the input, else fill: ALL eight corners, also those of forward weight 0
    dy/dc_w = lerp_d(lerp_h(v001 - v000, v011 - v010; f_h), lerp_h(v101 - v100, v111 - v110; f_h); f_d), d and h alike
    g_theta[k][j] = sum_p (sum_planes gy[p] dy/dc_k(p)) P_j(p)

dense: the input is padded by 2 with `fill` and the eight corners are indexed in it; nothing of the kernel's tiles,
partials or orders.
"""
import numpy as np

import affine_ref as R
import warp_backward_ref as B


def _lerp(a, b, f):
    return a + f * (b - a)


def derivatives(x, theta, out_size, fill):
    """dy/dc of one sample: x (D, H, W), theta (12,) -> (3, oD, oH, oW) float64, 0 at dead voxels."""
    x = np.asarray(x, dtype=np.float64)
    S = x.shape
    c = B.coords(theta, out_size)
    with np.errstate(invalid="ignore"):
        dead = np.zeros(c.shape[1:], dtype=bool)
        for k in range(3):
            dead |= ~((c[k] >= -1.0) & (c[k] <= float(S[k])))      # NaN is dead
    c = np.where(dead[None], 0.0, c)
    b = np.floor(c)
    f = c - b
    b = b.astype(np.int64) + 2                                     # index in the padded input
    xp = np.pad(x, 2, mode="constant", constant_values=float(fill))
    v = [[[xp[b[0] + i, b[1] + j, b[2] + l] for l in range(2)] for j in range(2)] for i in range(2)]
    fd, fh, fw = f
    dd = _lerp(_lerp(v[1][0][0] - v[0][0][0], v[1][0][1] - v[0][0][1], fw),
               _lerp(v[1][1][0] - v[0][1][0], v[1][1][1] - v[0][1][1], fw), fh)
    dh = _lerp(_lerp(v[0][1][0] - v[0][0][0], v[0][1][1] - v[0][0][1], fw),
               _lerp(v[1][1][0] - v[1][0][0], v[1][1][1] - v[1][0][1], fw), fd)
    dw = _lerp(_lerp(v[0][0][1] - v[0][0][0], v[0][1][1] - v[0][1][0], fh),
               _lerp(v[1][0][1] - v[1][0][0], v[1][1][1] - v[1][1][0], fh), fd)
    return np.where(dead[None], 0.0, np.stack([dd, dh, dw]))


def affine_warp_theta_grad_ref(x, gy, theta, fill=0.0, x1=None, gy1=None, fill1=0.0):
    """x: (n, D, H, W), gy: (n, oD, oH, oW), theta: (n, 12) -> (g_theta (n, 12), scale (n, 12)) float64, scale the sum of
    the absolute terms |gy dy/dc_k P_j| (per plane) that the GPU test's bound is relative to."""
    planes = [(np.asarray(x), np.asarray(gy, dtype=np.float64), fill)]
    if x1 is not None:
        planes.append((np.asarray(x1), np.asarray(gy1, dtype=np.float64), fill1))
    n, out_size = planes[0][1].shape[0], planes[0][1].shape[1:]
    theta = np.asarray(theta, dtype=np.float64).reshape(n, 12)
    P = np.concatenate([np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in out_size], indexing="ij")),
                        np.ones((1,) + tuple(out_size))]).reshape(4, -1)
    g, scale = np.zeros((n, 3, 4)), np.zeros((n, 3, 4))
    for s in range(n):
        for xs, gs, fl in planes:
            G = (gs[s][None] * derivatives(xs[s], theta[s], out_size, fl)).reshape(3, -1)
            g[s] += np.einsum("kp,jp->kj", G, P)
            scale[s] += np.einsum("kp,jp->kj", np.abs(G), P)
    return g.reshape(n, 12), scale.reshape(n, 12)


FILLS = (0.0, -1.0)
S567 = (5, 6, 7)
_EYE = np.eye(3, 4).reshape(12)
_ROT567 = R.theta_from_params((0.3, -0.2, 0.4), 1.1, (0.1, 0.2, -0.3), in_size=S567)
_NAN = _ROT567.copy()
_NAN[6] = np.nan                                                   # A[1][2]: c_h is NaN at every voxel

# name -> (n, in size (D, H, W), out size, theta (n, 12)): every case of the x backward and four of this file's own
CASES = dict(B.CASES)
CASES.update({
    "tiles3d": R._case(1, (9, 17, 33), (9, 17, 33), [(0.2, -0.15, 0.25)], [1.05], [(0.4, -0.7, 1.3)]),   # 3 x 3 x 2 tiles
    # 33 x 8 = 264 tiles of 1 x 8 x 32 per sample: the per-sample pass wraps past its 256 threads
    "many": R._case(2, (1, 264, 250), (1, 264, 250), [(0.3, 0, 0), (-0.2, 0, 0)], [1.1, 0.95],
                    [(0.0, 2.5, -1.25), (0.0, -3.0, 4.5)]),
    # every f == 0: only the zero-weight corners carry the derivative
    "integer": (3, S567, S567, np.stack([_EYE, np.array([-1, 0, 0, 4, 0, 1, 0, 0, 0, 0, -1, 6], dtype=np.float64),
                                         np.array([1, 0, 0, 1, 0, 1, 0, -2, 0, 0, 1, 3], dtype=np.float64)])),
    "nan": (2, S567, S567, np.stack([_NAN, _ROT567])),
})


def make_case(name, seed=0):
    """(x0, x1, gy0, gy1) fp32 numpy of a case, from the seed alone."""
    n, in_size, out_size, _ = CASES[name]
    return (R.make_input(n, in_size, seed=seed), R.make_input(n, in_size, seed=seed + 1),
            B.make_grad(n, out_size, seed=seed + 2), B.make_grad(n, out_size, seed=seed + 3))
