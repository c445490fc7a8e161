"""float64 numpy restatement of the paired affine warp (include/mpgan_hip.h: mpgan_affine_warp) and of the
sampler's convention, for the host and GPU tests.

    y[s][p] = sum over the 8 corners k of floor(c) + {0,1}^3 of weight_k * value_k,  c = A p + t,  (A | t) = theta[s]
    "constant": value_k = fill where the corner lies outside the input;  "border": c clamped to [0, S - 1] first
    theta_from_params: A = F R / s, R = R_d R_h R_w, t = c_in - A c_out + shift  (all in (d, h, w) index order)
"""
import numpy as np

CONSTANT, BORDER = "constant", "border"


def _dhw(size):
    size = tuple(int(s) for s in size)
    return (1,) * (3 - len(size)) + size


def coords(theta, out_size):
    """c = A p + t for every output voxel: (3, oD, oH, oW) float64."""
    th = np.asarray(theta, dtype=np.float64).reshape(3, 4)
    p = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in _dhw(out_size)], indexing="ij"))
    return np.einsum("ij,j...->i...", th[:, :3], p) + th[:, 3].reshape(3, 1, 1, 1)


def affine_warp_ref(x, theta, out_size=None, mode=BORDER, fill=0.0):
    """x: (n, D, H, W) (or (n, H, W)) array; theta: (n, 12); returns (n, oD, oH, oW) float64."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 3:
        x = x[:, None]
    n, S = x.shape[0], x.shape[1:]
    out_size = _dhw(S if out_size is None else out_size)
    theta = np.asarray(theta, dtype=np.float64).reshape(n, 12)
    out = np.empty((n,) + out_size, dtype=np.float64)
    for s in range(n):
        c = coords(theta[s], out_size)
        if mode == BORDER:
            for k in range(3):
                c[k] = np.clip(c[k], 0.0, S[k] - 1.0)
        else:
            assert mode == CONSTANT, mode
        base = np.floor(c)
        f = c - base
        base = base.astype(np.int64)
        acc = np.zeros(out_size, dtype=np.float64)
        for corner in range(8):
            bits = [(corner >> 2) & 1, (corner >> 1) & 1, corner & 1]
            idx = [base[k] + bits[k] for k in range(3)]
            w = np.ones(out_size, dtype=np.float64)
            inside = np.ones(out_size, dtype=bool)
            for k in range(3):
                w = w * (f[k] if bits[k] else 1.0 - f[k])
                inside &= (idx[k] >= 0) & (idx[k] < S[k])
            v = x[s][tuple(np.clip(idx[k], 0, S[k] - 1) for k in range(3))]
            acc += w * np.where(inside, v, float(fill))       # (border: an outside corner has weight 0)
        out[s] = acc
    return out


def rotation(angles):
    """R = R_d R_h R_w for angles (about d, about h, about w), in (d, h, w) index order."""
    ad, ah, aw = (float(a) for a in angles)
    c, s = np.cos, np.sin
    Rd = np.array([[1, 0, 0], [0, c(ad), -s(ad)], [0, s(ad), c(ad)]], dtype=np.float64)
    Rh = np.array([[c(ah), 0, s(ah)], [0, 1, 0], [-s(ah), 0, c(ah)]], dtype=np.float64)
    Rw = np.array([[c(aw), -s(aw), 0], [s(aw), c(aw), 0], [0, 0, 1]], dtype=np.float64)
    return Rd @ Rh @ Rw


def theta_from_params(angles=(0.0, 0.0, 0.0), scale=1.0, shift=(0.0, 0.0, 0.0), flips=(1, 1, 1), in_size=None,
                      out_size=None):
    """The 12 entries of (A | t): A = F R / s, t = c_in - A c_out + shift, c = (S - 1) / 2.  2-D (D = 1 on both sides):
    the angles are (in-plane, 0, 0)."""
    in_size = _dhw(in_size)
    out_size = in_size if out_size is None else _dhw(out_size)
    A = np.diag(np.asarray(flips, dtype=np.float64)) @ rotation(angles) / float(scale)
    c_in = (np.asarray(in_size, dtype=np.float64) - 1.0) / 2.0
    c_out = (np.asarray(out_size, dtype=np.float64) - 1.0) / 2.0
    t = c_in - A @ c_out + np.asarray(shift, dtype=np.float64)
    if in_size[0] == 1 and out_size[0] == 1:          # a 2-D image: the d row and column stay (1, 0, 0), t_d = 0
        A[0], A[:, 0], t[0] = (1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.0
    return np.concatenate([A, t[:, None]], axis=1).reshape(12)


def corner_shares(theta, in_size, out_size=None):
    """The shares of the output voxels (pooled over the samples of theta (n, 12)) whose corners floor(c) + {0,1}^3 lie
    all inside the input, some inside, none inside.  A corner of weight exactly 0 is no corner (it is never read): on
    an axis where c is an integer only the base corner counts, so a 2-D image (c_d = 0) has four corners per voxel."""
    in_size = _dhw(in_size)
    out_size = in_size if out_size is None else _dhw(out_size)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, 12)
    counts = np.zeros(3)
    for th in theta:
        c = coords(th, out_size)
        base = np.floor(c).astype(np.int64)
        frac = c - np.floor(c)
        n_in, n_all = np.zeros(out_size, dtype=np.int64), np.zeros(out_size, dtype=np.int64)
        for corner in range(8):
            inside, counted = np.ones(out_size, dtype=bool), np.ones(out_size, dtype=bool)
            for k, bit in enumerate(((corner >> 2) & 1, (corner >> 1) & 1, corner & 1)):
                inside &= (base[k] + bit >= 0) & (base[k] + bit < in_size[k])
                if bit:
                    counted &= frac[k] > 0
            n_in += inside & counted
            n_all += counted
        counts += [(n_in == n_all).sum(), ((n_in > 0) & (n_in < n_all)).sum(), (n_in == 0).sum()]
    return tuple(counts / counts.sum())


def make_input(n, size, seed=0):
    """Uniform in [-1, 1), fp32 values, (n, D, H, W): computed from the seed alone."""
    rng = np.random.default_rng(seed)
    return (rng.random((n,) + _dhw(size)) * 2.0 - 1.0).astype(np.float32)


# The rotated cases of the GPU tests: name -> (n, in size (D, H, W), out size, theta (n, 12)).
def _case(n, in_size, out_size, angles, scales, shifts):
    th = np.stack([theta_from_params(angles[s], scales[s], shifts[s], in_size=in_size, out_size=out_size) for s in range(n)])
    return n, _dhw(in_size), _dhw(out_size), th


CASES = {
    "rot3d": _case(2, (7, 9, 11), (7, 9, 11), [(0.4, -0.3, 0.5), (-0.7, 0.2, 0.1)], [1.1, 0.9],
                   [(0.3, -0.2, 0.1), (-1.4, 0.6, 2.2)]),
    "rot2d": _case(3, (1, 13, 10), (1, 13, 10), [(0.5, 0, 0), (-1.2, 0, 0), (2.8, 0, 0)], [0.8, 1.0, 1.25],
                   [(0.0, 0.4, -0.3)] * 3),
    "crop": _case(1, (12, 10, 14), (6, 7, 5), [(0.3, 0.6, -0.4)], [1.0], [(0.0, 0.0, 0.0)]),
}
ROTATED_CONSTANT = ("rot3d", "rot2d")       # the cases whose corner shares the host test pins
