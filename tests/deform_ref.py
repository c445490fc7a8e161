"""float64 numpy restatement of the elastic deformation and intensity augmentation (include/mpgan_hip.h:
mpgan_deform_warp), for the host and GPU tests.  The sums are the literal 64-term ones.

    lattice rule   xi = 1 + p (g - 3) / (S - 1), i = min(floor(xi), g - 3), f = xi - i; weights B_0..3(f) on the entries
                   i - 1 .. i + 2; an axis of extent 1 has the lattice extent 1 and the weight 1
    c      = (A p + t) + u(p)
    v      = trilinear(x, c)                                 constant / border as affine_ref
    v     += (v - lo) * expm1(b(p))                          on a plane with gain
    v      = lo + R * (max(v - lo, 0) / R) ** gamma          R = hi - lo; skipped when gamma == 1
"""
import numpy as np

import affine_ref as R

CONSTANT, BORDER = R.CONSTANT, R.BORDER


def axis_weights(S, g):
    """The four lattice entries (S, 4) int and their weights (S, 4) of every index 0..S-1 of one axis."""
    if S == 1:
        assert g == 1, (S, g)
        return np.zeros((1, 4), dtype=np.int64), np.array([[1.0, 0.0, 0.0, 0.0]])
    assert g >= 4, (S, g)
    p = np.arange(S, dtype=np.float64)
    xi = 1.0 + p * (g - 3) / (S - 1)
    i = np.minimum(np.floor(xi), g - 3)
    f = xi - i
    B = np.stack([(1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6, f ** 3 / 6], 1)
    return i.astype(np.int64)[:, None] + np.arange(4) - 1, B


def field(lattice, out_size):
    """The B-spline of one scalar lattice (g_d, g_h, g_w) at every voxel of out_size: (oD, oH, oW) float64."""
    lattice = np.asarray(lattice, dtype=np.float64)
    out_size = R._dhw(out_size)
    (id_, Bd), (ih, Bh), (iw, Bw) = (axis_weights(out_size[k], lattice.shape[k]) for k in range(3))
    acc = np.zeros(out_size, dtype=np.float64)
    for a in range(4):
        for b in range(4):
            for c in range(4):
                w = Bd[:, a, None, None] * Bh[None, :, b, None] * Bw[None, None, :, c]
                acc += w * lattice[id_[:, a, None, None], ih[None, :, b, None], iw[None, None, :, c]]
    return acc


def displacement(ctrl, out_size):
    """u (3, oD, oH, oW) of one sample's control lattice (3, g_d, g_h, g_w); u_k = 0 on an axis of extent 1."""
    out_size = R._dhw(out_size)
    u = np.stack([field(ctrl[k], out_size) for k in range(3)])
    for k in range(3):
        if out_size[k] == 1:
            u[k] = 0.0
    return u


def sample_at(x, c, mode, fill):
    """trilinear(x, c) for one sample x (D, H, W) at the coordinates c (3, *out): affine_ref's corner logic."""
    S, out_size = x.shape, c.shape[1:]
    c = c.copy()
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
        v = x[tuple(np.clip(idx[k], 0, S[k] - 1) for k in range(3))]
        acc += w * np.where(inside, v, float(fill))
    return acc


def intensity(v, log_gain=None, gamma=None, lo=-1.0, hi=1.0):
    """Gain, then gamma, of one sample's values; log_gain: the field b(p) or None; gamma: a number or None."""
    if log_gain is not None:
        v = v + (v - lo) * np.expm1(log_gain)
    if gamma is not None and gamma != 1.0:
        v = lo + (hi - lo) * (np.maximum(v - lo, 0.0) / (hi - lo)) ** gamma
    return v


def deform_warp_ref(x, theta, out_size=None, mode=BORDER, fill=0.0, ctrl=None, gain=None, gamma=None, lo=-1.0, hi=1.0):
    """One plane.  x: (n, D, H, W); theta: (n, 12); ctrl: (n, 3, g_d, g_h, g_w) or None; gain: (n, b_d, b_h, b_w) or None
    (None too for a plane outside gain_planes); gamma: (n,) for this plane or None.  Returns (n, oD, oH, oW) float64."""
    x = np.asarray(x, dtype=np.float64)
    n, S = x.shape[0], x.shape[1:]
    out_size = R._dhw(S if out_size is None else out_size)
    theta = np.asarray(theta, dtype=np.float64).reshape(n, 12)
    out = np.empty((n,) + out_size, dtype=np.float64)
    for s in range(n):
        c = R.coords(theta[s], out_size)
        if ctrl is not None:
            c = c + displacement(ctrl[s], out_size)
        v = sample_at(x[s], c, mode, fill)
        out[s] = intensity(v, None if gain is None else field(gain[s], out_size), None if gamma is None else float(gamma[s]),
                           lo, hi)
    return out


def jacobian_determinant(ctrl, out_size):
    """det of d(p + u(p)) / dp by central differences (one-sided at the faces) over the voxel grid; an axis of extent 1
    contributes the factor 1."""
    out_size = R._dhw(out_size)
    u = displacement(ctrl, out_size)
    J = np.zeros((3, 3) + out_size)
    for k in range(3):
        for j in range(3):
            g = np.gradient(u[k], axis=j) if out_size[j] > 1 else np.zeros(out_size)
            J[k, j] = g + (1.0 if k == j else 0.0)
    return np.linalg.det(np.moveaxis(J, (0, 1), (-2, -1)))


def spacing(out_size, grid):
    return [(s - 1) / (g - 3) if g > 1 else 0.0 for s, g in zip(R._dhw(out_size), grid)]


def make_input(n, size, seed=0, low=-1.0):
    """affine_ref.make_input mapped from [-1, 1) to [low, 1): fp32 values."""
    x = R.make_input(n, size, seed).astype(np.float64)
    return (low + (x + 1.0) * (1.0 - low) / 2.0).astype(np.float32)


# The GPU tests' cases: name -> (n, in size, out size, theta (n, 12), ctrl (n, 3, *grid), gain (n, *grid), gamma (n, 2)).
# Control displacements up to 1.5 voxels, log-gains up to 0.3, gamma in [0.5, 2]; theta: the rotated cases of affine_ref,
# whose samples leave the input in part.
def _case(name, ctrl_grid, gain_grid, seed):
    n, in_size, out_size, theta = R.CASES[name]
    rng = np.random.default_rng(seed)
    ctrl = (rng.random((n, 3) + ctrl_grid) * 2.0 - 1.0) * 1.5
    gain = (rng.random((n,) + gain_grid) * 2.0 - 1.0) * 0.3
    gamma = np.exp((rng.random((n, 2)) * 2.0 - 1.0) * np.log(2.0))
    gamma[0] = (0.5, 2.0)                                   # both ends of the range
    return n, in_size, out_size, theta, ctrl, gain, gamma


CASES = {
    "ffd3d": _case("rot3d", (4, 5, 6), (4, 4, 5), 11),
    "ffd2d": _case("rot2d", (1, 4, 5), (1, 4, 5), 12),
    "ffdcrop": _case("crop", (4, 4, 4), (4, 5, 4), 13),
}
