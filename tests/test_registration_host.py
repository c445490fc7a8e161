"""The registration phantom and its float64 restatement (tests/registration_ref.py) hold the tight conditions that the
GPU test's looser ones stand on, and the host plumbing of mpgan_amd.registration (parameters -> theta, the pyramid's
conversion, the theta algebra: pure torch, so it runs here) agrees with numpy.  No GPU.

Measured on the CPU with the defaults levels (2, 1), iters (80, 40), lr (0.02, 0.01):

    case      corner error before -> after (voxels)   share    final -MI    -MI at theta_true
    seed 1    7.27 -> 1.28                              0.176    -0.9557      -0.9424
    seed 2    14.75 -> 1.39                             0.094    -0.9574      -0.9536
    2-D       7.08 -> 1.19   (levels (1,), iters (80,), lr (0.02,))   0.169    -1.1987      -1.1627

The optimum of MI sits a little beside the truth (interpolation smooths the warped image, which MI rewards), so the
condition is a share of the initial error, not a sub-voxel one."""
import functools

import numpy as np
import pytest
import torch

import affine_ref as R
import registration_ref as G

EYE = np.eye(3, 4).reshape(12)


@functools.lru_cache(maxsize=None)
def _registered(seed):
    moving, fixed, theta_true = G.case(seed)
    return G.register_ref(moving[None], fixed[None])


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_registers_the_phantom(seed):
    moving, fixed, theta_true = G.case(seed)
    theta, final, history = _registered(seed)
    before, after = G.corner_error(EYE, theta_true, G.S), G.corner_error(theta[0], theta_true, G.S)
    at_true = float(G.loss_at(moving[None], fixed[None], theta_true[None])[0])
    print(f"seed {seed}: corner error {before:.2f} -> {after:.2f} ({after / before:.3f}), final -MI {final[0]:.4f}, "
          f"at theta_true {at_true:.4f}")
    assert abs(before - {1: 7.27, 2: 14.75}[seed]) < 0.005
    assert after <= 0.25 * before                              # measured 0.176 and 0.094
    assert final[0] <= at_true - 2e-3                          # measured 1.3e-2 and 3.7e-3 below
    assert history.shape == (120, 1) and history[-1, 0] < history[0, 0]


def test_restatement_registers_the_slice():
    moving, fixed, theta_true = G.case_2d()
    size = (1,) + G.S[1:]
    theta, final, history = G.register_ref(moving[None], fixed[None], levels=(1,), iters=(80,), lr=(0.02,))
    before, after = G.corner_error(EYE, theta_true, size), G.corner_error(theta[0], theta_true, size)
    print(f"2-D: corner error {before:.2f} -> {after:.2f} ({after / before:.3f}), final -MI {final[0]:.4f}")
    assert after <= 0.25 * before                              # measured 0.169
    assert np.array_equal(theta[0].reshape(3, 4)[0], [1, 0, 0, 0]) and np.array_equal(theta[0].reshape(3, 4)[:, 0], [1, 0, 0])


def test_phantom_is_one_anatomy_under_two_contrasts():
    t1, t2 = G.phantom(1)
    assert t1.shape == G.S and t1.min() >= -1.0 and t2.max() <= 1.0 and t1.max() <= 1.0
    assert abs(t1[0, 0, 0] + 1.0) < 1e-3 and abs(t2[0, 0, 0] + 1.0) < 1e-3           # background at the fill value
    moving, fixed, theta_true = G.case(1)
    back = R.affine_warp_ref(moving[None], theta_true[None], G.S, mode=R.CONSTANT, fill=G.FILL)[0]
    inner = (slice(8, -8),) * 3
    # theta_true undoes the misalignment but for two trilinear interpolations (measured: 0.052)
    assert np.abs(back - t1)[inner].max() < 0.25 * np.abs(moving - t1)[inner].max()


# ---- the host plumbing of mpgan_amd.registration -------------------------------------------------------------------------
def _thetas(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([R.theta_from_params(rng.uniform(-0.5, 0.5, 3), rng.uniform(0.8, 1.2), rng.uniform(-3, 3, 3),
                                         in_size=(9, 11, 13)) for _ in range(n)])


def test_theta_algebra_against_numpy():
    from mpgan_amd import registration as reg
    a, b = _thetas(3, 0), _thetas(3, 1)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    got = reg.compose_theta(ta, tb).numpy()
    inv = reg.invert_theta(ta).numpy()
    err = reg.registration_error(ta, tb, (9, 11, 13)).numpy()
    err2 = reg.registration_error(ta, tb, (11, 13)).numpy()
    for s in range(3):
        assert np.abs(got[s] - G.compose(a[s], b[s])).max() <= 1e-13
        assert np.abs(inv[s] - G.invert(a[s])).max() <= 1e-13
        assert abs(err[s] - G.corner_error(a[s], b[s], (9, 11, 13))) <= 1e-12
        assert abs(err2[s] - G.corner_error(a[s], b[s], (1, 11, 13))) <= 1e-12
    p = np.array([2.0, -1.0, 3.5, 1.0])                       # c = a(b(p))
    for s in range(3):
        bp = np.append(b[s].reshape(3, 4) @ p, 1.0)
        assert np.abs(got[s].reshape(3, 4) @ p - a[s].reshape(3, 4) @ bp).max() <= 1e-12
    eye = reg.compose_theta(ta, reg.invert_theta(ta)).numpy()
    assert np.abs(eye - EYE).max() <= 1e-12
    assert float(reg.registration_error(ta, ta, (9, 11, 13)).max()) == 0.0


@pytest.mark.parametrize("size", [(9, 11, 13), (11, 13)], ids=str)
def test_parameters_to_theta(size):
    from mpgan_amd import registration as reg
    ndim, S3 = len(size), R._dhw(size)
    n_ang = 3 if ndim == 3 else 1
    assert [reg.num_params(t, ndim) for t in reg.TRANSFORMS] == ([3, 6, 7, 12] if ndim == 3 else [2, 3, 4, 12])
    rng = np.random.default_rng(3)
    for transform in reg.TRANSFORMS:
        P = reg.num_params(transform, ndim)
        zero = reg.params_to_theta(torch.zeros(2, P, dtype=torch.float64), transform, size).numpy()
        assert np.array_equal(zero, np.stack([EYE, EYE]))                          # zero at the identity, exactly
        q = rng.uniform(-0.3, 0.3, (2, P))
        got = reg.params_to_theta(torch.from_numpy(q), transform, size).numpy()
        for s in range(2):
            if transform == "affine":
                dA = np.zeros((3, 3))
                dA[3 - ndim:, 3 - ndim:] = q[s, :9].reshape(3, 3)[3 - ndim:, 3 - ndim:]
                A = np.eye(3) + dA
                c = (np.asarray(S3) - 1.0) / 2.0
                shift = np.array([q[s, 9 + k] * S3[k] / 2.0 if k >= 3 - ndim else 0.0 for k in range(3)])
                want = np.concatenate([A, (c - A @ c + shift)[:, None]], axis=1).reshape(12)
            else:
                ang = np.zeros(3)
                col = 0
                if transform != "translation":
                    ang[:n_ang] = q[s, :n_ang]
                    col = n_ang
                shift = np.zeros(3)
                shift[3 - ndim:] = q[s, col:col + ndim] * np.asarray(S3[3 - ndim:]) / 2.0
                scale = float(np.exp(q[s, col + ndim])) if transform == "similarity" else 1.0
                want = R.theta_from_params(ang, scale, shift, in_size=S3)           # A = R / s, t = c - A c + shift
            assert np.abs(got[s] - want).max() <= 1e-12, (transform, s)
    # autograd reaches the parameters
    q = torch.zeros(1, reg.num_params("rigid", ndim), dtype=torch.float64, requires_grad=True)
    reg.params_to_theta(q, "rigid", size)[0, 11].backward()
    assert q.grad[0, -1] == size[-1] / 2.0                                          # t_w moves by half the extent per unit
    with pytest.raises(ValueError):
        reg.params_to_theta(torch.zeros(1, 5, dtype=torch.float64), "rigid", size)
    with pytest.raises(ValueError):
        reg.num_params("elastic", 3)


@pytest.mark.parametrize("size,level", [((32, 40, 48), 2), ((32, 40, 48), 4), ((40, 48), 2)], ids=str)
def test_level_theta_is_the_map_between_pooled_grids(size, level):
    """A level voxel q sits at p = L q + o of the full grid: the level theta must send q to (theta p - o) / L."""
    from mpgan_amd import registration as reg
    S3 = R._dhw(size)
    theta = R.theta_from_params((0.2, -0.1, 0.15) if len(size) == 3 else (0.2, 0, 0), 1.1, (0.0 if len(size) == 2 else 1.5, -2.0, 0.5),
                                in_size=S3)
    got = reg.level_theta(torch.from_numpy(theta[None]), level, size).numpy()[0].reshape(3, 4)
    want = G.to_level(torch.from_numpy(theta[None]), level, S3).numpy()[0].reshape(3, 4)
    assert np.abs(got - want).max() <= 1e-13
    Lv = np.array([level if s > 1 else 1 for s in S3], dtype=np.float64)
    o = (Lv - 1.0) / 2.0
    for q in ([0, 0, 0], [0 if S3[0] == 1 else 3, 5, 7]):
        q = np.asarray(q, dtype=np.float64)
        full = theta.reshape(3, 4) @ np.append(Lv * q + o, 1.0)
        assert np.abs(got @ np.append(q, 1.0) - (full - o) / Lv).max() <= 1e-12
    assert np.array_equal(reg.level_theta(torch.from_numpy(theta[None]), 1, size).numpy()[0], theta)


def test_register_affine_refuses_before_any_launch():
    from mpgan_amd import registration as reg
    x = torch.zeros(1, 1, 16, 20, 24)
    with pytest.raises(ValueError, match="device"):
        reg.register_affine(x, x)
