"""Elastic deformation and intensity augmentation, everything that needs no GPU: the float64 restatement
(tests/deform_ref.py), the sampler on the CPU, the no-folding condition behind the cap on `elastic`, the module's and
the trainer's options, and the library's host-side refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import deform_ref as D


# ---- the restatement's field -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size,grid", [((7, 9, 11), (4, 5, 6)), ((1, 13, 10), (1, 4, 5)), ((6, 1, 5), (7, 1, 4)),
                                           ((2, 3, 70), (64, 4, 9))], ids=str)
def test_constant_and_linear_lattices_are_reproduced(out_size, grid):
    for S, g in zip(out_size, grid):                                    # the weights: >= 0, a partition of unity
        idx, B = D.axis_weights(S, g)
        assert idx.min() >= 0 and idx.max() <= g - 1 and B.min() >= 0.0
        assert np.abs(B.sum(1) - 1.0).max() <= 5e-16
    assert np.abs(D.field(np.full(grid, 0.37), out_size) - 0.37).max() <= 1e-14
    assert not D.field(np.zeros(grid), out_size).any()                 # 0 * w sums to exactly 0
    # cubic B-splines reproduce linear functions: a lattice linear in its index gives a field linear in p, with the
    # lattice coordinate xi_k = 1 + p_k (g_k - 3) / (S_k - 1) in the place of the index
    coef = np.array([0.3, -0.2, 0.11])
    j = np.meshgrid(*[np.arange(g, dtype=np.float64) for g in grid], indexing="ij")
    lattice = 0.05 + sum(coef[k] * j[k] for k in range(3))
    p = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in out_size], indexing="ij")
    xi = [1.0 + p[k] * (grid[k] - 3) / (out_size[k] - 1) if out_size[k] > 1 else np.zeros(out_size) for k in range(3)]
    want = 0.05 + sum(coef[k] * xi[k] for k in range(3))
    assert np.abs(D.field(lattice, out_size) - want).max() <= 1e-12
    # the displacement: no component along an axis of extent 1
    u = D.displacement(np.stack([lattice] * 3), out_size)
    for k in range(3):
        assert u[k].any() == (out_size[k] > 1)


def test_restatement_without_lattices_is_the_affine_restatement():
    R = D.R
    for name in R.CASES:
        n, in_size, out_size, theta = R.CASES[name]
        x = R.make_input(n, in_size)
        for mode in (D.CONSTANT, D.BORDER):
            a = R.affine_warp_ref(x, theta, out_size, mode, fill=-1.0)
            assert np.array_equal(D.deform_warp_ref(x, theta, out_size, mode, fill=-1.0), a)
            zero = np.zeros((n, 3, 1 if out_size[0] == 1 else 4, 4, 5))
            b = D.deform_warp_ref(x, theta, out_size, mode, fill=-1.0, ctrl=zero, gain=zero[:, 0], gamma=np.ones(n))
            assert np.array_equal(b, a)
    v = np.array([-1.0, -0.5, 0.25])
    got = D.intensity(v, np.full(3, 0.2), 0.6)
    assert got[0] == -1.0 and np.all(got[1:] > v[1:] - 1.0)            # lo stays lo


# ---- the sampler -----------------------------------------------------------------------------------------------------
FULL = dict(elastic=0.4, elastic_grid=(5, 4, 7), bias_field=0.3, bias_grid=(4, 5, 4), gamma=0.5, intensity_prob=0.6,
            intensity_planes=(0, 1))


def test_sample_deform_params_ranges_and_draw_order():
    from mpgan_amd import augment as A
    n, spatial = 300, (24, 20, 28)
    p = A.sample_deform_params(n, spatial, generator=torch.Generator().manual_seed(9), **FULL)
    assert isinstance(p, A.DeformParams) and p._fields == ("ctrl", "gain", "gamma")
    assert p.ctrl.shape == (n, 3, 5, 4, 7) and p.gain.shape == (n, 4, 5, 4) and p.gamma.shape == (n, 2)
    assert all(t.dtype == torch.float64 and t.is_contiguous() for t in p)
    # replay: one torch.rand each for ctrl, gain, gamma, then the intensity gate
    g = torch.Generator().manual_seed(9)
    rand = lambda *shape: torch.rand(shape, generator=g, dtype=torch.float64)
    delta = torch.tensor(D.spacing(spatial, FULL["elastic_grid"]), dtype=torch.float64)
    assert delta.tolist() == [23 / 2, 19 / 1, 27 / 4]
    ctrl = (2 * rand(n, 3, 5, 4, 7) - 1) * (0.4 * delta).view(1, 3, 1, 1, 1)
    gain = 0.3 * (2 * rand(n, 4, 5, 4) - 1)
    gam = torch.exp(0.5 * (2 * rand(n, 2) - 1))
    on = rand(n) < 0.6
    assert torch.allclose(p.ctrl, ctrl, rtol=0, atol=1e-13)
    assert torch.allclose(p.gain, torch.where(on.view(n, 1, 1, 1), gain, torch.zeros_like(gain)), rtol=0, atol=1e-15)
    assert torch.allclose(p.gamma, torch.where(on[:, None], gam, torch.ones_like(gam)), rtol=0, atol=1e-15)
    # ranges: |ctrl_k| <= elastic * delta_k, and most of the range is used
    for k in range(3):
        top = float(p.ctrl[:, k].abs().max())
        assert 0.95 * 0.4 * float(delta[k]) < top <= 0.4 * float(delta[k])
    assert 0.28 < float(p.gain.abs().max()) <= 0.3
    assert np.exp(-0.5) <= float(p.gamma.min()) and float(p.gamma.max()) <= np.exp(0.5)
    # gated-off samples are exactly zero / 1.0; the others are not
    off = ~on
    assert 0.5 < float(on.double().mean()) < 0.7
    assert not bool(p.gain[off].any()) and bool((p.gamma[off] == 1.0).all())
    assert bool(p.gain[on].flatten(1).any(1).all()) and bool((p.gamma[on] != 1.0).all())
    # the spatial gate zeroes ctrl and draws nothing
    gate = torch.arange(n) % 3 != 0
    q = A.sample_deform_params(n, spatial, spatial_gate=gate, generator=torch.Generator().manual_seed(9), **FULL)
    assert not bool(q.ctrl[~gate].any()) and torch.equal(q.ctrl[gate], p.ctrl[gate])
    assert torch.equal(q.gain, p.gain) and torch.equal(q.gamma, p.gamma)
    # one plane: the other's gamma is exactly 1
    one = A.sample_deform_params(8, spatial, gamma=0.5, generator=torch.Generator().manual_seed(1))
    assert one.ctrl is None and one.gain is None
    assert bool((one.gamma[:, 1] == 1.0).all()) and bool((one.gamma[:, 0] != 1.0).all())


def test_sample_deform_params_2d_and_extent_one_axes():
    from mpgan_amd import augment as A
    p = A.sample_deform_params(5, (13, 10), elastic=0.3, elastic_grid=(4, 5), bias_field=0.2, generator=torch.Generator().manual_seed(2))
    assert p.ctrl.shape == (5, 2, 4, 5) and p.gain.shape == (5, 4, 4) and p.gamma is None
    assert float(p.ctrl[:, 0].abs().max()) <= 0.3 * 12 / 1 and float(p.ctrl[:, 1].abs().max()) <= 0.3 * 9 / 2
    q = A.sample_deform_params(2, (1, 13, 10), elastic=0.3)             # one int: 1 on the axis of extent 1
    assert q.ctrl.shape == (2, 3, 1, 6, 6) and not bool(q.ctrl[:, 0].any())
    with pytest.raises(ValueError):
        A.sample_deform_params(2, (1, 13, 10), elastic=0.3, elastic_grid=(4, 4, 4))
    with pytest.raises(ValueError):
        A.sample_deform_params(2, (13, 10), elastic=0.3, elastic_grid=(4, 4, 4))


def test_disabled_options_draw_nothing_and_bad_values_raise():
    from mpgan_amd import augment as A
    g = torch.Generator().manual_seed(4)
    state = g.get_state()
    for spatial in ((8, 9), (5, 6, 7)):
        for kw in ({}, dict(elastic_grid=5, bias_grid=7), dict(bias_field=0.3, gamma=0.4, intensity_prob=0.0),
                   dict(bias_field=0.3, gamma=0.4, intensity_planes=()), dict(intensity_prob=0.5)):
            p = A.sample_deform_params(6, spatial, generator=g, **kw)
            assert p == (None, None, None), kw
            assert torch.equal(g.get_state(), state), kw
    # each option alone takes the draws it takes in the full call when the options before it are off
    spatial = (5, 6, 7)
    g1 = torch.Generator().manual_seed(4)
    a = A.sample_deform_params(6, spatial, elastic=0.2, generator=g1)
    b = A.sample_deform_params(6, spatial, bias_field=0.2, generator=g1)
    c = A.sample_deform_params(6, spatial, gamma=0.2, generator=g1)
    g2 = torch.Generator().manual_seed(4)
    full = A.sample_deform_params(6, spatial, elastic=0.2, bias_field=0.2, gamma=0.2, generator=g2)
    assert torch.equal(full.ctrl, a.ctrl) and torch.equal(full.gain, b.gain) and torch.equal(full.gamma, c.gamma)
    assert torch.equal(g1.get_state(), g2.get_state())
    assert a.gain is None and a.gamma is None and b.ctrl is None and c.gain is None
    for bad in (dict(elastic=0.5), dict(elastic=-0.1), dict(elastic=0.2, elastic_grid=3), dict(elastic_grid=65),
                dict(bias_grid=(4, 4)), dict(gamma=-0.1), dict(bias_field=-1.0), dict(intensity_prob=1.5),
                dict(intensity_planes=(2,))):
        with pytest.raises(ValueError):
            A.sample_deform_params(2, spatial, **bad)
    with pytest.raises(ValueError):
        A.sample_deform_params(2, (8,), elastic=0.1)


# ---- the cap on `elastic`: the map does not fold ----------------------------------------------------------------------
@pytest.mark.parametrize("spatial,grid", [((24, 20, 28), (5, 4, 7)), ((16, 16, 16), 4)], ids=str)
def test_the_deformation_does_not_fold_at_the_cap(spatial, grid):
    """elastic = 0.4, the largest value the sampler takes: random lattices from the sampler and lattices with every
    entry at +-0.4 delta.  The central-difference Jacobian determinant of p + u(p) is > 0 at every voxel."""
    from mpgan_amd import augment as A
    n = 6
    ctrl = A.sample_deform_params(n, spatial, elastic=A.ELASTIC_MAX, elastic_grid=grid,
                                  generator=torch.Generator().manual_seed(21)).ctrl.numpy()
    g = ctrl.shape[2:]
    delta = np.array(D.spacing(spatial, g)).reshape(1, 3, 1, 1, 1)
    assert np.abs(ctrl).max() <= 0.4 * delta.max() and (np.abs(ctrl) <= 0.4 * delta).all()
    rng = np.random.default_rng(22)
    signs = np.where(rng.random((n, 3) + g) < 0.5, -1.0, 1.0) * 0.4 * delta
    checker = np.indices(g).sum(0) % 2 * 2.0 - 1.0                    # one lattice alternates from entry to entry
    signs[0] = checker[None] * 0.4 * delta[0]
    low = []
    for lattice in list(ctrl) + list(signs):
        det = D.jacobian_determinant(lattice, spatial)
        low.append(float(det.min()))
        assert det.min() > 0.0, low
    print(f"{spatial} grid {g}: smallest Jacobian determinant {min(low):.3f}")


# ---- the module and the trainer --------------------------------------------------------------------------------------
def test_pair_augment_keeps_the_new_options_apart():
    from mpgan_amd import augment as A
    affine_keys = {"rotate", "scale", "shift", "flip", "prob", "noise_std", "noise_prob"}
    m = A.PairAugment(rotate=0.2, elastic=0.3, elastic_grid=(5, 4, 7), bias_field=0.2, gamma=0.1, intensity_prob=0.5,
                      intensity_keys=("t2w", "t1w"), value_range=(0.0, 1.0))
    assert set(m.options) == affine_keys                               # what sample_affine_params takes
    A.sample_affine_params(2, (8, 9, 10), **m.options)
    assert m.deform_options == dict(elastic=0.3, elastic_grid=(5, 4, 7), bias_field=0.2, bias_grid=4, gamma=0.1,
                                    intensity_prob=0.5)
    A.sample_deform_params(2, (8, 9, 10), intensity_planes=m.intensity_planes, **m.deform_options)
    assert m.intensity_planes == [0, 1] and m.value_range == (0.0, 1.0) and m.deforms and m.last_deform is None
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    plain = A.PairAugment(rotate=0.2)
    assert set(plain.options) == affine_keys and not plain.deforms and plain.intensity_planes == [0]
    assert plain.value_range == (-1.0, 1.0) and "elastic" not in repr(plain) and "elastic=0.3" in repr(m)
    for bad in (dict(elastic=0.5), dict(elastic_grid=3), dict(gamma=-0.1), dict(intensity_keys=("t3w",)),
                dict(bias_field=-0.2), dict(intensity_prob=2.0), dict(value_range=(1.0, 1.0)), dict(bias_grid=(4, 4, 4, 4))):
        with pytest.raises(ValueError):
            A.PairAugment(**bad)
    with pytest.raises(ValueError, match="GPU"):
        A.PairAugment(elastic=0.3)({"t1w": torch.zeros(2, 1, 8, 8), "t2w": torch.zeros(2, 1, 8, 8)})
    with pytest.raises(ValueError, match="GPU"):
        A.deform_warp(torch.zeros(2, 1, 8, 8), torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).repeat(2, 1))


def test_trainer_takes_the_new_keywords(monkeypatch):
    from mpgan_amd import gan as G
    from mpgan_amd.augment import PairAugment
    plain = G.GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu")
    a = G.GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu", pair_augment=dict(elastic=0.3))
    assert isinstance(a.pair_augment, PairAugment) and a.pair_augment.deform_options["elastic"] == 0.3
    assert list(a.state_dict()) == list(plain.state_dict())            # no parameter, no buffer
    assert set(vars(a.hparams)) - set(vars(plain.hparams)) == {"pair_augment"}
    assert vars(a.hparams)["pair_augment"] == dict(elastic=0.3)

    def refuse(*args, **kw):
        raise AssertionError("a network was built")

    monkeypatch.setattr(G, "CasNetGenerator", refuse)
    monkeypatch.setattr(G, "Discriminator", refuse)
    for bad in (dict(elastic=0.9), dict(elastic=0.2, elastic_grid=2), dict(gamma=-1.0), dict(intensity_keys=("t3w",))):
        with pytest.raises(ValueError):
            G.GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu", pair_augment=bad)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def _lib():
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_host_side_refusals_happen_before_any_launch():
    """As test_pair_augment_host.py: the pointers are never dereferenced on these paths."""
    lib = _lib()
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)
    p = 4096                                                           # any non-null address
    ok, grid = i3(1, 8, 8), i3(1, 4, 5)

    def warp(x0=p, x1=p, n=2, in_dhw=ok, out_dhw=ok, theta=p, ctrl=p, ctrl_dhw=grid, gain=p, gain_dhw=grid, gain_planes=1,
             gamma=p, lo=-1.0, hi=1.0, mode=1, noise0=p, noise1=p, sigma=p, y0=p, y1=p):
        return lib.mpgan_deform_warp(x0, x1, n, in_dhw, out_dhw, theta, ctrl, ctrl_dhw, gain, gain_dhw, gain_planes, gamma,
                                     lo, hi, mode, -1.0, -1.0, noise0, noise1, sigma, y0, y1, None)

    cases = [  # everything mpgan_affine_warp refuses
             ({"x0": None}, b"null"), ({"y0": None}, b"null"), ({"theta": None}, b"null"), ({"in_dhw": None}, b"null"),
             ({"out_dhw": None}, b"null"),
             ({"x1": None}, b"y1 alone"), ({"y1": None}, b"x1 alone"),
             ({"n": 0}, b"n = 0"), ({"n": -3}, b"n = -3"),
             ({"in_dhw": i3(0, 8, 8)}, b"input extent"), ({"out_dhw": i3(1, 8, -1)}, b"output extent"),
             ({"mode": 2}, b"mode"), ({"mode": -1}, b"mode"),
             ({"sigma": None}, b"noise without sigma"), ({"noise0": None, "noise1": None}, b"sigma without noise"),
             ({"x1": None, "y1": None}, b"noise1 without the second plane"),
             ({"n": 1024, "in_dhw": i3(128, 128, 128)}, b"input n * D * H * W"),
             ({"n": 1, "out_dhw": i3(2048, 1024, 1024), "ctrl": None, "gain": None}, b"32-bit"),
             # the lattices
             ({"ctrl_dhw": None}, b"ctrl without its size triple"), ({"gain_dhw": None}, b"gain without its size triple"),
             ({"ctrl_dhw": i3(4, 4, 5)}, b"ctrl lattice 4 x 4 x 5: axis 0"),           # D = 1 needs g_d = 1
             ({"ctrl_dhw": i3(1, 3, 5)}, b"ctrl lattice 1 x 3 x 5: axis 1"),
             ({"gain_dhw": i3(1, 4, 65)}, b"gain lattice 1 x 4 x 65: axis 2"),
             ({"gain_dhw": i3(1, 4, 1)}, b"gain lattice 1 x 4 x 1: axis 2"),
             ({"out_dhw": i3(8, 8, 8), "in_dhw": i3(8, 8, 8)}, b"ctrl lattice 1 x 4 x 5: axis 0"),
             # the intensity arguments
             ({"gain_planes": 0}, b"gain with gain_planes == 0"), ({"gain_planes": 4}, b"unknown gain_planes bits"),
             ({"gain_planes": -1}, b"unknown gain_planes bits"),
             ({"gain_planes": 3, "x1": None, "y1": None, "noise1": None}, b"plane 1 without the second plane"),
             ({"hi": -1.0}, b"hi must exceed lo"), ({"hi": -2.0, "gain": None}, b"hi must exceed lo"),
             ({"lo": float("nan"), "ctrl": None, "gain": None}, b"hi must exceed lo")]
    for kw, word in cases:
        assert warp(**kw) == -1, kw
        msg = lib.mpgan_last_error()
        assert b"mpgan_deform_warp" in msg and word in msg, (kw, msg)
