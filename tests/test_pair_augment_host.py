"""Paired affine augmentation, everything that needs no GPU: the float64 restatement (tests/affine_ref.py) against
torch's grid_sample and scipy's affine_transform, the coverage of the GPU tests' cases, the sampler on the CPU, the
trainer option's defaults, and the library's host-side refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import affine_ref as R


# ---- the restatement ------------------------------------------------------------------------------------------------
def _grid_sample(x, theta, out_size, padding_mode):
    """torch.nn.functional.grid_sample(align_corners=True) in float64 at the restatement's coordinates (an extent-1
    axis is dropped: its normalised coordinate does not exist)."""
    n, S = x.shape[0], x.shape[1:]
    keep = [k for k in range(3) if S[k] > 1]
    out = []
    for s in range(n):
        c = R.coords(theta[s], out_size)
        assert all(np.all(c[k] == 0) for k in range(3) if k not in keep)
        norm = [2.0 * c[k] / (S[k] - 1) - 1.0 for k in reversed(keep)]                 # (x, y, z) = (w, h, d)
        grid = torch.from_numpy(np.stack(norm, -1))
        grid = grid.reshape(1, *[out_size[k] for k in keep], len(keep))
        img = torch.from_numpy(np.asarray(x[s], dtype=np.float64)).reshape(1, 1, *[S[k] for k in keep])
        y = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode=padding_mode, align_corners=True)
        out.append(y.reshape(out_size).numpy())
    return np.stack(out)


@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("mode,padding", [(R.CONSTANT, "zeros"), (R.BORDER, "border")])
def test_restatement_equals_grid_sample(case, mode, padding):
    n, in_size, out_size, theta = R.CASES[case]
    x = R.make_input(n, in_size)
    got = R.affine_warp_ref(x, theta, out_size, mode, fill=0.0)
    want = _grid_sample(x, theta, out_size, padding)
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("mode,scipy_mode", [(R.CONSTANT, "grid-constant"), (R.BORDER, "nearest")])
def test_restatement_equals_scipy(case, mode, scipy_mode):
    ndimage = pytest.importorskip("scipy.ndimage")
    n, in_size, out_size, theta = R.CASES[case]
    x = R.make_input(n, in_size).astype(np.float64)
    got = R.affine_warp_ref(x, theta, out_size, mode, fill=0.0)
    for s in range(n):
        th = theta[s].reshape(3, 4)
        want = ndimage.affine_transform(x[s], th[:, :3], offset=th[:, 3], output_shape=out_size, order=1, mode=scipy_mode,
                                        cval=0.0)
        assert np.abs(got[s] - want).max() <= 1e-12, s


def test_restatement_fill_and_identity():
    n, in_size, out_size, theta = R.CASES["rot3d"]
    x = R.make_input(n, in_size)
    a = R.affine_warp_ref(x, theta, out_size, R.CONSTANT, fill=-1.0)
    b = R.affine_warp_ref(x.astype(np.float64) + 1.0, theta, out_size, R.CONSTANT, fill=0.0) - 1.0     # linear in (x, fill)
    assert np.abs(a - b).max() <= 1e-12
    eye = np.tile(np.eye(3, 4).reshape(1, 12), (n, 1))
    for mode in (R.CONSTANT, R.BORDER):
        assert np.array_equal(R.affine_warp_ref(x, eye, in_size, mode, fill=7.0), x.astype(np.float64))


def test_the_gpu_cases_cover_inside_partial_and_outside():
    """Pooled over the samples of each rotated case: the GPU tests cannot pass on inputs that never leave the image, or
    never stay in it."""
    for case in R.ROTATED_CONSTANT:
        n, in_size, out_size, theta = R.CASES[case]
        inside, partial, outside = R.corner_shares(theta, in_size, out_size)
        assert 0.2 <= inside <= 0.8, (case, inside)
        assert partial >= 0.1, (case, partial)
        assert outside >= 0.05, (case, outside)
        assert abs(np.abs(R.coords(theta[0], out_size)).max()) <= 2.0 ** 8         # the bound's coordinate magnitude
    assert R.corner_shares(R.CASES["crop"][3], R.CASES["crop"][1], R.CASES["crop"][2]) == (1.0, 0.0, 0.0)
    # 2-D: the d row and column of the table's theta are neutral
    th = R.CASES["rot2d"][3].reshape(-1, 3, 4)
    assert np.array_equal(th[:, 0], np.tile([1.0, 0, 0, 0], (3, 1))) and not th[:, 1:, 0].any()


# ---- the sampler ------------------------------------------------------------------------------------------------------
FULL = dict(rotate=(0.3, 0.2, 0.5), scale=0.2, shift=(0.1, 0.05, 0.2), flip=(0, 2), prob=0.7, noise_std=0.1, noise_prob=0.6,
            noise_planes=(0, 1))


def _params_from_draws(n, spatial, opts, seed):
    """Replay the documented draw order with plain torch.rand calls and build theta with the restatement."""
    g = torch.Generator().manual_seed(seed)
    ndim = len(spatial)
    S = (1,) * (3 - ndim) + tuple(spatial)
    first = 3 - ndim
    rand = lambda *shape: torch.rand(shape, generator=g, dtype=torch.float64).numpy()
    prob = opts.get("prob", 1.0)
    if prob == 0:                                     # no spatial op draws at all
        opts = {k: v for k, v in opts.items() if k.startswith("noise")}
    rot = opts.get("rotate", 0.0)
    rot = ([rot, 0.0, 0.0] if ndim == 2 else [rot] * 3) if isinstance(rot, (int, float)) else list(rot)
    angles = np.zeros((n, 3))
    if any(r > 0 for r in rot):
        u = rand(n, 3 if ndim == 3 else 1)
        for k in range(u.shape[1]):
            angles[:, k] = (2 * u[:, k] - 1) * rot[k]
    scale = np.ones(n)
    if opts.get("scale", 0.0) > 0:
        scale = 1 + opts["scale"] * (2 * rand(n) - 1)
    sh = opts.get("shift", 0.0)
    sh = [sh] * ndim if isinstance(sh, (int, float)) else list(sh)
    shift = np.zeros((n, 3))
    if any(f > 0 for f in sh):
        u = rand(n, ndim)
        for k in range(ndim):
            shift[:, first + k] = (2 * u[:, k] - 1) * (sh[k] * S[first + k])
    flips = np.ones((n, 3))
    axes = sorted(opts.get("flip", ()))
    if axes:
        u = rand(n, len(axes))
        for j, a in enumerate(axes):
            flips[:, first + a] = np.where(u[:, j] < 0.5, -1.0, 1.0)
    on = np.ones(n, dtype=bool)
    if 0 < prob < 1:
        on = rand(n) < prob
    theta = np.stack([R.theta_from_params(angles[s], scale[s], shift[s], flips[s], in_size=S) if on[s]
                      else np.eye(3, 4).reshape(12) for s in range(n)])
    sigma = np.zeros((n, 2))
    planes = sorted(opts.get("noise_planes", (0,)))
    if opts.get("noise_std", 0.0) > 0 and opts.get("noise_prob", 1.0) > 0:
        draw = rand(n, len(planes)) * opts["noise_std"]
        if opts.get("noise_prob", 1.0) < 1:
            draw = np.where(rand(n, len(planes)) < opts["noise_prob"], draw, 0.0)
        for j, k in enumerate(planes):
            sigma[:, k] = draw[:, j]
    return dict(theta=theta, sigma=sigma.astype(np.float32), angles=angles, scale=scale, shift=shift, flips=flips, on=on)


@pytest.mark.parametrize("spatial", [(9, 12, 7), (128, 128, 128)], ids=str)
def test_sample_affine_params_3d(spatial):
    from mpgan_amd import augment as A
    n = 400
    p = A.sample_affine_params(n, spatial, generator=torch.Generator().manual_seed(9), **FULL)
    assert p.theta.dtype == torch.float64 and p.theta.shape == (n, 12) and p.theta.is_contiguous()
    assert p.sigma.dtype == torch.float32 and p.sigma.shape == (n, 2) and p.sigma.is_contiguous()
    want = _params_from_draws(n, spatial, FULL, 9)                    # the draw order and the convention
    assert np.abs(p.theta.numpy() - want["theta"]).max() <= 1e-12
    assert np.array_equal(p.sigma.numpy(), want["sigma"])
    # ranges and gates (from the replay's intermediate draws, which the line above ties to the sampler)
    top = np.abs(want["angles"]).max(0)
    assert (top <= np.array(FULL["rotate"])).all() and (top > 0.8 * np.array(FULL["rotate"])).all()
    assert 0.8 <= want["scale"].min() < 0.85 and 1.15 < want["scale"].max() <= 1.2
    for k in range(3):
        lim = FULL["shift"][k] * spatial[k]
        assert np.abs(want["shift"][:, k]).max() <= lim and np.abs(want["shift"][:, k]).max() > 0.8 * lim
    assert set(np.unique(want["flips"][:, 0])) == {-1.0, 1.0} == set(np.unique(want["flips"][:, 2]))
    assert np.all(want["flips"][:, 1] == 1.0)
    assert 0.6 < want["on"].mean() < 0.8
    off = ~torch.from_numpy(want["on"])
    eye = torch.eye(3, 4, dtype=torch.float64).reshape(1, 12)
    assert torch.equal(p.theta[off], eye.expand(int(off.sum()), 12))  # gated off: exactly (I | 0)
    assert not bool((p.theta[~off] == eye).all(1).any())
    sig = p.sigma.numpy()
    assert sig.min() >= 0 and sig.max() < FULL["noise_std"] and sig.max() > 0.9 * FULL["noise_std"]
    assert 0.5 < (sig > 0).mean() < 0.7                               # noise_prob per plane
    # determinism from the generator
    again = A.sample_affine_params(n, spatial, generator=torch.Generator().manual_seed(9), **FULL)
    assert torch.equal(again.theta, p.theta) and torch.equal(again.sigma, p.sigma)
    g = torch.Generator().manual_seed(9)
    A.sample_affine_params(n, spatial, generator=g, **FULL)
    other = A.sample_affine_params(n, spatial, generator=g, **FULL)   # the generator has moved on
    assert not torch.equal(other.theta, p.theta)


def test_sample_affine_params_2d():
    from mpgan_amd import augment as A
    opts = dict(rotate=0.6, scale=0.25, shift=0.1, flip=(1,), noise_std=0.05)
    n, spatial = 64, (13, 10)
    p = A.sample_affine_params(n, spatial, generator=torch.Generator().manual_seed(2), **opts)
    want = _params_from_draws(n, spatial, opts, 2)
    assert np.abs(p.theta.numpy() - want["theta"]).max() <= 1e-12
    th = p.theta.view(n, 3, 4)
    assert th[:, 0].tolist() == [[1.0, 0.0, 0.0, 0.0]] * n and th[:, 1:, 0].tolist() == [[0.0, 0.0]] * n
    assert np.abs(want["angles"][:, 0]).max() > 0.5 and not want["angles"][:, 1:].any()
    assert bool((p.sigma[:, 0] > 0).all()) and not bool(p.sigma[:, 1].any())       # the default plane is t1w's
    with pytest.raises(ValueError, match="rotate"):
        A.sample_affine_params(2, spatial, rotate=(0.1, 0.2, 0.3))


def test_sample_affine_params_disabled_ops_draw_nothing():
    from mpgan_amd import augment as A
    eye = torch.eye(3, 4, dtype=torch.float64).reshape(1, 12)
    g = torch.Generator().manual_seed(4)
    state = g.get_state()
    for spatial in ((8, 9), (5, 6, 7)):
        for kw in ({}, dict(prob=0.0, rotate=0.5, scale=0.3, shift=0.2, flip=(0, 1)), dict(noise_std=0.3, noise_prob=0.0),
                   dict(noise_std=0.3, noise_planes=())):
            p = A.sample_affine_params(6, spatial, generator=g, **kw)
            assert torch.equal(p.theta, eye.expand(6, 12)) and not bool(p.sigma.any()), kw
            assert torch.equal(g.get_state(), state), kw              # nothing was drawn
    # the draw order that replays rely on: rotate, scale, shift, flip, the gate, sigma, its gate -- each op alone takes
    # the draws it takes in the full call when the ops before it are disabled
    spatial = (5, 6, 7)
    g1 = torch.Generator().manual_seed(4)
    only_rot = A.sample_affine_params(6, spatial, rotate=FULL["rotate"], generator=g1)
    only_scale = A.sample_affine_params(6, spatial, scale=0.2, generator=g1)
    g2 = torch.Generator().manual_seed(4)
    both = A.sample_affine_params(6, spatial, rotate=FULL["rotate"], scale=0.2, generator=g2)
    A1, A2, A12 = (t.theta.view(6, 3, 4)[:, :, :3] for t in (only_rot, only_scale, both))
    s = 1.0 / A2[:, 0, 0]
    assert torch.allclose(A12, A1 / s[:, None, None], rtol=0, atol=1e-14)
    assert torch.equal(g1.get_state(), g2.get_state())
    # noise alone leaves theta neutral; the spatial ops alone leave sigma 0
    p = A.sample_affine_params(6, spatial, noise_std=0.1, generator=g1)
    assert torch.equal(p.theta, eye.expand(6, 12)) and bool((p.sigma[:, 0] > 0).all())
    assert not bool(both.sigma.any())
    for bad in (dict(scale=1.0), dict(scale=-0.1), dict(prob=1.5), dict(rotate=-1.0), dict(flip=(3,)), dict(noise_std=-1.0),
                dict(noise_planes=(2,)), dict(shift=(0.1, 0.1))):
        with pytest.raises(ValueError):
            A.sample_affine_params(2, spatial, **bad)
    with pytest.raises(ValueError):
        A.sample_affine_params(2, (8,))


def test_flips_are_exact_index_reversals():
    from mpgan_amd import augment as A
    spatial = (4, 7, 10)
    p = A.sample_affine_params(64, spatial, flip=(0, 1, 2), generator=torch.Generator().manual_seed(3))
    th = p.theta.view(64, 3, 4)
    seen = set()
    for s in range(64):
        sign = []
        for k in range(3):
            row = th[s, k].tolist()
            f = row[k]
            assert f in (1.0, -1.0) and all(row[j] == 0 for j in range(3) if j != k)
            assert row[3] == (0.0 if f > 0 else spatial[k] - 1.0)      # c = S - 1 - p: exact
            sign.append(f)
        seen.add(tuple(sign))
        x = R.make_input(1, spatial, seed=s)
        want = np.flip(x, [k + 1 for k in range(3) if sign[k] < 0])
        for mode in (R.CONSTANT, R.BORDER):
            assert np.array_equal(R.affine_warp_ref(x, th[s].reshape(1, 12).numpy(), spatial, mode, fill=9.0), want)
    assert len(seen) == 8


# ---- the function and the module -------------------------------------------------------------------------------------
def test_there_is_no_cpu_path():
    from mpgan_amd import augment as A
    p = A.sample_affine_params(2, (8, 8), rotate=0.3)
    with pytest.raises(ValueError, match="GPU"):
        A.affine_warp(torch.zeros(2, 1, 8, 8), p.theta)
    with pytest.raises(ValueError, match="GPU"):
        A.PairAugment(rotate=0.3)({"t1w": torch.zeros(2, 1, 8, 8), "t2w": torch.zeros(2, 1, 8, 8)})


def test_pair_augment_module_options():
    from mpgan_amd import augment as A
    m = A.PairAugment(rotate=0.2, noise_std=0.1, noise_keys=("t2w", "t1w"))
    assert m.noise_planes == [0, 1] and m.mode == "border" and m.fill == -1.0 and m.last_params is None
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    assert A.PairAugment(rotate=(0.1, 0.2, 0.3), flip=(2,)).options["rotate"] == (0.1, 0.2, 0.3)
    for bad in (dict(noise_keys=("t3w",)), dict(mode="reflect"), dict(scale=1.5), dict(prob=-0.1), dict(flip=(5,))):
        with pytest.raises(ValueError):
            A.PairAugment(**bad)


# ---- the trainer option ---------------------------------------------------------------------------------------------
def test_trainer_defaults_and_hparams():
    from mpgan_amd.augment import PairAugment
    from mpgan_amd.gan import GAN
    g = GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu")
    assert g.hparams.pair_augment is None and "pair_augment" not in vars(g.hparams)
    assert g.pair_augment is None and g.aug_generator is None
    assert not any(isinstance(m, PairAugment) for m in g.modules())
    keys = list(g.state_dict())
    opts = dict(rotate=0.3, scale=0.1, flip=(1,), noise_std=0.05, mode="constant", fill=-1.0)
    a = GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu", pair_augment=opts)
    assert vars(a.hparams)["pair_augment"] == opts and vars(a.hparams)["pair_augment"] is not opts
    assert isinstance(a.pair_augment, PairAugment) and a.pair_augment.mode == "constant"
    assert a.pair_augment.options["rotate"] == 0.3 and a.pair_augment.noise_planes == [0]
    assert list(a.state_dict()) == keys                              # no parameter, no buffer
    assert a.aug_generator is None and a.augment is None
    assert set(vars(a.hparams)) - set(vars(g.hparams)) == {"pair_augment"}
    both = GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu", pair_augment={}, diff_augment="color")
    assert both.pair_augment is not None and both.augment is not None


def test_a_bad_pair_augment_option_raises_before_anything_is_built(monkeypatch):
    from mpgan_amd import gan as G

    def refuse(*a, **k):
        raise AssertionError("a network was built")

    monkeypatch.setattr(G, "CasNetGenerator", refuse)
    monkeypatch.setattr(G, "Discriminator", refuse)
    for bad in (dict(rotation=0.3), dict(rotate=0.3, generator=None), dict(scale=2.0), dict(mode="zeros"), "rotate", ["rotate"]):
        with pytest.raises(ValueError):
            G.GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu", pair_augment=bad)


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def _lib():
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_host_side_refusals_happen_before_any_launch():
    """As test_capi_symbols.py::test_error_reporting_without_gpu: the pointers are never dereferenced on these paths."""
    lib = _lib()
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)
    p = 4096                                                           # any non-null address
    ok = i3(1, 8, 8)

    def warp(x0=p, x1=p, n=2, in_dhw=ok, out_dhw=ok, theta=p, mode=1, noise0=p, noise1=p, sigma=p, y0=p, y1=p):
        return lib.mpgan_affine_warp(x0, x1, n, in_dhw, out_dhw, theta, mode, -1.0, -1.0, noise0, noise1, sigma, y0, y1, None)

    cases = [({"x0": None}, b"null"), ({"y0": None}, b"null"), ({"theta": None}, b"null"), ({"in_dhw": None}, b"null"),
             ({"out_dhw": None}, b"null"),
             ({"x1": None}, b"y1 alone"), ({"y1": None}, b"x1 alone"),
             ({"n": 0}, b"n = 0"), ({"n": -3}, b"n = -3"),
             ({"in_dhw": i3(0, 8, 8)}, b"input extent"), ({"out_dhw": i3(1, 8, -1)}, b"output extent"),
             ({"mode": 2}, b"mode"), ({"mode": -1}, b"mode"),
             ({"sigma": None}, b"noise without sigma"), ({"sigma": None, "noise0": None}, b"noise without sigma"),
             ({"noise0": None, "noise1": None}, b"sigma without noise"),
             ({"x1": None, "y1": None}, b"noise1 without the second plane"),
             ({"n": 1024, "in_dhw": i3(128, 128, 128)}, b"input n * D * H * W"),
             ({"n": 1024, "out_dhw": i3(128, 128, 128)}, b"output n * D * H * W"),
             ({"n": 1, "out_dhw": i3(2048, 1024, 1024)}, b"32-bit")]
    for kw, word in cases:
        assert warp(**kw) == -1, kw
        msg = lib.mpgan_last_error()
        assert b"mpgan_affine_warp" in msg and word in msg, (kw, msg)
