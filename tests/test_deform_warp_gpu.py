"""The elastic deformation and intensity kernel (csrc/pair_augment.hip: mpgan_deform_warp) through augment.deform_warp
against the float64 restatement of tests/deform_ref.py, at the smallest shapes at which it can go wrong: odd extents,
W % 4 != 0, more than one 1 x 8 x 32 tile per axis, in != out sizes, D = 1 (lattice extent 1), lattices of unequal extents.

Bound, on every voxel:  |got - ref| <= 2^-24 |ref| + 1e-11
  2^-24 |ref|   the one fp32 rounding of an fp64 value
  1e-11         the coordinate c = (A p + t) + u(p): <= 4 fp64 roundings of A p + t at magnitude <= 2^8 (1.1e-13 voxels, as
                test_pair_augment_gpu.py); u is a sum of 64 terms of magnitude <= 1.5 whose weights sum to 1 (64 * 1.5 *
                2^-53 = 1.1e-14) with weights of a fraction f that carries the roundings of the lattice coordinate
                xi <= 64 (3 * 2^6 * 2^-53 = 2e-14; |dB/df| <= 3/4, four entries <= 1.5 per axis, three axes: 3e-13).
                Together < 4.5e-13 voxels, times a value slope <= 6 per voxel (data in [-1, 1): 2 per axis): 2.7e-12.
                The gain multiplies v - lo by at most e^0.3 = 1.35: 3.7e-12.  Gamma maps base = (v - lo) / R with the
                slope gamma * base^(gamma - 1): the gamma cases have data in [-0.8, 1) and the fill -0.75, so base >= 0.1 * e^-0.3
                = 0.074 and <= 1.35, gamma in [0.5, 2]: the slope is <= max(0.5 * 0.074^-0.5, 2 * 1.35) = 2.7: 1e-11.
                expm1, pow and the lerps add their own roundings (~1e-15 each).
The cases without gamma stay below 3.7e-12 of that; one bound serves all.
Zero lattices, one plane against two, two runs, views, background and the untouched plane are compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

import deform_ref as D

R = D.R
pytestmark = pytest.mark.gpu

MODES = (D.CONSTANT, D.BORDER)
FILL = -1.0
GAMMA_LOW = -0.8                                     # the data of the gamma cases: base >= 0.1 before the gain
GAMMA_FILL = -0.75                                   # their fill: above GAMMA_LOW, and a float32 (the C ABI's fill is one)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _pair(n, size, low=-1.0):
    """The two planes (fp32, (n, D, H, W) numpy) with values in [low, 1): computed once, never modified."""
    return D.make_input(n, size, seed=0, low=low), D.make_input(n, size, seed=1, low=low)


@functools.lru_cache(maxsize=None)
def _reference(case, mode, plane, intensity):
    """The elastic warp alone (fill -1, data in [-1, 1)), or with gain on both planes and gamma (data >= -0.8, fill -0.75)."""
    n, in_size, out_size, theta, ctrl, gain, gamma = D.CASES[case]
    if not intensity:
        return D.deform_warp_ref(_pair(n, in_size)[plane], theta, out_size, mode, FILL, ctrl=ctrl)
    return D.deform_warp_ref(_pair(n, in_size, GAMMA_LOW)[plane], theta, out_size, mode, GAMMA_FILL, ctrl=ctrl, gain=gain,
                             gamma=gamma[:, plane])


def _dev(a, two_d=False):
    """(n, D, H, W) numpy -> the (n, 1, D, H, W) (or (n, 1, H, W)) device tensor."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = t[:, 0] if two_d else t
    return t.unsqueeze(1).cuda()


def _lattice(a, two_d=False, ctrl=False):
    """A restatement lattice (n, [3,] g_d, g_h, g_w) -> augment.deform_warp's device tensor (2-D: without d)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if two_d:
        t = t[:, 1:, 0] if ctrl else t[:, 0]
    return t.contiguous().cuda()


def _theta(theta, n):
    return torch.as_tensor(np.asarray(theta), dtype=torch.float64).reshape(n, 12).cuda()


def _deform(x0, x1, theta, out_size=None, mode=D.BORDER, fill=FILL, ctrl=None, gain=None, gamma=None, two_d=False, **kw):
    from mpgan_amd import augment as A
    gamma = None if gamma is None else torch.as_tensor(np.asarray(gamma), dtype=torch.float64).cuda()
    return A.deform_warp(x0, _theta(theta, x0.shape[0]), x1, ctrl=_lattice(ctrl, two_d, True), gain=_lattice(gain, two_d),
                         gamma=gamma, out_size=out_size, mode=mode, fill=fill, **kw)


def _affine(x0, x1, theta, out_size=None, mode=D.BORDER, fill=FILL, **kw):
    from mpgan_amd import augment as A
    return A.affine_warp(x0, _theta(theta, x0.shape[0]), x1, out_size=out_size, mode=mode, fill=fill, **kw)


def _check(got, ref, what):
    got = got.detach().cpu().double().numpy().reshape(ref.shape)
    err = np.abs(got - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-11
    worst = float((err / bound).max())
    print(f"{what}: max |got - ref| = {err.max():.3e}, worst err / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, float(err.max()), worst)


# ---- against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(D.CASES))
def test_elastic_cases_against_fp64(case, mode):
    n, in_size, out_size, theta, ctrl, gain, gamma = D.CASES[case]
    assert np.abs(ctrl).max() > 1.4 and np.abs(ctrl).max() <= 1.5
    two_d = in_size[0] == 1
    out = out_size[1:] if two_d else out_size
    x0, x1 = (_dev(a, two_d) for a in _pair(n, in_size))
    y0, y1 = _deform(x0, x1, theta, out, mode, ctrl=ctrl, two_d=two_d)
    assert y0.shape == (n, 1, *out) and y1.shape == y0.shape
    _check(y0, _reference(case, mode, 0, False), f"{case} {mode} elastic plane 0")
    _check(y1, _reference(case, mode, 1, False), f"{case} {mode} elastic plane 1")
    assert not torch.equal(y0, _affine(x0, None, theta, out, mode))     # the lattice moved something
    # one plane and two planes give the same bits; so do two runs
    assert torch.equal(_bits(_deform(x0, None, theta, out, mode, ctrl=ctrl, two_d=two_d)), _bits(y0))
    assert torch.equal(_bits(_deform(x1, None, theta, out, mode, ctrl=ctrl, two_d=two_d)), _bits(y1))
    again = _deform(x0, x1, theta, out, mode, ctrl=ctrl, two_d=two_d)
    assert torch.equal(_bits(again[0]), _bits(y0)) and torch.equal(_bits(again[1]), _bits(y1))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(D.CASES))
def test_elastic_gain_and_gamma_cases_against_fp64(case, mode):
    n, in_size, out_size, theta, ctrl, gain, gamma = D.CASES[case]
    assert gamma.min() >= 0.5 and gamma.max() <= 2.0 and np.abs(gain).max() <= 0.3
    two_d = in_size[0] == 1
    out = out_size[1:] if two_d else out_size
    x0, x1 = (_dev(a, two_d) for a in _pair(n, in_size, GAMMA_LOW))
    assert float(x0.min()) >= GAMMA_LOW and float(x1.min()) >= GAMMA_LOW
    kw = dict(ctrl=ctrl, gain=gain, gamma=gamma, two_d=two_d, gain_planes=(0, 1))
    y0, y1 = _deform(x0, x1, theta, out, mode, GAMMA_FILL, **kw)
    _check(y0, _reference(case, mode, 0, True), f"{case} {mode} elastic + gain + gamma plane 0")
    _check(y1, _reference(case, mode, 1, True), f"{case} {mode} elastic + gain + gamma plane 1")
    again = _deform(x0, x1, theta, out, mode, GAMMA_FILL, **kw)
    assert torch.equal(_bits(again[0]), _bits(y0)) and torch.equal(_bits(again[1]), _bits(y1))
    kw["gain_planes"] = (0,)
    one = _deform(x0, None, theta, out, mode, GAMMA_FILL, **kw)
    assert torch.equal(_bits(one), _bits(y0))
    # gain and gamma apart, and with noise on top
    g0 = _deform(x0, None, theta, out, mode, GAMMA_FILL, gain=gain, two_d=two_d)
    _check(g0, D.deform_warp_ref(_pair(n, in_size, GAMMA_LOW)[0], theta, out_size, mode, GAMMA_FILL, gain=gain), f"{case} gain alone")
    sigma = torch.tensor([[0.05, 0.0]] * n, dtype=torch.float32)
    noise = torch.randn(n, 1, *out, generator=torch.Generator().manual_seed(7))
    z0 = _deform(x0, None, theta, out, mode, GAMMA_FILL, gamma=gamma, two_d=two_d, noise=noise.cuda(), sigma=sigma.cuda())
    ref = D.deform_warp_ref(_pair(n, in_size, GAMMA_LOW)[0], theta, out_size, mode, GAMMA_FILL, gamma=gamma[:, 0])
    _check(z0, ref + float(sigma[0, 0]) * noise.double().numpy().reshape(ref.shape), f"{case} gamma alone + noise")


# ---- bit for bit ------------------------------------------------------------------------------------------------------
def _rotated_theta(n, size):
    return np.stack([R.theta_from_params((0.4, -0.3, 0.5), 1.1, (0.3, -0.2, 0.1), in_size=size),
                     R.theta_from_params((-0.7, 0.2, 0.1), 0.9, (-1.4, 0.6, 2.2), in_size=size)][:n])


@pytest.mark.parametrize("mode", MODES)
def test_zero_lattices_and_gamma_one_give_affine_warps_bits(mode):
    size = (5, 9, 35)                                   # more than one tile along d, h and w; W % 4 != 0
    x0, x1 = (_dev(a) for a in _pair(2, size))
    theta = _rotated_theta(2, size)
    want = _affine(x0, x1, theta, mode=mode)
    sigma = torch.tensor([[0.1, 0.2], [0.0, 0.3]], dtype=torch.float32).cuda()
    noise = [torch.randn(2, 1, *size, generator=torch.Generator().manual_seed(k)).cuda() for k in (1, 2)]
    noisy = _affine(x0, x1, theta, mode=mode, noise=noise, sigma=sigma)
    zc, zg, ones = np.zeros((2, 3, 4, 5, 6)), np.zeros((2, 4, 4, 5)), np.ones((2, 2))
    for kw in (dict(), dict(ctrl=zc), dict(gain=zg, gain_planes=(0, 1)), dict(gamma=ones),
               dict(ctrl=zc, gain=zg, gamma=ones, gain_planes=(0, 1))):
        y = _deform(x0, x1, theta, mode=mode, **kw)
        assert torch.equal(_bits(y[0]), _bits(want[0])) and torch.equal(_bits(y[1]), _bits(want[1])), list(kw)
        y = _deform(x0, x1, theta, mode=mode, noise=noise, sigma=sigma, **kw)
        assert torch.equal(_bits(y[0]), _bits(noisy[0])) and torch.equal(_bits(y[1]), _bits(noisy[1])), list(kw)
    # 2-D
    a0, a1 = (_dev(a, two_d=True) for a in _pair(3, (1, 13, 10)))
    th = R.CASES["rot2d"][3]
    y = _deform(a0, a1, th, mode=mode, ctrl=np.zeros((3, 3, 1, 4, 5)), gain=np.zeros((3, 1, 4, 4)), gamma=np.ones((3, 2)), two_d=True)
    want = _affine(a0, a1, th, mode=mode)
    assert torch.equal(_bits(y[0]), _bits(want[0])) and torch.equal(_bits(y[1]), _bits(want[1]))


def _offset_view(t):
    """A contiguous copy of t that starts 4 (float32) or 8 (float64) bytes into its allocation."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


@pytest.mark.parametrize("mode", MODES)
def test_unaligned_views_give_the_same_bits(mode):
    from mpgan_amd import ops
    n, in_size, out_size, theta, ctrl, gain, gamma = D.CASES["ffd3d"]   # W = 11: W % 4 != 0
    x0, x1 = (_dev(a) for a in _pair(n, in_size))
    th, c, g, gm = _theta(theta, n), _lattice(ctrl), _lattice(gain), torch.from_numpy(gamma).cuda()
    sigma = torch.tensor([[0.1, 0.2], [0.3, 0.0]], dtype=torch.float32).cuda()
    noise = torch.randn(2, n, 1, *out_size, generator=torch.Generator().manual_seed(8)).cuda()
    m = ops.WARP_BORDER if mode == D.BORDER else ops.WARP_CONSTANT
    y = ops.deform_warp(x0, x1, th, c, g, 3, gm, -1.0, 1.0, m, FILL, FILL, noise[0], noise[1], sigma, torch.empty_like(x0),
                        torch.empty_like(x0))
    o = _offset_view
    v = ops.deform_warp(o(x0), o(x1), th, o(c), o(g), 3, gm, -1.0, 1.0, m, FILL, FILL, o(noise[0]), o(noise[1]), sigma,
                        o(torch.empty_like(x0)), o(torch.empty_like(x0)))
    assert torch.equal(_bits(v[0]), _bits(y[0])) and torch.equal(_bits(v[1]), _bits(y[1]))


@pytest.mark.parametrize("mode", MODES)
def test_background_stays_background_and_the_other_plane_is_untouched(mode):
    size, n = (6, 12, 40), 2
    box = (slice(None), slice(1, 5), slice(3, 10), slice(5, 34))
    x = np.full((n,) + size, -1.0, dtype=np.float32)
    x[box] = _pair(n, size, GAMMA_LOW)[0][box]
    x0, x1 = _dev(x), _dev(_pair(n, size)[1])
    eye = np.tile(np.eye(3, 4).reshape(1, 12), (n, 1))
    rng = np.random.default_rng(3)
    gain = (rng.random((n, 4, 5, 6)) * 2 - 1) * 0.3
    gamma = np.array([[0.6, 1.0]] * n)
    y0, y1 = _deform(x0, x1, eye, mode=mode, ctrl=np.zeros((n, 3, 4, 4, 4)), gain=gain, gamma=gamma, gain_planes=(0,))
    outside = torch.from_numpy(x == -1.0).unsqueeze(1)
    assert int(outside.sum()) > x.size // 2
    assert bool((y0.cpu()[outside] == -1.0).all())                      # every background voxel is exactly -1.0
    ref = D.deform_warp_ref(x, eye, size, mode, FILL, gain=gain, gamma=gamma[:, 0])
    _check(y0, ref, f"background {mode}")
    inside = ~outside
    assert not bool((y0.cpu()[inside] == x0.cpu()[inside]).all())      # the box did change
    # plane 1: outside gain_planes and gamma exactly 1 -- the bits of the call without gain (here: of the input)
    assert torch.equal(_bits(y1), _bits(_deform(x0, x1, eye, mode=mode, gamma=gamma)[1]))
    assert torch.equal(_bits(y1), _bits(x1))
    rot = _rotated_theta(n, size)
    with_gain = _deform(x0, x1, rot, mode=mode, gain=gain, gain_planes=(0,))
    without = _deform(x0, x1, rot, mode=mode)
    assert torch.equal(_bits(with_gain[1]), _bits(without[1])) and not torch.equal(with_gain[0], without[0])
    swapped = _deform(x0, x1, rot, mode=mode, gain=gain, gain_planes=(1,))
    assert torch.equal(_bits(swapped[0]), _bits(without[0])) and not torch.equal(swapped[1], without[1])


# ---- a ramp reads the map ---------------------------------------------------------------------------------------------
def test_a_ramp_reads_the_displacement():
    size, n = (5, 9, 35), 2
    w = np.arange(size[2], dtype=np.float64)
    x = np.broadcast_to((w / 64.0).astype(np.float32), (n,) + size).copy()        # exact in fp32
    rng = np.random.default_rng(5)
    ctrl = np.zeros((n, 3, 4, 5, 6))
    ctrl[:, 2] = (rng.random((n, 4, 5, 6)) * 2 - 1) * 1.5
    eye = np.tile(np.eye(3, 4).reshape(1, 12), (n, 1))
    y = _deform(_dev(x), None, eye, mode=D.BORDER, ctrl=ctrl).cpu().double().numpy().reshape((n,) + size)
    u = np.stack([D.displacement(ctrl[s], size)[2] for s in range(n)])
    c = w + u
    inside = (c >= 0.0) & (c <= size[2] - 1.0)
    assert 0.5 < inside.mean() < 1.0 and np.abs(u).max() > 0.5
    # x is linear in w with the slope 1/64, so y = (w + u_w) / 64 wherever c stays inside: the bound on y, times 64
    err = np.abs(y * 64.0 - w - u)[inside]
    bound = (2.0 ** -24 * np.abs(c / 64.0) + 1e-11)[inside] * 64.0
    print(f"ramp: max |y * 64 - w - u_w| = {err.max():.3e}, worst err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


# ---- launch paths -----------------------------------------------------------------------------------------------------
def test_many_tiles_per_sample():
    """(9, 17, 70): 9 * 3 * 3 tiles of 1 x 8 x 32 per sample, ragged along h and w, lattices of the largest and the
    smallest extents."""
    size, n = (9, 17, 70), 2
    rng = np.random.default_rng(6)
    ctrl = (rng.random((n, 3, 4, 64, 9)) * 2 - 1) * 0.4
    gain = (rng.random((n, 7, 4, 64)) * 2 - 1) * 0.3
    gamma = np.array([[0.7, 1.5], [1.0, 2.0]])
    theta = _rotated_theta(n, size)
    x = _pair(n, size, GAMMA_LOW)
    y0, y1 = _deform(_dev(x[0]), _dev(x[1]), theta, mode=D.BORDER, ctrl=ctrl, gain=gain, gamma=gamma, gain_planes=(0, 1))
    for k, y in enumerate((y0, y1)):
        ref = D.deform_warp_ref(x[k], theta, size, D.BORDER, FILL, ctrl=ctrl, gain=gain, gamma=gamma[:, k])
        _check(y, ref, f"many tiles plane {k}")


# ---- the function and the module --------------------------------------------------------------------------------------
def test_deform_warp_refuses_what_it_cannot_do():
    from mpgan_amd import augment as A
    x = torch.zeros(2, 1, 8, 8, device="cuda")
    th = torch.eye(3, 4, dtype=torch.float64, device="cuda").reshape(1, 12).repeat(2, 1)
    ctrl = torch.zeros(2, 2, 4, 4, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="differentiable"):
        A.deform_warp(x.clone().requires_grad_(True), th, ctrl=ctrl)
    with torch.no_grad():
        assert torch.equal(A.deform_warp(x.clone().requires_grad_(True), th, ctrl=ctrl), x)
    for bad in (dict(ctrl=ctrl.float()), dict(ctrl=ctrl[:, :1]), dict(ctrl=ctrl[:1]), dict(ctrl=ctrl[..., :3]),
                dict(ctrl=torch.zeros(2, 3, 1, 4, 4, dtype=torch.float64, device="cuda")), dict(gain=ctrl),
                dict(gain=ctrl[:, 0], gain_planes=()), dict(gain=ctrl[:, 0], gain_planes=(1,)),
                dict(gain=ctrl[:, 0], gain_planes=(2,)), dict(gain=ctrl[:, 0], value_range=(1.0, -1.0)),
                dict(gamma=torch.ones(2, 2, device="cuda")), dict(gamma=torch.ones(2, 1, dtype=torch.float64, device="cuda")),
                dict(ctrl=ctrl.cpu()), dict(mode="reflect")):
        with pytest.raises(ValueError):
            A.deform_warp(x, th, **bad)


def test_pair_augment_module_replays_from_its_draws():
    from mpgan_amd import augment as A
    g = torch.Generator().manual_seed(3)
    shape = (3, 1, 6, 20, 12)
    batch = {k: (torch.rand(*shape, generator=g) * 1.8 - 0.8).cuda() for k in ("t1w", "t2w")}
    batch["name"] = "kept"
    m = A.PairAugment(rotate=0.4, scale=0.2, prob=0.7, noise_std=0.1, mode="constant", elastic=0.4, elastic_grid=(4, 6, 5),
                      bias_field=0.3, gamma=0.3, intensity_prob=0.6, generator=torch.Generator(device="cuda").manual_seed(12))
    out = m(batch)
    assert out is not batch and out["name"] == "kept" and set(out) == set(batch)
    # the draw order: the affine parameters, the lattices, the noise field
    replay = torch.Generator(device="cuda").manual_seed(12)
    p = A.sample_affine_params(3, shape[2:], generator=replay, device="cuda", noise_planes=[0], **m.options)
    eye = torch.eye(3, 4, dtype=torch.float64, device="cuda").reshape(1, 12)
    gate = ~(p.theta == eye).all(1)
    q = A.sample_deform_params(3, shape[2:], generator=replay, device="cuda", intensity_planes=[0], spatial_gate=gate,
                               **m.deform_options)
    field = torch.randn((1, *shape), generator=replay, device="cuda")
    assert isinstance(m.last_params, A.AffineParams) and isinstance(m.last_deform, A.DeformParams)
    assert torch.equal(p.theta, m.last_params.theta) and torch.equal(p.sigma, m.last_params.sigma)
    assert all(torch.equal(a, b) for a, b in zip(q, m.last_deform)) and torch.equal(field, m.last_noise)
    assert q.ctrl.shape == (3, 3, 4, 6, 5) and q.gain.shape == (3, 4, 4, 4) and bool((q.gamma[:, 1] == 1.0).all())
    assert not bool(q.ctrl[~gate].any())                               # no map, no deformation
    y1, y2 = A.deform_warp(batch["t1w"], p.theta, batch["t2w"], ctrl=q.ctrl, gain=q.gain, gamma=q.gamma, mode="constant",
                           fill=-1.0, noise=field[0], sigma=p.sigma)
    assert torch.equal(_bits(out["t1w"]), _bits(y1)) and torch.equal(_bits(out["t2w"]), _bits(y2))
    assert not out["t1w"].requires_grad and not torch.equal(out["t2w"], batch["t2w"])
    # t2w gets the spatial map alone
    assert torch.equal(_bits(y2), _bits(A.deform_warp(batch["t2w"], p.theta, ctrl=q.ctrl, mode="constant", fill=-1.0)))
    # everything gated off: a bit copy in new tensors, nothing drawn
    gen = torch.Generator(device="cuda").manual_seed(1)
    state = gen.get_state()
    off = A.PairAugment(rotate=0.4, prob=0.0, elastic=0.3, bias_field=0.3, gamma=0.3, intensity_prob=0.0, generator=gen)
    res = off(batch)
    assert torch.equal(_bits(res["t1w"]), _bits(batch["t1w"])) and res["t1w"].data_ptr() != batch["t1w"].data_ptr()
    assert torch.equal(_bits(res["t2w"]), _bits(batch["t2w"])) and off.last_deform == (None, None, None)
    assert torch.equal(gen.get_state(), state)
    # every new option off: the affine launch, the draws and the attributes of before
    plain = A.PairAugment(rotate=0.4, noise_std=0.1, generator=torch.Generator(device="cuda").manual_seed(5))
    res = plain(batch)
    replay = torch.Generator(device="cuda").manual_seed(5)
    p = A.sample_affine_params(3, shape[2:], generator=replay, device="cuda", noise_planes=[0], **plain.options)
    field = torch.randn((1, *shape), generator=replay, device="cuda")
    want = A.affine_warp(batch["t1w"], p.theta, batch["t2w"], noise=field[0], sigma=p.sigma)
    assert plain.last_deform is None and isinstance(plain.last_params, A.AffineParams)
    assert torch.equal(_bits(res["t1w"]), _bits(want[0])) and torch.equal(_bits(res["t2w"]), _bits(want[1]))
