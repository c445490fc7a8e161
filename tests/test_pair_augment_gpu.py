"""The paired affine warp (csrc/pair_augment.hip) through ops.affine_warp and augment.affine_warp against the float64
restatement of tests/affine_ref.py, at the smallest shapes at which it can go wrong: odd extents, W % 4 != 0, extents
that are no multiple of the 4 x 8 x 32 tile, more than one tile per sample, in != out sizes, D = 1.

Bound, on every voxel:  |got - ref| <= 2^-24 |ref| + 1e-11
  2^-24 |ref|   the one fp32 rounding of an fp64 value
  1e-11         <= 4 fp64 roundings of a coordinate of magnitude <= 2^8 (4 * 2^8 * 2^-53 = 1.1e-13 voxels) times a value
                slope <= 6 per voxel (data in [-1, 1): 2 per axis), plus the lerps' own roundings (~1e-15): < 1e-12
Integer-valued maps (identity, flips, quarter turns, integer shifts) are compared bit for bit with torch index ops."""
import functools
import itertools

import numpy as np
import pytest
import torch

import affine_ref as R

pytestmark = pytest.mark.gpu

MODES = (R.CONSTANT, R.BORDER)
FILL = -1.0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _pair(n, size):
    """The two planes (fp32, (n, D, H, W) numpy): computed once, never modified."""
    return R.make_input(n, size, seed=0), R.make_input(n, size, seed=1)


@functools.lru_cache(maxsize=None)
def _reference(case, mode, plane):
    n, in_size, out_size, theta = R.CASES[case]
    return R.affine_warp_ref(_pair(n, in_size)[plane], theta, out_size, mode, FILL)


def _dev(a, two_d=False):
    """(n, D, H, W) numpy -> the (n, 1, D, H, W) (or (n, 1, H, W)) device tensor."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = t[:, 0] if two_d else t
    return t.unsqueeze(1).cuda()


def _warp(x0, x1, theta, out_size=None, mode=R.BORDER, fill=FILL, **kw):
    from mpgan_amd import augment as A
    th = torch.as_tensor(np.asarray(theta), dtype=torch.float64).reshape(x0.shape[0], 12).cuda()
    return A.affine_warp(x0, th, x1, out_size=out_size, mode=mode, fill=fill, **kw)


def _check(got, ref, what):
    got = got.detach().cpu().double().numpy().reshape(ref.shape)
    err = np.abs(got - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-11
    worst = float((err / bound).max())
    print(f"{what}: max |got - ref| = {err.max():.3e}, worst err / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, float(err.max()), worst)


# ---- against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(R.CASES))
def test_rotated_cases_against_fp64(case, mode):
    n, in_size, out_size, theta = R.CASES[case]
    two_d = in_size[0] == 1
    x0, x1 = (_dev(a, two_d) for a in _pair(n, in_size))
    out = out_size[1:] if two_d else out_size
    y0, y1 = _warp(x0, x1, theta, out, mode)
    assert y0.shape == (n, 1, *out) and y1.shape == y0.shape
    _check(y0, _reference(case, mode, 0), f"{case} {mode} plane 0")
    _check(y1, _reference(case, mode, 1), f"{case} {mode} plane 1")
    # one plane and two planes give the same bits; so do two runs
    assert torch.equal(_bits(_warp(x0, None, theta, out, mode)), _bits(y0))
    assert torch.equal(_bits(_warp(x1, None, theta, out, mode)), _bits(y1))
    again = _warp(x0, x1, theta, out, mode)
    assert torch.equal(_bits(again[0]), _bits(y0)) and torch.equal(_bits(again[1]), _bits(y1))
    # a fill per plane
    z0, z1 = _warp(x0, x1, theta, out, mode, fill=(FILL, 0.5))
    assert torch.equal(_bits(z0), _bits(y0))
    if mode == R.CONSTANT and case != "crop":
        _check(z1, R.affine_warp_ref(_pair(n, in_size)[1], theta, out_size, mode, 0.5), f"{case} fill 0.5")
    else:
        assert torch.equal(_bits(z1), _bits(y1))


@pytest.mark.parametrize("mode", MODES)
def test_downsampling_by_two_is_the_block_mean(mode):
    in_size, out_size = (8, 12, 16), (4, 6, 8)
    x = _pair(2, in_size)[0]
    theta = np.tile(np.concatenate([2.0 * np.eye(3), np.full((3, 1), 0.5)], 1).reshape(1, 12), (2, 1))
    y = _warp(_dev(x), None, theta, out_size, mode)
    want = x.astype(np.float64).reshape(2, 4, 2, 6, 2, 8, 2).mean(axis=(2, 4, 6))
    _check(y, want, f"2x downsample {mode}")


# ---- bit for bit against torch index ops --------------------------------------------------------------------------------
def _theta_rows(A, t, n):
    row = np.concatenate([np.asarray(A, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3, 1)], 1)
    return np.tile(row.reshape(1, 12), (n, 1))


@pytest.mark.parametrize("mode", MODES)
def test_identity_and_flips_copy_bits(mode):
    size = (5, 9, 35)                                   # more than one tile along d, h and w; W % 4 != 0
    x0, x1 = (_dev(a) for a in _pair(2, size))
    for axes in [(), (0,), (1,), (2,), (0, 1, 2)]:
        f = [-1.0 if k in axes else 1.0 for k in range(3)]
        theta = _theta_rows(np.diag(f), [size[k] - 1.0 if k in axes else 0.0 for k in range(3)], 2)
        y0, y1 = _warp(x0, x1, theta, mode=mode)
        dims = [k + 2 for k in axes]
        assert torch.equal(_bits(y0), _bits(torch.flip(x0, dims) if dims else x0)), axes
        assert torch.equal(_bits(y1), _bits(torch.flip(x1, dims) if dims else x1)), axes
    # 2-D
    a0, a1 = (_dev(a, two_d=True) for a in _pair(3, (1, 13, 10)))
    theta = _theta_rows(np.diag([1.0, -1.0, -1.0]), [0.0, 12.0, 9.0], 3)
    y0, y1 = _warp(a0, a1, theta, mode=mode)
    assert torch.equal(_bits(y0), _bits(torch.flip(a0, [2, 3]))) and torch.equal(_bits(y1), _bits(torch.flip(a1, [2, 3])))


@pytest.mark.parametrize("mode", MODES)
def test_quarter_turns_of_a_cube_copy_bits(mode):
    x = _dev(_pair(1, (9, 9, 9))[0])
    idx = torch.arange(9)
    for (i, j), k in itertools.product([(0, 1), (0, 2), (1, 2)], range(4)):
        # y[p] = x[A p + t], A the k-fold quarter turn in the (i, j) plane about the centre 4
        c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][k]
        A = np.eye(3)
        A[i, i], A[i, j], A[j, i], A[j, j] = c, -s, s, c
        t = 4.0 - A @ np.full(3, 4.0)
        y = _warp(x, None, _theta_rows(A, t, 1), mode=mode)
        src = [None, None, None]                        # the source index of every axis, as integer index arithmetic
        grid = torch.meshgrid(idx, idx, idx, indexing="ij")
        for r in range(3):
            src[r] = sum(int(A[r, q]) * grid[q] for q in range(3)) + int(t[r])
        want = x[0, 0].cpu()[src[0], src[1], src[2]]
        assert torch.equal(_bits(y[0, 0]), _bits(want)), ((i, j), k)
        assert torch.equal(_bits(y), _bits(torch.rot90(x, -k, dims=(i + 2, j + 2)))), ((i, j), k)


@pytest.mark.parametrize("mode", MODES)
def test_an_integer_shift_fills_or_replicates(mode):
    size, shift = (6, 7, 9), (2, -1, 3)
    x0, x1 = (_dev(a) for a in _pair(2, size))
    y0, y1 = _warp(x0, x1, _theta_rows(np.eye(3), shift, 2), mode=mode, fill=(FILL, 0.25))
    for x, y, fill in ((x0, y0, FILL), (x1, y1, 0.25)):
        idx = [torch.arange(size[k]) + shift[k] for k in range(3)]
        inside = [(i >= 0) & (i < size[k]) for k, i in enumerate(idx)]
        idx = [i.clamp(0, size[k] - 1).cuda() for k, i in enumerate(idx)]
        moved = x[:, :, idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]
        if mode == R.CONSTANT:
            keep = (inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]).cuda()
            moved = torch.where(keep, moved, torch.full_like(moved, fill))
        assert torch.equal(_bits(y), _bits(moved))
    # far outside, and a map that is not a number: `fill` / the clamped edge
    for t in ((1e12, 0, 0), (0, -1e300, 0), (0, 0, float("nan"))):
        y = _warp(x0, None, _theta_rows(np.eye(3), t, 2), mode=mode)
        if mode == R.CONSTANT:
            assert bool((y == FILL).all()), t
        else:
            assert bool(torch.isfinite(y).all()) and float(y.abs().max()) <= 1.0, t


# ---- noise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_noise_is_added_in_fp64_and_zero_sigma_changes_nothing(mode):
    n, in_size, out_size, theta = R.CASES["rot3d"]
    x0, x1 = (_dev(a) for a in _pair(n, in_size))
    sigma = torch.tensor([[0.0, 0.07], [0.05, 0.0]], dtype=torch.float32)
    g = torch.Generator().manual_seed(7)
    noise = [torch.randn(n, 1, *out_size, generator=g) for _ in range(2)]
    plain = _warp(x0, x1, theta, out_size, mode)
    y = _warp(x0, x1, theta, out_size, mode, noise=[t.cuda() for t in noise], sigma=sigma.cuda())
    for k in range(2):
        ref = _reference("rot3d", mode, k) + (sigma[:, k].double().view(n, 1, 1, 1) * noise[k][:, 0].double()).numpy()
        _check(y[k], ref, f"noise {mode} plane {k}")
        for s in range(n):
            same = torch.equal(_bits(y[k][s]), _bits(plain[k][s]))
            assert same == (float(sigma[s, k]) == 0.0), (k, s)
    # a field on one plane alone; a missing pointer is the call without noise on that plane
    only0 = _warp(x0, x1, theta, out_size, mode, noise=noise[0].cuda(), sigma=sigma.cuda())
    assert torch.equal(_bits(only0[0]), _bits(y[0])) and torch.equal(_bits(only0[1]), _bits(plain[1]))
    only1 = _warp(x0, x1, theta, out_size, mode, noise=(None, noise[1].cuda()), sigma=sigma.cuda())
    assert torch.equal(_bits(only1[0]), _bits(plain[0])) and torch.equal(_bits(only1[1]), _bits(y[1]))
    one = _warp(x0, None, theta, out_size, mode, noise=noise[0].cuda(), sigma=sigma.cuda())
    assert torch.equal(_bits(one), _bits(y[0]))


# ---- launch paths ---------------------------------------------------------------------------------------------------------
def _offset_view(t):
    """A contiguous copy of t that starts 4 bytes into its allocation."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("mode", MODES)
def test_unaligned_views_give_the_same_bits(mode):
    from mpgan_amd import ops
    n, in_size, out_size, theta = R.CASES["rot3d"]      # W = 11: W % 4 != 0
    x0, x1 = (_dev(a) for a in _pair(n, in_size))
    th = torch.from_numpy(theta).cuda()
    sigma = torch.tensor([[0.1, 0.2], [0.3, 0.0]], dtype=torch.float32).cuda()
    noise = torch.randn(2, n, 1, *out_size, generator=torch.Generator().manual_seed(8)).cuda()
    m = ops.WARP_BORDER if mode == R.BORDER else ops.WARP_CONSTANT
    y = ops.affine_warp(x0, x1, th, m, FILL, FILL, noise[0], noise[1], sigma, torch.empty_like(x0), torch.empty_like(x0))
    v = ops.affine_warp(_offset_view(x0), _offset_view(x1), th, m, FILL, FILL, _offset_view(noise[0]), _offset_view(noise[1]),
                        sigma, _offset_view(torch.empty_like(x0)), _offset_view(torch.empty_like(x0)))
    assert torch.equal(_bits(v[0]), _bits(y[0])) and torch.equal(_bits(v[1]), _bits(y[1]))


def test_many_tiles_per_sample():
    """The launch has no grid cap: 2 x 3 x 300 x 70 has 2 * 1 * 38 * 3 tiles of 4 x 8 x 32 and the image 600 x 200 has
    75 * 7 tiles of 1 x 8 x 32; against index arithmetic (a half-voxel shift along w: the lerp of two neighbours)."""
    for size in ((3, 300, 70), (600, 200)):
        n = 2 if len(size) == 3 else 1
        x = torch.rand(n, 1, *size, generator=torch.Generator().manual_seed(5)).cuda() * 2 - 1
        theta = _theta_rows(np.eye(3), (0.0, 0.0, 0.5), n)
        y = _warp(x, None, theta, mode=R.BORDER)
        right = torch.cat([x[..., 1:], x[..., -1:]], -1)
        want = (x.double() + 0.5 * (right.double() - x.double())).float()
        assert torch.equal(_bits(y), _bits(want))


# ---- the function and the module --------------------------------------------------------------------------------------------
def test_affine_warp_refuses_what_it_cannot_do():
    from mpgan_amd import augment as A
    x = torch.zeros(2, 1, 8, 8, device="cuda")
    th = torch.eye(3, 4, dtype=torch.float64, device="cuda").reshape(1, 12).repeat(2, 1)
    with pytest.raises(ValueError, match="differentiable"):
        A.affine_warp(x.clone().requires_grad_(True), th)
    with torch.no_grad():
        assert torch.equal(A.affine_warp(x.clone().requires_grad_(True), th), x)
    with pytest.raises(ValueError, match="mode"):
        A.affine_warp(x, th, mode="reflect")
    with pytest.raises(ValueError, match="theta"):
        A.affine_warp(x, th.float())
    with pytest.raises(ValueError, match="theta"):
        A.affine_warp(x, th[:1])
    with pytest.raises(ValueError, match="sigma"):
        A.affine_warp(x, th, noise=torch.zeros_like(x))
    with pytest.raises(ValueError, match="out_size"):
        A.affine_warp(x, th, out_size=(2, 8, 8))
    with pytest.raises(ValueError):
        A.affine_warp(x, th, torch.zeros(2, 1, 8, 9, device="cuda"))


def test_pair_augment_module_replays_from_its_draw():
    from mpgan_amd import augment as A
    g = torch.Generator().manual_seed(3)
    batch = {k: (torch.rand(3, 1, 6, 20, 12, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}
    batch["name"] = "kept"
    m = A.PairAugment(rotate=0.4, scale=0.2, shift=0.1, flip=(2,), prob=0.7, noise_std=0.1, mode="constant",
                      generator=torch.Generator(device="cuda").manual_seed(11))
    out = m(batch)
    assert out is not batch and out["name"] == "kept" and set(out) == set(batch)
    replay = torch.Generator(device="cuda").manual_seed(11)
    p = A.sample_affine_params(3, (6, 20, 12), generator=replay, device="cuda", noise_planes=[0], **m.options)
    field = torch.randn((1, 3, 1, 6, 20, 12), generator=replay, device="cuda")
    assert torch.equal(p.theta, m.last_params.theta) and torch.equal(p.sigma, m.last_params.sigma)
    assert torch.equal(field, m.last_noise)
    y1, y2 = A.affine_warp(batch["t1w"], p.theta, batch["t2w"], mode="constant", fill=-1.0, noise=field[0], sigma=p.sigma)
    assert torch.equal(_bits(out["t1w"]), _bits(y1)) and torch.equal(_bits(out["t2w"]), _bits(y2))
    assert not torch.equal(out["t1w"], batch["t1w"]) and not out["t1w"].requires_grad
    # t2w has no noise: it is the plain warp
    assert torch.equal(_bits(y2), _bits(A.affine_warp(batch["t2w"], p.theta, mode="constant", fill=-1.0)))
    # gated off and without noise: a bit copy in new tensors
    off = A.PairAugment(rotate=0.4, prob=0.0)(batch)
    assert torch.equal(_bits(off["t1w"]), _bits(batch["t1w"])) and off["t1w"].data_ptr() != batch["t1w"].data_ptr()
    assert torch.equal(_bits(off["t2w"]), _bits(batch["t2w"]))
