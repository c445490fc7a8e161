"""mpgan_amd.preprocess (percentiles, scale_intensity_range_percentiles, resample_to_identity_grid) on the MI355X at
small, edge-case inputs against the float64 references of metric_small_ref.py and oracle/: data that isolates each of
the radix select's three passes, the sign boundary of its key map, sizes around its 2048 x 256-thread cap and around
the scale kernel's 4096 x 256 one; flipped, rotated and reflected direction matrices, an input axis of size 1, the two
half-voxel border rules hit exactly, and an output above the resample kernel's 8192 x 256-thread cap.  Bounds are derived
in DESIGN.md section 8.2; test_metric_small_ref_host.py holds the input conditions.  Each test prints its figures
before it asserts (-s shows them)."""
import numpy as np
import pytest
import torch

import metric_small_ref as R
from mpgan_amd import preprocess

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()   # a writable, contiguous copy (the shared inputs are read-only)


# ---- percentiles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.percentile_datasets()))
def test_percentiles_are_exact_order_statistics(name):
    """Within one fp32 ulp of the float64 interpolation of the sorted data, and the order statistic itself, bit for
    bit, wherever no interpolation happens (q = 0, q = 100, the median of an odd count, equal neighbours)."""
    x = R.percentile_datasets()[name]
    xd = _dev(x)
    worst, exact = 0.0, 0
    for qs in R.PCT_QS:
        out = preprocess.percentiles(xd, qs)
        again = preprocess.percentiles(xd, qs)
        assert torch.equal(out.view(torch.int32), again.view(torch.int32)), (name, qs)
        got = out.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (len(qs),)
        for g, q in zip(got, qs):
            v, s_lo, s_hi, t = R.order_stat_percentile(x, q)
            if t == 0.0 or s_lo == s_hi:
                exact += 1
                if s_lo == 0.0:                                  # -0.0 and +0.0 sort either way
                    assert g == 0.0, (name, q, g)
                else:
                    assert g.view(np.uint32) == s_lo.view(np.uint32), (name, q, g, s_lo)
            else:
                w32 = np.float32(v)
                ulps = abs(float(g) - float(w32)) / float(R.f32_ulp(max(abs(v), float(np.finfo(np.float32).tiny))))
                worst = max(worst, ulps)
                assert ulps <= 1.0, (name, q, g, v)
                assert s_lo <= g <= s_hi, (name, q, g, s_lo, s_hi)
    print(f"percentiles {name} (n={x.size}): {exact} exact results, interpolated ones within {worst:.2f} ulp")


def test_percentiles_take_non_contiguous_and_reject_empty():
    x = R.percentile_datasets()["n257"][:16 * 16].reshape(16, 16)
    view = _dev(x.T).t()
    assert not view.is_contiguous()
    for qs in R.PCT_QS:
        assert torch.equal(preprocess.percentiles(view, qs), preprocess.percentiles(_dev(x), qs))
    with pytest.raises(RuntimeError, match="bad argument"):
        preprocess.percentiles(torch.empty(0, device="cuda"), (50.0,))


# ---- scale intensity range --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("n", R.SCALE_SIZES)
def test_scale_intensity_range_on_both_sides_of_the_grid_cap(n, clip):
    """The scaling kernel alone: the reference takes a_min / a_max from the device's own fp32 percentiles; four fp32
    roundings (subtract, span, divide, multiply-add) of a value of magnitude (b_max - b_min) max(1, |v|)."""
    from oracle.metrics_ref import scale_intensity_range_percentiles
    x = R.scale_input(n)
    xd = _dev(x)
    for lower, upper, b_min, b_max in ((1.0, 99.0, -1.0, 1.0), (5.0, 95.0, 0.0, 255.0)):
        mm = preprocess.percentiles(xd, (lower, upper)).cpu().numpy().astype(np.float64)
        for q, m in zip((lower, upper), mm):
            assert abs(m - R.order_stat_percentile(x, q)[0]) <= float(R.f32_ulp(m)), (q, m)
        want = scale_intensity_range_percentiles(x.astype(np.float64), lower, upper, b_min, b_max, clip, a_min=mm[0],
                                                 a_max=mm[1])
        got = preprocess.scale_intensity_range_percentiles(xd, lower, upper, b_min, b_max, clip).cpu().numpy()
        lim = (b_max - b_min) * 4 * R.U32 * np.maximum(1.0, np.abs(want))
        ratio = float((np.abs(got.astype(np.float64) - want) / lim).max())
        print(f"scale range n={n} clip={clip} [{b_min}, {b_max}]: worst err / limit {ratio:.3f}, max |v| {np.abs(want).max():.2f}")
        assert got.shape == (n,) and ratio <= 1.0, ratio
        if clip:
            assert got.min() == b_min and got.max() == b_max
        else:
            assert got.max() > b_max


@pytest.mark.parametrize("fill", [0.0, 3.5])
def test_scale_intensity_range_degenerate_returns_x_minus_a_min(fill):
    """p1 == p99: MONAI returns x - a_min, neither scaled nor clipped."""
    x = R.degenerate_scale_input(fill)
    xd = _dev(x)
    mm = preprocess.percentiles(xd, (1.0, 99.0)).cpu().numpy()
    assert mm[0] == fill and mm[1] == fill
    for clip in (True, False):
        got = preprocess.scale_intensity_range_percentiles(xd, clip=clip).cpu().numpy()
        want = x - np.float32(fill)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert got.max() > 1.0


# ---- resample ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.RESAMPLE_GEOMS))
def test_resample_geometries(name):
    """With every continuous index at least 1e-6 from a border (the host test asserts it) the inside / outside
    decisions of the kernel and the float64 restatement agree, and the interpolated values, both formed in double and
    rounded once, differ by at most one fp32 ulp.  Outside is exactly 0; the input is >= 1 everywhere."""
    from oracle.resample_ref import resample_to_identity_grid
    g = R.RESAMPLE_GEOMS[name]
    vol = R.resample_volume(name)
    ref = resample_to_identity_grid(vol, g["origin"], g["spacing"], g["direction"], g["out_size"])
    got = preprocess.resample_to_identity_grid(_dev(vol), g["origin"], g["spacing"], g["direction"].tolist(),
                                               g["out_size"]).cpu().numpy()
    assert got.shape == tuple(reversed(g["out_size"])) and got.dtype == np.float32
    outside = ref == 0
    ulps = np.abs(got.astype(np.float64) - ref.astype(np.float64))[~outside] / R.f32_ulp(ref[~outside])
    print(f"resample {name}: inside share {1 - outside.mean():.3f}, worst {ulps.max():.2f} ulp, "
          f"{int((got[outside] != 0).sum())} outside voxels non-zero")
    assert not got[outside].any()
    assert (got[~outside] != 0).all()
    assert ulps.max() <= 1.0


def test_resample_half_voxel_borders_exactly():
    """c = 2 i - 0.5 on every axis: i = 0 sits on the inclusive border -0.5 and takes the base sample alone, i = 1..3
    are midpoints, i = 4 sits on the exclusive border 7.5 and is outside.  64 voxels inside, bit for bit."""
    from oracle.resample_ref import resample_to_identity_grid
    g = R.BORDER_CASE
    vol = (1.0 + 99.0 * np.random.RandomState(8).rand(*g["in_dhw"])).astype(np.float32)
    ref = resample_to_identity_grid(vol, g["origin"], g["spacing"], g["direction"], g["out_size"])
    got = preprocess.resample_to_identity_grid(_dev(vol), g["origin"], g["spacing"], g["direction"].tolist(),
                                               g["out_size"]).cpu().numpy()
    assert int((got != 0).sum()) == 64 and (got[:4, :4, :4] != 0).all()
    assert not got[4:].any() and not got[:, 4:].any() and not got[:, :, 4:].any()
    assert got[0, 0, 0] == vol[0, 0, 0]
    f = vol.astype(np.float64)
    lerp = lambda lo, hi: lo + 0.5 * (hi - lo)
    # i = 0 along one axis (the base sample of that axis alone), the first midpoint (1.5) along the other two
    assert got[0, 1, 1] == np.float32(lerp(lerp(f[0, 1, 1], f[0, 1, 2]), lerp(f[0, 2, 1], f[0, 2, 2])))
    assert got[1, 0, 1] == np.float32(lerp(lerp(f[1, 0, 1], f[1, 0, 2]), lerp(f[2, 0, 1], f[2, 0, 2])))
    assert got[1, 1, 0] == np.float32(lerp(lerp(f[1, 1, 0], f[1, 2, 0]), lerp(f[2, 1, 0], f[2, 2, 0])))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_resample_takes_non_contiguous_input():
    g = R.RESAMPLE_GEOMS["rotation"]
    vol = R.resample_volume("rotation")
    view = _dev(vol.transpose(2, 1, 0)).permute(2, 1, 0)
    assert not view.is_contiguous()
    args = (g["origin"], g["spacing"], g["direction"].tolist(), g["out_size"])
    assert torch.equal(preprocess.resample_to_identity_grid(view, *args),
                       preprocess.resample_to_identity_grid(_dev(vol), *args))
