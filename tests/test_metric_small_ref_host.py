"""CPU checks of tests/metric_small_ref.py: the references against numpy and the oracle, and the conditions the shared
inputs must meet so that the bounds of test_metrics_small_gpu.py / test_preprocess_small_gpu.py cannot hide a failure
(near-tie share of every rescale input, margin and inside share of every resample geometry, exact-integer ranges of
the error inputs).  Change an input so that a cap no longer holds and this file fails."""
import math

import numpy as np
import pytest

import metric_small_ref as R


# ---- order_stat_percentile -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1000, 100003, 524289])
def test_order_stat_percentile_is_np_percentile(n):
    x = (np.random.RandomState(n % 9973).rand(n) * 2000 - 1000).astype(np.float32)
    for qs in R.PCT_QS + ((33.3, 66.6), (99.999,)):
        for q in qs:
            v, a, b, t = R.order_stat_percentile(x, q)
            want = np.percentile(x.astype(np.float64), q)
            assert np.float32(v) == np.float32(want), (n, q, v, want)            # 0 fp32 ulp
            assert a <= np.float32(v) <= b and 0.0 <= t < 1.0


def test_order_stat_percentile_interpolates_by_hand():
    x = np.array([4.0, 1.0, 2.0, 8.0], dtype=np.float32)
    assert R.order_stat_percentile(x, 50.0) == (3.0, 2.0, 4.0, 0.5)
    assert R.order_stat_percentile(x, 0.0)[0] == 1.0 and R.order_stat_percentile(x, 100.0)[0] == 8.0
    v, a, b, t = R.order_stat_percentile(x, 25.0)                                # r = 0.75
    assert (a, b) == (1.0, 2.0) and v == 1.75 and t == 0.75
    inf = np.array([-np.inf, -np.inf, 0.0, np.inf], dtype=np.float32)
    assert R.order_stat_percentile(inf, 0.0)[0] == -np.inf and R.order_stat_percentile(inf, 100.0)[0] == np.inf


def test_percentile_datasets_meet_their_descriptions():
    d = R.percentile_datasets()

    def key(x):                                     # the kernel's monotone uint32 image of a float
        u = x.view(np.uint32)
        return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)

    for sign in ("pos", "neg"):
        for name in ("low10_" + sign, "low10_all_" + sign):
            k = key(d[name])
            assert np.unique(k >> 10).size == 1 and np.unique(k & 1023).size > 500, name
        assert np.unique(key(d["low10_all_" + sign]) & 1023).size == 1024
        k = key(d["mid11_" + sign])
        assert np.unique(k >> 21).size == 1 and np.unique((k >> 10) & 2047).size > 1000 and np.unique(k & 1023).size == 1
        k = key(d["mid11_low10_" + sign])
        assert np.unique(k >> 21).size == 1 and np.unique(k & 1023).size > 500
    for name in ("signs_small", "signs_inf"):
        x = d[name]
        assert (x < 0).any() and (x > 0).any() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
        assert (np.abs(x[x != 0]) < np.finfo(np.float32).tiny).sum() >= 2        # subnormals of both signs
        assert np.finfo(np.float32).max in x and -np.finfo(np.float32).max in x
    assert np.isinf(d["signs_inf"]).sum() == 6 and not np.isinf(d["signs_small"]).any()
    assert np.unique(d["all_equal"]).size == 1
    assert sorted(np.unique(d["one_low"], return_counts=True)[1]) == [1, 999]
    assert sorted(np.unique(d["one_high"], return_counts=True)[1]) == [1, 999]
    assert (np.diff(d["ramp_up"]) > 0).all() and (np.diff(d["ramp_down"]) < 0).all()
    assert {d[f"n{n}"].size for n in R.PCT_SIZES} == set(R.PCT_SIZES) and 2048 * 256 in R.PCT_SIZES
    # no case interpolates between an infinity and another value (NaN by numpy's rule as well: out of scope)
    for name, x in d.items():
        assert not np.isnan(x).any()
        for qs in R.PCT_QS:
            for q in qs:
                v, a, b, t = R.order_stat_percentile(x, q)
                assert not math.isnan(v), (name, q)
                if not (np.isfinite(a) and np.isfinite(b)):
                    assert t == 0.0 or a == b, (name, q)


# ---- ssim_window ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 7), (7, 7, 7)])
@pytest.mark.parametrize("kind", R.SSIM_KINDS)
def test_ssim_window_matches_the_oracle_on_single_windows(shape, kind):
    from oracle.metrics_ref import structural_similarity
    a, b, dr = R.ssim_pair(shape, kind)
    assert abs(R.ssim_window(a, b, dr) - structural_similarity(a, b, data_range=dr)) <= 1e-12


def test_ssim_inputs_meet_their_descriptions():
    for shape in R.SSIM_SHAPES:
        a, b, dr = R.ssim_pair(shape, "pair")
        assert dr == 256.0 and (a == np.round(a)).all() and a.min() >= 0 and b.max() <= 255 and (a != b).any()
        a, b, _ = R.ssim_pair(shape, "equal_const")
        assert np.unique(a).size == 1 and (a == b).all()
        a, b, _ = R.ssim_pair(shape, "diff_const")
        assert np.unique(a).size == 1 and np.unique(b).size == 1 and a.flat[0] != b.flat[0]
        # closed form of two constant images: the variance factor is C2 / C2
        c1 = (0.01 * 256.0) ** 2
        want = (2 * 93.0 * 201.0 + c1) / (93.0 ** 2 + 201.0 ** 2 + c1)
        assert abs(R.ssim_want(a, b, 256.0) - want) <= 1e-12
        a, b, _ = R.ssim_pair(shape, "one_const")
        assert np.unique(a).size > 1 and np.unique(b).size == 1
        a, b, dr = R.ssim_pair(shape, "inverted")
        assert (a + b == 255).all() and R.ssim_want(a, b, dr) < 0
        a, b, dr = R.ssim_pair(shape, "unit_range")
        assert dr == 1.0 and a.min() >= 0 and a.max() <= 1 and b.min() >= 0 and b.max() <= 1
    # the tile of the kernel is 4 x 8 x 32 window corners: every edge is met exactly and one past
    ow = {s[-1] - 6 for s in R.SSIM_SHAPES}
    oh = {s[-2] - 6 for s in R.SSIM_SHAPES}
    od = {s[0] - 6 for s in R.SSIM_SHAPES_3D}
    assert {1, 32, 33} <= ow and {1, 8, 9} <= oh and {1, 4, 5} <= od


# ---- rescale inputs ---------------------------------------------------------------------------------------------------
def test_rescale_cases_cover_the_sizes_and_placements():
    assert {n for n, _ in R.RESCALE_CASES} == set(R.SIZES)
    assert set(R.SIZES) >= {1, 2, 255, 256, 257, R.T - 1, R.T, R.T + 1, 2 * R.T + 77, 3 * R.T - 1}
    for n in R.STRIDE_SIZES:
        p = R.rescale_placements(n)
        assert set(p) == {"ends", "ends_swapped", "interior", "last_block_min", "last_block_max"}
        assert p["ends"] == (0, n - 1) and p["ends_swapped"] == (n - 1, 0)
        for i in (p["last_block_min"][0], p["last_block_max"][1]):
            assert 0 <= i < n and (i // 256) % 1024 == 1023
        assert all(0 < i < n - 1 for i in p["interior"])


@pytest.mark.parametrize("n,placement", R.RESCALE_CASES)
def test_rescale_inputs_have_few_near_ties_and_unique_extremes(n, placement):
    x = R.rescale_input(n, placement)
    imin, imax = R.rescale_placements(n)[placement]
    assert x.size == n and int(np.argmin(x)) == imin and (x == x.min()).sum() == 1
    if n > 1:
        assert int(np.argmax(x)) == imax and (x == x.max()).sum() == 1
    ref = R.rescale_ref(x)
    share = R.near_tie_mask(ref).mean()
    assert share <= R.NEAR_TIE_CAP, (n, placement, share)
    assert ref.min() == 0.0 and (n == 1 or ref.max() == 255.0)


def test_rescale_ref_and_near_tie_rule_by_hand():
    assert R.RESCALE_TOL == 255 * 4 * 2.0 ** -24
    np.testing.assert_array_equal(R.rescale_ref(np.array([2.0, 4.0, 3.0], dtype=np.float32)), [0.0, 255.0, 127.5])
    np.testing.assert_array_equal(R.rescale_ref(np.full(5, 7.0, dtype=np.float32)), np.zeros(5))
    m = R.near_tie_mask(np.array([127.5, 127.5 + 5e-5, 127.5 - 7e-5, 3.0, 0.49995]))
    assert m.tolist() == [True, True, False, False, True]
    for n in R.SIZES[1:]:
        x = R.integer_image(n)
        assert x.min() == 0 and x.max() == 255 and (x == np.round(x)).all()
        assert not R.near_tie_mask(R.rescale_ref(x)).any()                       # integers: far from every tie


# ---- image-error inputs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_error_inputs_keep_the_partial_sums_exact(n):
    m = R.error_terms_per_thread(n)
    assert m == math.ceil(n / (256 * min(math.ceil(n / 256), 1024)))
    assert m * 256 * 4096 <= 2 ** 24                 # a block's fp32 sum of squares stays an exact integer
    a, b = R.errors_int_pair(n)
    assert (a == np.round(a)).all() and (b == np.round(b)).all()
    assert a.min() >= 0 and a.max() <= 255 and b.min() >= 0 and b.max() <= 255
    assert np.abs(a - b).max() <= 64 and (a != b).any()
    fa, fb = R.errors_float_pair(n)
    assert (fa != fb).any() and np.abs(fa).max() <= 1 and np.abs(fb).max() <= 1.25


def test_errors_ref_by_hand():
    assert R.error_terms_per_thread(3 * R.T - 1) == 3 and R.error_terms_per_thread(R.T) == 1
    assert R.error_rel_bound(R.T + 1) == 13 * 2.0 ** -24
    mae, mse, psnr = R.errors_ref(np.array([1.0, 2.0, 3.0, 4.0]), np.array([1.0, 0.0, 3.0, 8.0]), 256.0)
    assert (mae, mse) == (1.5, 5.0) and abs(psnr - 10 * math.log10(65536 / 5.0)) < 1e-12
    assert R.errors_ref(np.ones(3), np.ones(3), 1.0) == (0.0, 0.0, math.inf)
    assert R.f32_ulp(1.0) == 2.0 ** -23 and R.f32_ulp(-3.0) == 2.0 ** -22


# ---- scale-range inputs -----------------------------------------------------------------------------------------------
def test_scale_inputs_meet_their_descriptions():
    assert set(R.SCALE_SIZES) >= {1000, 4096 * 256 - 1, 4096 * 256, 4096 * 256 + 513}
    for fill in (0.0, 3.5):
        x = R.degenerate_scale_input(fill)
        assert (x == fill).mean() >= 0.99 and (x != fill).any()
        assert R.order_stat_percentile(x, 1.0)[0] == fill == R.order_stat_percentile(x, 99.0)[0]
    x = R.scale_input(1000)
    assert R.order_stat_percentile(x, 1.0)[0] < R.order_stat_percentile(x, 99.0)[0]


# ---- resample geometries ----------------------------------------------------------------------------------------------
def test_resample_geometries_cover_the_list():
    g = R.RESAMPLE_GEOMS
    assert np.array_equal(g["identity"]["direction"], np.eye(3))
    assert np.array_equal(g["flip_xy"]["direction"], np.diag([-1.0, -1.0, 1.0]))
    rot, ref = g["rotation"]["direction"], g["reflection"]["direction"]
    assert abs(np.linalg.det(rot) - 1) < 1e-12 and abs(np.linalg.det(ref) + 1) < 1e-12
    assert (np.abs(rot) > 0.01).all()                                            # no axis left alone
    np.testing.assert_allclose(rot @ rot.T, np.eye(3), atol=1e-12)
    assert [g[k]["in_dhw"].index(1) for k in ("size1_z", "size1_y", "size1_x")] == [0, 1, 2]
    assert len(set(g["noncubic"]["out_size"])) == 3
    assert np.prod(g["stride"]["out_size"]) > 8192 * 256


@pytest.mark.parametrize("name", list(R.RESAMPLE_GEOMS))
def test_resample_geometry_margin_and_inside_share(name):
    from oracle.resample_ref import resample_to_identity_grid
    g = R.RESAMPLE_GEOMS[name]
    c, share, margin = R.resample_geometry_info(g["in_dhw"], g["origin"], g["spacing"], g["direction"], g["out_size"])
    assert margin >= R.RESAMPLE_MARGIN, (name, margin)
    if name != "stride":
        assert R.RESAMPLE_SHARE[0] <= share <= R.RESAMPLE_SHARE[1], (name, share)
    else:
        assert 0.05 <= share <= 0.95, (name, share)
    if name != "stride":                             # the helper's inside test is the oracle's
        ref = resample_to_identity_grid(R.resample_volume(name), g["origin"], g["spacing"], g["direction"], g["out_size"])
        assert ref.shape == tuple(reversed(g["out_size"]))
        assert abs((ref != 0).mean() - share) < 1e-12
        assert R.resample_volume(name).min() >= 1.0


def test_resample_border_case_is_exact():
    g = R.BORDER_CASE
    c, share, margin = R.resample_geometry_info(g["in_dhw"], g["origin"], g["spacing"], g["direction"], g["out_size"])
    want = 2.0 * np.arange(32) - 0.5
    for d in range(3):
        assert np.array_equal(np.moveaxis(c[..., d], d, 0)[:, 0, 0], want)
    assert margin == 0.0 and share == (4 / 32) ** 3
