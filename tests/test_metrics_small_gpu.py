"""mpgan_amd.metrics (rescale_0_255, image_errors, ssim) on the MI355X at small, edge-case shapes against the float64
references of metric_small_ref.py: sizes on both sides of the 1024 x 256-thread grid cap (the grid-stride loops), the
SSIM tile edges (4 x 8 x 32 window corners), degenerate inputs and the API-level behaviours.  Every bound is derived from
the kernels' arithmetic; test_metric_small_ref_host.py holds the input conditions they need.
Each test prints its figures before it asserts (-s shows them)."""
import math

import numpy as np
import pytest
import torch

import metric_small_ref as R
from mpgan_amd import metrics

pytestmark = pytest.mark.gpu

PSNR_K = 10.0 / math.log(10.0)


def _dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()   # a writable, contiguous copy (the shared inputs are read-only)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- rescale ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,placement", R.RESCALE_CASES)
def test_rescale_matches_float64_on_both_sides_of_the_grid_cap(n, placement):
    """Unrounded: four fp32 roundings of a value <= 255.  Rounded: rint of the float64 value, except that a value
    within that distance of a half-integer may land on either neighbour.  The only minimum and maximum sit in the
    element named by the placement, so a block or tail that the reduction misses changes every output."""
    x = R.rescale_input(n, placement)
    ref = R.rescale_ref(x)
    xd = _dev(x)
    got_u = metrics.rescale_0_255(xd, do_round=False).cpu().numpy().astype(np.float64)
    got_r = metrics.rescale_0_255(xd).cpu().numpy().astype(np.float64)
    err = float(np.abs(got_u - ref).max())
    want = np.rint(ref)
    off = got_r != want
    tie = R.near_tie_mask(ref)
    print(f"rescale n={n} {placement}: unrounded max err {err:.3e} (limit {R.RESCALE_TOL:.3e}); rounded: {int(off.sum())} "
          f"of {int(tie.sum())} near-ties on the other neighbour")
    assert got_u.shape == (n,) and err <= R.RESCALE_TOL, err
    imin, imax = R.rescale_placements(n)[placement]
    assert got_u[imin] == 0.0 and (n == 1 or got_u[imax] == 255.0)
    assert not (off & ~tie).any(), int((off & ~tie).sum())
    assert (np.abs(got_r - want)[off] == 1.0).all()


@pytest.mark.parametrize("n", R.SIZES[1:])
def test_rescale_exact_cases(n):
    x = R.integer_image(n)
    xd = _dev(x)
    y = metrics.rescale_0_255(xd)
    assert _same_bits(y, xd)                                   # integers 0..255 with both ends present: unchanged
    assert _same_bits(metrics.rescale_0_255(y), y)             # idempotent
    f = _dev(R.rescale_input(n, "ends"))
    y = metrics.rescale_0_255(f)
    assert _same_bits(metrics.rescale_0_255(y), y)
    const = torch.full((n,), 37.25, device="cuda")
    for do_round in (True, False):
        out = metrics.rescale_0_255(const, do_round=do_round)
        assert _same_bits(out, torch.zeros(n, device="cuda"))  # span == 0
    # a contiguous view at an odd storage offset against the same data at offset 0
    view = f.flatten()[1:]
    assert view.is_contiguous() and view.storage_offset() == 1
    for do_round in (True, False):
        assert _same_bits(metrics.rescale_0_255(view, do_round=do_round),
                          metrics.rescale_0_255(view.clone(), do_round=do_round))


def test_rescale_takes_non_contiguous_and_any_shape():
    x = R.rescale_input(R.T + 1, "interior")[:40 * 48 * 44].reshape(40, 48, 44)
    base = _dev(x.transpose(2, 0, 1))                          # contiguous (44, 40, 48)
    view = base.permute(1, 2, 0)                               # == x, not contiguous
    assert not view.is_contiguous() and tuple(view.shape) == x.shape
    assert _same_bits(metrics.rescale_0_255(view), metrics.rescale_0_255(_dev(x)))


# ---- image errors -----------------------------------------------------------------------------------------------------
def _check_psnr(got, ref, rel, where):
    lim = PSNR_K * rel + float(R.f32_ulp(ref))
    print(f"{where}: psnr err {abs(got - ref):.3e} (limit {lim:.3e})")
    assert abs(got - ref) <= lim, (where, got, ref)


@pytest.mark.parametrize("data_range", [256.0, 1.0])
@pytest.mark.parametrize("n", R.SIZES)
def test_image_errors_float_inputs(n, data_range):
    """MAE and MSE within (m + 11) 2^-24 relative of float64, m the terms one thread adds; PSNR by the same bound."""
    a, b = R.errors_float_pair(n)
    mae, mse, psnr = R.errors_ref(a, b, data_range)
    got = metrics.image_errors(_dev(a), _dev(b), data_range)
    g = {k: float(v.item()) for k, v in got.items()}
    rel = R.error_rel_bound(n)
    e1, e2 = abs(g["mae"] - mae) / mae, abs(g["mse"] - mse) / mse
    print(f"errors float n={n} m={R.error_terms_per_thread(n)}: rel err mae {e1:.3e} mse {e2:.3e} (limit {rel:.3e})")
    assert e1 <= rel and e2 <= rel, (g, mae, mse)
    _check_psnr(g["psnr"], psnr, rel, f"errors float n={n} range={data_range}")


@pytest.mark.parametrize("data_range", [256.0, 1.0])
@pytest.mark.parametrize("n", R.SIZES)
def test_image_errors_integer_inputs_are_exact_sums(n, data_range):
    """Integer images with |a - b| <= 64: every fp32 partial sum is an exact integer, so MAE and MSE are the fp32
    roundings of the float64 figures to within one ulp."""
    a, b = R.errors_int_pair(n)
    mae, mse, psnr = R.errors_ref(a, b, data_range)
    got = metrics.image_errors(_dev(a), _dev(b), data_range)
    g = {k: float(v.item()) for k, v in got.items()}
    for k, want in (("mae", mae), ("mse", mse)):
        w32 = float(np.float32(want))
        ulps = abs(g[k] - w32) / float(R.f32_ulp(want))
        print(f"errors int n={n}: {k} {ulps:.2f} ulp from float32(ref)")
        assert ulps <= 1.0, (k, g[k], want)
    _check_psnr(g["psnr"], psnr, 2.0 ** -23, f"errors int n={n} range={data_range}")


@pytest.mark.parametrize("n", [1, 257, R.T + 1, 3 * R.T - 1])
def test_image_errors_of_identical_images(n):
    a = _dev(R.errors_float_pair(n)[0])
    for data_range in (256.0, 1.0):
        got = metrics.image_errors(a, a.clone(), data_range)
        assert float(got["mae"]) == 0.0 and float(got["mse"]) == 0.0
        assert float(got["psnr"]) == math.inf


def test_image_errors_non_contiguous_offset_and_empty():
    a, b = R.errors_float_pair(R.T + 1)
    a2, b2 = a[:300 * 211].reshape(300, 211), b[:300 * 211].reshape(300, 211)
    view = _dev(a2.T).t()                                      # == a2, not contiguous
    assert not view.is_contiguous()
    want = metrics.image_errors(_dev(a2), _dev(b2))
    got = metrics.image_errors(view, _dev(b2))
    for k in ("mae", "mse", "psnr"):
        assert _same_bits(got[k], want[k]), k
    ad, bd = _dev(a), _dev(b)
    got = metrics.image_errors(ad[1:], bd[1:])                 # odd storage offset
    want = metrics.image_errors(ad[1:].clone(), bd[1:].clone())
    for k in ("mae", "mse", "psnr"):
        assert _same_bits(got[k], want[k]), k
    empty = torch.empty(0, device="cuda")
    with pytest.raises(RuntimeError, match="bad argument"):
        metrics.image_errors(empty, empty)
    with pytest.raises(RuntimeError, match="bad argument"):
        metrics.rescale_0_255(empty)
    with pytest.raises(ValueError):
        metrics.image_errors(ad, bd[1:])


# ---- SSIM -------------------------------------------------------------------------------------------------------------
def _ssim(a, b, data_range):
    return float(metrics.ssim(_dev(a), _dev(b), data_range).item())


@pytest.mark.parametrize("kind", R.SSIM_KINDS)
@pytest.mark.parametrize("shape", R.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_at_the_tile_edges(shape, kind):
    """The kernel sums in double and stores fp32: 2^-23 of the float64 reference (the closed form of one window for
    the single-window shapes, the oracle's restatement of skimage's algorithm elsewhere)."""
    a, b, data_range = R.ssim_pair(shape, kind)
    want = R.ssim_want(a, b, data_range)
    got = _ssim(a, b, data_range)
    print(f"ssim {shape} {kind}: got {got:.9f} want {want:.9f} err {abs(got - want):.3e} (limit {R.SSIM_TOL:.3e})")
    assert abs(got - want) <= R.SSIM_TOL, (got, want)
    if kind == "equal_const":
        assert got == 1.0
    if kind == "diff_const":
        c1 = (0.01 * data_range) ** 2
        closed = (2 * 93.0 * 201.0 + c1) / (93.0 ** 2 + 201.0 ** 2 + c1)
        assert abs(got - closed) <= R.SSIM_TOL
    if kind == "inverted":
        assert got < 0.0
    if kind == "pair":
        assert float(metrics.ssim(_dev(a), _dev(a), data_range).item()) == 1.0


@pytest.mark.parametrize("shape", R.SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_sees_every_voxel_of_the_last_partial_tile(shape):
    """One changed voxel in the last (partial) tile -- the last voxel of the image, which only the last window
    holds, and the first voxel of that window -- changes the result, which still matches the reference."""
    a, b, data_range = R.ssim_pair(shape, "pair")
    base = _ssim(a, b, data_range)
    last = tuple(s - 1 for s in shape)
    first_of_last_window = tuple(s - 7 for s in shape)
    for pos in (last, first_of_last_window):
        a2 = a.copy()
        a2[pos] = (a2[pos] + 128.0) % 256.0
        want = R.ssim_want(a2, b, data_range)
        got = _ssim(a2, b, data_range)
        print(f"ssim {shape} voxel {pos} changed: {base:.9f} -> {got:.9f}, err {abs(got - want):.3e}")
        assert got != base
        assert abs(got - want) <= R.SSIM_TOL, (pos, got, want)


@pytest.mark.parametrize("shape", [(15, 39), (11, 15, 39)])
def test_ssim_non_contiguous_equals_contiguous(shape):
    a, b, data_range = R.ssim_pair(shape, "pair")
    perm = tuple(reversed(range(len(shape))))
    view = _dev(a.transpose(perm)).permute(perm)               # == a, not contiguous
    assert not view.is_contiguous() and tuple(view.shape) == shape
    bd = _dev(b)
    assert _same_bits(metrics.ssim(view, bd, data_range), metrics.ssim(_dev(a), bd, data_range))
    pad = torch.cat([torch.zeros(1, device="cuda"), _dev(a).flatten()])
    off = pad[1:].view(shape)                                  # odd storage offset
    assert off.storage_offset() == 1
    assert _same_bits(metrics.ssim(off, bd, data_range), metrics.ssim(_dev(a), bd, data_range))


def test_score_volume_above_the_grid_cap_matches_float64():
    """score_volume on a volume above the 262,144-thread cap: the rescaled volumes by the near-tie rule, then MAE / MSE /
    PSNR of the device's own rescaled volumes by the image-error bound, and SSIM."""
    shape = (61, 67, 71)                                       # 290,177 voxels
    n = int(np.prod(shape))
    a, b = R.errors_float_pair(2 * R.T + 77)
    a, b = a[:n].reshape(shape), b[:n].reshape(shape)
    s = metrics.score_volume(_dev(a), _dev(b))
    ga = metrics.rescale_0_255(_dev(a)).cpu().numpy().astype(np.float64)
    gb = metrics.rescale_0_255(_dev(b)).cpu().numpy().astype(np.float64)
    for g, x in ((ga, a), (gb, b)):
        ref = R.rescale_ref(x)
        off = g != np.rint(ref)
        assert not (off & ~R.near_tie_mask(ref)).any() and (np.abs(g - np.rint(ref))[off] == 1).all()
    mae, mse, psnr = R.errors_ref(ga, gb, 256.0)
    rel = R.error_rel_bound(n)
    assert abs(float(s["mae"]) - mae) <= rel * mae and abs(float(s["mse"]) - mse) <= rel * mse
    _check_psnr(float(s["psnr"]), psnr, rel, "score_volume")
    from oracle.metrics_ref import structural_similarity
    want = structural_similarity(ga, gb, data_range=256.0)
    print(f"score_volume ssim err {abs(float(s['ssim']) - want):.3e}")
    assert abs(float(s["ssim"]) - want) <= R.SSIM_TOL
