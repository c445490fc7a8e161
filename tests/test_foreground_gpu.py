"""The foreground-mask kernels (csrc/foreground.hip) against the references of foreground_ref.py, at the small shapes
where they can go wrong: smaller than one group of four, item lengths that leave later items unaligned for 16-byte
access, several blocks per item, W = 1, and views one element into an allocation.

Tolerance of the masked L1 (derived, not measured): every term is exact in fp64; an fp64 sum of n terms errs by at most
n 2^-53 relative; the result is rounded to fp32 once.  So |loss - ref| <= 2^-23 |ref| + 1e-12, and every gradient element
gets the same bound against its reference value.  No element is exempted."""
import ctypes
import math

import numpy as np
import pytest
import torch

import foreground_ref as R
import metric_small_ref as MR
from mpgan_amd import _lib, losses, metrics, ops
from mpgan_amd import preprocess as P

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
REL = 2.0 ** -23
PSNR_K = 10.0 / math.log(10.0)


def _dev(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the shared inputs are read-only


def _offset(x):
    """The same values as a contiguous view one element into a fresh allocation: unaligned for 16-byte access."""
    t = _dev(x)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    buf[1:] = t.flatten()
    view = buf[1:].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- Otsu ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", R.BINS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_otsu_threshold_equals_the_reference_bit_for_bit(shape, bins):
    x, counts, want = R.otsu_case(shape, bins)
    for c in counts:                                     # a condition on the inputs, before the device is consulted
        assert R.sigma_gap(c, LO, HI) > R.SIGMA_GAP
    got = P.otsu_threshold(_dev(x), bins, (LO, HI))
    assert got.shape == shape[:2] and got.dtype == torch.float32 and got.is_cuda
    assert _same_bits(got.cpu().numpy().ravel(), want), (got, want)
    assert _same_bits(P.otsu_threshold(_offset(x), bins, (LO, HI)).cpu().numpy().ravel(), want)
    if shape[0] * shape[1] == 1:                         # unbatched: a 0-d tensor
        single = P.otsu_threshold(_dev(x[0, 0] if shape[2] > 1 else x[0, 0, 0]), bins, (LO, HI))
        assert single.dim() == 0 and _same_bits(single.cpu().numpy().reshape(1), want)


def test_otsu_includes_lo_and_hi_and_drops_the_rest():
    """Bins 0, 1, 2 and 3 of 4 hold 4, 4, 1 and 8 values, the 8 exactly at hi: without them the threshold differs."""
    inside = [LO] * 4 + [-0.25] * 4 + [0.25] + [HI] * 8
    x = np.array(inside + [1.5, -1.5, np.nan, np.inf, -np.inf, 1.0000001, -1.0000001], np.float32)
    counts = R.histogram(x, LO, HI, 4)
    assert counts.tolist() == [4, 4, 1, 8] and R.sigma_gap(counts, LO, HI) > R.SIGMA_GAP
    want = R.otsu_from_counts(counts, LO, HI)
    assert want != R.otsu_from_counts(np.array([4, 4, 1, 0]), LO, HI)
    assert want != R.otsu_from_counts(np.array([0, 4, 1, 8]), LO, HI)
    got = P.otsu_threshold(_dev(x.reshape(1, 1, 1, -1)), 4, (LO, HI))
    assert _same_bits(got.cpu().numpy().ravel(), np.array([want]))


def test_otsu_degenerate_items():
    n = 3 * 5 * 7
    x = np.empty((4, 1, 3, 5, 7), np.float32)
    x[0] = 5.0                                           # nothing inside the range
    x[1] = np.nan
    x[2] = 0.3                                           # one occupied bin
    x[3] = np.where(np.arange(n).reshape(3, 5, 7) % 2 == 0, 0.3, 7.0)     # one occupied bin and dropped values
    for bins in R.BINS:
        got = P.otsu_threshold(_dev(x), bins, (LO, HI)).cpu().numpy().ravel()
        want = np.array([R.otsu_threshold(x[i], LO, HI, bins) for i in range(4)], np.float32)
        assert np.isnan(want[:2]).all() and np.isnan(got[:2]).all()
        assert _same_bits(got[2:], want[2:]) and got[2] == got[3]


# ---- mask, box, count ---------------------------------------------------------------------------------------------------
def _all_outputs(x, thr, margin=(0, 0, 0)):
    items, spatial = x.shape[0] * x.shape[1], x.shape[2:]
    mask = torch.full(x.shape, 7, dtype=torch.uint8, device="cuda")
    box = torch.full((items, 2, 3), -5, dtype=torch.int32, device="cuda")
    count = torch.full((items,), -5, dtype=torch.int64, device="cuda")
    ops.foreground_mask(x, spatial, items, thr, margin, mask=mask, box=box, count=count)
    return mask, box, count


def _check_against_reference(x_np, thr_np, margin, x_dev=None):
    items = x_np.shape[0] * x_np.shape[1]
    vol = x_np.reshape((items,) + (1,) * (5 - x_np.ndim) + x_np.shape[2:])
    want_mask = R.foreground(vol, thr_np)
    want_box = np.stack([R.bounding_box(m, margin) for m in want_mask])
    want_count = want_mask.reshape(items, -1).sum(axis=1).astype(np.int64)
    x = _dev(x_np) if x_dev is None else x_dev
    thr = _dev(np.asarray(thr_np, np.float32))
    mask, box, count = _all_outputs(x, thr, margin)
    assert np.array_equal(mask.cpu().numpy().reshape(want_mask.shape), want_mask)
    assert np.array_equal(box.cpu().numpy(), want_box), (box, want_box)
    assert np.array_equal(count.cpu().numpy(), want_count)
    # each output asked for alone gives the same bits
    spatial = x.shape[2:]
    alone = torch.empty_like(mask)
    ops.foreground_mask(x, spatial, items, thr, margin, mask=alone)
    assert torch.equal(alone, mask)
    alone = torch.empty_like(box)
    ops.foreground_mask(x, spatial, items, thr, margin, box=alone)
    assert torch.equal(alone, box)
    alone = torch.empty_like(count)
    ops.foreground_mask(x, spatial, items, thr, margin, count=alone)
    assert torch.equal(alone, count)
    return want_mask, want_box, want_count


@pytest.mark.parametrize("shape", R.SHAPES)
def test_mask_box_and_count_equal_the_reference(shape):
    x, _, thr = R.otsu_case(shape, 256)
    for margin in ((0, 0, 0), (1, 2, 3), (100, 0, 1)):   # the last clips at both faces
        _, _, count = _check_against_reference(x, thr, margin)
        assert (count > 0).all() and (count < int(np.prod(shape[2:]))).all()
    _check_against_reference(x, thr, (1, 1, 1), x_dev=_offset(x))


def test_mask_public_functions_agree_with_the_kernel_outputs():
    shape = R.SHAPES[1]
    x, _, thr = R.otsu_case(shape, 256)
    xd = _dev(x)
    want = R.foreground(x.reshape((2,) + shape[2:]), thr).reshape(shape)
    mask = P.foreground_mask(xd)                         # "otsu" over (-1, 1) with 256 bins
    assert mask.dtype == torch.uint8 and mask.shape == xd.shape and np.array_equal(mask.cpu().numpy(), want)
    assert torch.equal(P.foreground_mask(xd, _dev(thr)), mask)
    assert torch.equal(P.foreground_mask(xd[0], float(thr[0])), mask[0])
    box = P.foreground_bbox(xd, margin=(1, 0, 2))
    assert box.shape == (2, 1, 2, 3) and box.dtype == torch.int32 and box.is_cuda
    for i in range(2):
        assert np.array_equal(box[i, 0].cpu().numpy(), R.bounding_box(want[i, 0], (1, 0, 2)))
    assert np.array_equal(P.foreground_count(xd).cpu().numpy().ravel(), want.reshape(2, -1).sum(axis=1))
    # 2-D: the box has two columns, an unbatched input no batch axes
    x2, _, thr2 = R.otsu_case(R.SHAPES[0], 256)
    box2 = P.foreground_bbox(_dev(x2[0, 0, 0]), margin=1)
    want2 = R.bounding_box(R.foreground(x2[0], thr2)[0], (0, 1, 1))[:, 1:]
    assert box2.shape == (2, 2) and np.array_equal(box2.cpu().numpy(), want2)
    # crop_foreground: the one host read; the crop is x inside the box of source
    crop, start, end = P.crop_foreground(xd[:1], margin=1)
    b = R.bounding_box(want[0, 0], (1, 1, 1))
    assert start == tuple(b[0]) and end == tuple(b[1])
    assert torch.equal(crop, xd[:1, :, b[0, 0]:b[1, 0], b[0, 1]:b[1, 1], b[0, 2]:b[1, 2]])
    other = _dev(np.arange(x[:1].size, dtype=np.float32).reshape(x[:1].shape))
    crop2, s2, e2 = P.crop_foreground(other, source=xd[:1], margin=1)
    assert (s2, e2) == (start, end) and crop2.shape == crop.shape and float(crop2.flatten()[0]) == float(
        other[0, 0, b[0, 0], b[0, 1], b[0, 2]])
    # a foreground_mask output goes into mutual_information as its explicit mask as it is
    y = _dev(np.clip(x + 0.05, -1, 1).astype(np.float32))
    mi = metrics.mutual_information(xd, y, bins=32, value_range=(LO, HI), mask=mask)
    inside = np.isfinite(x) & (x >= LO) & (x <= HI)
    assert int(mi["count"]) == int((want.astype(bool) & inside).sum())


def test_mask_edge_cases():
    shape = (1, 1, 4, 5, 6)
    # empty and full foreground, a NaN threshold, NaN values
    x = np.linspace(-1, 1, 120, dtype=np.float32).reshape(shape)
    for thr, kind in ((10.0, "empty"), (-10.0, "full"), (np.nan, "empty")):
        mask, box, count = _check_against_reference(x, [thr], (1, 1, 1))
        assert count[0] == (120 if kind == "full" else 0)
        assert box.tolist() == ([[[0, 0, 0], [4, 5, 6]]] if kind == "full" else [[[0, 0, 0], [0, 0, 0]]])
    xn = x.copy()
    xn[0, 0, 1] = np.nan
    _, _, count = _check_against_reference(xn, [-10.0], (0, 0, 0))
    assert count[0] == 90
    # a value equal to the threshold is background
    t = np.float32(x[0, 0, 2, 3, 4])
    mask, _, count = _check_against_reference(x, [t], (0, 0, 0))
    assert mask[0, 2, 3, 4] == 0 and count[0] == int((x > t).sum())
    # a single voxel at each of the eight corners, with a margin that clips at the faces it touches
    for corner in np.ndindex(2, 2, 2):
        z, y, w = (c * (e - 1) for c, e in zip(corner, shape[2:]))
        one = np.zeros(shape, np.float32)
        one[0, 0, z, y, w] = 1.0
        _, box, count = _check_against_reference(one, [0.5], (0, 0, 0))
        assert count[0] == 1 and box[0].tolist() == [[z, y, w], [z + 1, y + 1, w + 1]]
        _check_against_reference(one, [0.5], (2, 1, 3))
    # items with different thresholds, one of them empty
    two = np.stack([x[0], x[0]])
    _, box, count = _check_against_reference(two, [0.0, 5.0], (0, 0, 0))
    assert count.tolist() == [60, 0] and box[1].tolist() == [[0, 0, 0], [0, 0, 0]]


# ---- masked L1 ----------------------------------------------------------------------------------------------------------
def _within(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool((np.abs(got - ref) <= REL * np.abs(ref) + 1e-12).all())


def _run_l1(pred, target, reduction, weights, gout, **source):
    p, t = pred.clone().requires_grad_(True), target.clone().requires_grad_(True)
    loss = losses.masked_l1_loss(p, t, fg_weight=weights[0], bg_weight=weights[1], reduction=reduction, **source)
    loss.backward(gout)
    return loss.detach(), p.grad, t.grad


@pytest.mark.parametrize("reduction", R.REDUCTIONS)
@pytest.mark.parametrize("weights", R.WEIGHTS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_masked_l1_against_float64_and_between_its_two_mask_sources(shape, weights, reduction):
    pred, target, thr = R.l1_case(shape)
    mask = R.foreground(target.reshape((-1,) + shape[2:]), thr).reshape(shape)
    gout_np = np.linspace(0.5, 1.5, shape[0]) if reduction == "none" else np.float64(1.0)
    gout = torch.as_tensor(gout_np, dtype=torch.float32, device="cuda")
    gout_np = gout.cpu().numpy().astype(np.float64)
    want = R.masked_l1_numpy(pred, target, mask, *weights, reduction)
    want_grad = R.masked_l1_grad(pred, target, mask, *weights, reduction, gout_np)
    pd, td = _dev(pred), _dev(target)
    by_mask = _run_l1(pd, td, reduction, weights, gout, mask=_dev(mask))
    by_thr = _run_l1(pd, td, reduction, weights, gout, threshold=_dev(thr))
    for a, b in zip(by_mask, by_thr):                    # the two mask sources: the same bits
        assert _same_bits(_bits(a), _bits(b))
    loss, da, db = by_thr
    assert loss.shape == ((shape[0],) if reduction == "none" else ())
    print(f"masked l1 {shape} {weights} {reduction}: loss err {np.abs(loss.cpu().numpy() - want).max():.3e}, "
          f"grad err {np.abs(da.cpu().numpy() - want_grad).max():.3e}")
    assert _within(loss.cpu().numpy(), want), (loss, want)
    assert _within(da.cpu().numpy(), want_grad)
    assert _same_bits(_bits(db), _bits(-da))             # db == -da, bit for bit
    assert (da.cpu().numpy()[pred == target] == 0).all()
    again = _run_l1(pd, td, reduction, weights, gout, threshold=_dev(thr))
    for a, b in zip(by_thr, again):                      # two runs: the same bits
        assert _same_bits(_bits(a), _bits(b))
    # unaligned views of the same values: the same bits (a thread's values and their order do not depend on alignment)
    shifted = _run_l1(_offset(pred), _offset(target), reduction, weights, gout, mask=_offset(mask))
    for a, b in zip(by_thr, shifted):
        assert _same_bits(_bits(a), _bits(b))
    # "otsu" finds the same threshold on the device, a number serves every item, a bool mask is a uint8 one
    if reduction == "mean":
        for row in target.reshape(shape[0] * shape[1], -1):
            assert R.sigma_gap(R.histogram(row, LO, HI, 256), LO, HI) > R.SIGMA_GAP
        assert torch.equal(_run_l1(pd, td, reduction, weights, gout, threshold="otsu")[0], loss)
        assert torch.equal(_run_l1(pd, td, reduction, weights, gout, mask=_dev(mask.astype(bool)))[0], loss)
        if shape[0] * shape[1] == 1:
            assert torch.equal(_run_l1(pd, td, reduction, weights, gout, threshold=float(thr[0]))[0], loss)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_masked_l1_with_equal_weights_is_the_plain_l1(shape):
    """(w_fg, w_bg) = (1, 1) over items of one size: the mean over the items is mpgan_l1_loss's mean over all values.
    That kernel rounds a - b to fp32, adds m = ceil(n / (256 blocks)) terms per thread in fp32, folds them through six
    shuffle levels and three wave additions and stores fp32: (m + 11) 2^-24 relative (all terms non-negative), beside the
    masked loss's own 2^-23."""
    pred, target, thr = R.l1_case(shape)
    pd, td = _dev(pred), _dev(target)
    got = float(losses.masked_l1_loss(pd, td, threshold=_dev(thr), fg_weight=1.0, bg_weight=1.0))
    loss = torch.empty((), device="cuda")
    ops.l1_loss(pd, td, torch.empty(ops.l1_partials(), device="cuda"), loss)
    n = pred.size
    blocks = min(-(-n // 256), ops.l1_partials())
    m = -(-n // (256 * blocks))
    bound = (REL + (m + 11) * 2.0 ** -24) * abs(float(loss)) + 1e-12
    print(f"masked l1 (1, 1) {shape}: {got} against l1_loss {float(loss)}, limit {bound:.3e}")
    assert abs(got - float(loss)) <= bound


def test_masked_l1_item_without_weight_and_broadcast_mask():
    shape = (2, 2, 3, 17, 19)
    rng = np.random.RandomState(11)
    pred = rng.rand(*shape).astype(np.float32)
    target = rng.rand(*shape).astype(np.float32)
    mask = (rng.rand(2, 1, 3, 17, 19) < 0.4).astype(np.uint8)
    mask[1] = 0                                          # batch entry 1: no foreground in either channel
    full = np.broadcast_to(mask, shape)
    for reduction in R.REDUCTIONS:
        p = _dev(pred).requires_grad_(True)
        loss = losses.masked_l1_loss(p, _dev(target), _dev(mask), reduction=reduction)      # channel extent 1: broadcast
        loss.sum().backward()
        want = R.masked_l1_numpy(pred, target, full, 1.0, 0.0, reduction)
        assert _within(loss.detach().cpu().numpy(), want)
        grad = p.grad.cpu().numpy()
        assert (grad[1] == 0).all() and np.isfinite(grad).all() and (grad[0][full[0] != 0] != 0).any()
        assert _within(grad, R.masked_l1_grad(pred, target, full, 1.0, 0.0, reduction))
        if reduction == "none":
            assert float(loss.detach()[1]) == 0.0
    mod = losses.MaskedL1Loss(fg_weight=2.0, bg_weight=0.5)
    assert _within(float(mod(_dev(pred), _dev(target), _dev(full.copy()))),
                   R.masked_l1_numpy(pred, target, full, 2.0, 0.5, "mean"))
    fg = losses.ForegroundL1Loss(threshold=0.5)
    assert _within(float(fg(_dev(pred), _dev(target))), R.masked_l1_numpy(pred, target, target > 0.5, 1.0, 0.0, "mean"))


# ---- masked errors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES)
def test_masked_image_errors_against_float64(shape):
    pred, target, thr = R.l1_case(shape)
    a, b = (pred * 128 + 128).astype(np.float32), (target * 128 + 128).astype(np.float32)
    mask = R.foreground(target.reshape((-1,) + shape[2:]), thr).reshape(shape)
    for data_range in (256.0, 1.0):
        mae, mse, psnr, count = R.masked_errors(a, b, mask, data_range)
        for ad, bd, md in ((_dev(a), _dev(b), _dev(mask)), (_offset(a), _offset(b), _offset(mask.astype(bool)))):
            got = metrics.image_errors(ad, bd, data_range, mask=md)
            assert set(got) == {"mae", "mse", "psnr", "count"} and got["mae"].dtype == torch.float64
            g = {k: float(v) for k, v in got.items()}
            print(f"masked errors {shape}: mae {abs(g['mae'] - mae) / mae:.3e} mse {abs(g['mse'] - mse) / mse:.3e} "
                  f"psnr {abs(g['psnr'] - psnr):.3e}")
            assert abs(g["mae"] - mae) <= REL * mae and abs(g["mse"] - mse) <= REL * mse
            assert abs(g["psnr"] - psnr) <= 1e-5 and g["count"] == count


def test_masked_image_errors_edge_cases():
    pred, target, _ = R.l1_case(R.SHAPES[3])
    a, b = _dev(pred), _dev(target)
    none = metrics.image_errors(a, b, 2.0, mask=torch.zeros_like(a, dtype=torch.uint8))
    assert all(math.isnan(float(none[k])) for k in ("mae", "mse", "psnr")) and float(none["count"]) == 0.0
    same = metrics.image_errors(a, a.clone(), 2.0, mask=torch.ones_like(a, dtype=torch.bool))
    plain = metrics.image_errors(a, a.clone(), 2.0)
    assert float(same["mse"]) == 0.0 and float(same["psnr"]) == float(plain["psnr"]) == math.inf
    # a mask of all ones against the unmasked kernel, within that kernel's own fp32 bound (test_metrics_small_gpu.py)
    n = pred.size
    ones = metrics.image_errors(a, b, 2.0, mask=torch.ones_like(a, dtype=torch.uint8))
    plain = metrics.image_errors(a, b, 2.0)
    rel = MR.error_rel_bound(n)
    for k in ("mae", "mse"):
        assert abs(float(plain[k]) - float(ones[k])) <= rel * float(ones[k]), k
    assert abs(float(plain["psnr"]) - float(ones["psnr"])) <= PSNR_K * rel + float(MR.f32_ulp(float(ones["psnr"])))
    assert float(ones["count"]) == n
    # score_volume hands the mask to the errors alone
    vol, ref = a[0, 0], b[0, 0]
    m = P.foreground_mask(ref)
    scored, whole = metrics.score_volume(vol, ref, mask=m), metrics.score_volume(vol, ref)
    assert float(scored["count"]) == float(m.sum()) and torch.equal(scored["ssim"], whole["ssim"])
    direct = metrics.image_errors(metrics.rescale_0_255(vol), metrics.rescale_0_255(ref), 256.0, mask=m)
    assert float(scored["mae"]) == float(direct["mae"]) and "count" not in whole


# ---- C ABI: invalid arguments are refused before any launch -----------------------------------------------------------
def test_invalid_arguments_return_err_invalid():
    lib = _lib.lib()
    x = torch.zeros(64, device="cuda")
    ws = torch.zeros(1024, dtype=torch.float64, device="cuda")
    out = torch.zeros(16, dtype=torch.float64, device="cuda")
    m = torch.zeros(64, dtype=torch.uint8, device="cuda")
    px, pw, po, pm = x.data_ptr(), ws.data_ptr(), out.data_ptr(), m.data_ptr()
    dhw = (ctypes.c_int32 * 3)(1, 8, 8)

    def refused(rc, word):
        assert rc == -1 and word in lib.mpgan_last_error(), (rc, lib.mpgan_last_error())

    assert lib.mpgan_otsu_workspace(0, 64) == -1 and lib.mpgan_otsu_workspace(1, 1) == -1
    assert lib.mpgan_otsu_workspace(1, 257) == -1 and lib.mpgan_otsu_workspace(2, 256) == 2 * 256 * 8
    refused(lib.mpgan_otsu_threshold(None, 64, 1, -1.0, 1.0, 64, pw, px, None), b"otsu_threshold")
    refused(lib.mpgan_otsu_threshold(px, 64, 1, -1.0, 1.0, 64, None, px, None), b"otsu_threshold")
    refused(lib.mpgan_otsu_threshold(px, 64, 1, -1.0, 1.0, 64, pw, None, None), b"otsu_threshold")
    refused(lib.mpgan_otsu_threshold(px, 64, 1, -1.0, 1.0, 1, pw, px, None), b"bins")
    refused(lib.mpgan_otsu_threshold(px, 64, 1, -1.0, 1.0, 257, pw, px, None), b"bins")
    refused(lib.mpgan_otsu_threshold(px, 64, 0, -1.0, 1.0, 64, pw, px, None), b"items")
    refused(lib.mpgan_otsu_threshold(px, 0, 1, -1.0, 1.0, 64, pw, px, None), b"numel_per_item")
    refused(lib.mpgan_otsu_threshold(px, 64, 1, 1.0, 1.0, 64, pw, px, None), b"hi > lo")
    refused(lib.mpgan_otsu_threshold(px, 64, 1, -1.0, float("inf"), 64, pw, px, None), b"non-finite")

    refused(lib.mpgan_foreground_mask(None, dhw, 1, px, None, pm, None, None, None), b"foreground_mask")
    refused(lib.mpgan_foreground_mask(px, None, 1, px, None, pm, None, None, None), b"foreground_mask")
    refused(lib.mpgan_foreground_mask(px, dhw, 1, None, None, pm, None, None, None), b"foreground_mask")
    refused(lib.mpgan_foreground_mask(px, dhw, 1, px, None, None, None, None, None), b"no output")
    refused(lib.mpgan_foreground_mask(px, dhw, 0, px, None, pm, None, None, None), b"items")
    refused(lib.mpgan_foreground_mask(px, (ctypes.c_int32 * 3)(1, 0, 8), 1, px, None, pm, None, None, None), b"extents")
    refused(lib.mpgan_foreground_mask(px, dhw, 1, px, (ctypes.c_int32 * 3)(0, -1, 0), pm, None, None, None), b"margin")

    assert lib.mpgan_masked_l1_workspace(0, 1) == -1 and lib.mpgan_masked_l1_workspace(64, 0) == -1
    need = lib.mpgan_masked_l1_workspace(64, 1)
    assert 0 < need <= ws.numel() * 8

    def fwd(a=px, b=px, n=64, items=1, channels=1, mask=pm, thr=None, w_fg=1.0, w_bg=0.0, work=pw, nbytes=need, den=po,
            reduction=0, loss=px):
        return lib.mpgan_masked_l1_forward(a, b, n, items, channels, mask, thr, w_fg, w_bg, work, nbytes, den, reduction,
                                           loss, None)

    assert fwd() == 0
    refused(fwd(a=None), b"masked_l1_forward")
    refused(fwd(b=None), b"masked_l1_forward")
    refused(fwd(work=None), b"masked_l1_forward")
    refused(fwd(den=None), b"masked_l1_forward")
    refused(fwd(loss=None), b"masked_l1_forward")
    refused(fwd(mask=pm, thr=px), b"both")
    refused(fwd(mask=None, thr=None), b"neither")
    refused(fwd(items=0), b"items")
    refused(fwd(n=0), b"numel_per_item")
    refused(fwd(items=3, channels=2), b"channels")
    refused(fwd(w_fg=-1.0), b"weights")
    refused(fwd(w_bg=float("nan")), b"weights")
    refused(fwd(reduction=3), b"reduction")
    refused(fwd(nbytes=need - 8), b"workspace")

    def bwd(a=px, b=px, n=64, items=1, channels=1, mask=pm, thr=None, den=po, up=px, stride=0, scale=1.0, da=px, db=None):
        return lib.mpgan_masked_l1_backward(a, b, n, items, channels, mask, thr, 1.0, 0.0, den, up, stride, scale, da, db,
                                            None)

    g = torch.zeros(64, device="cuda")
    assert bwd(da=g.data_ptr()) == 0
    refused(bwd(a=None), b"masked_l1_backward")
    refused(bwd(den=None), b"masked_l1_backward")
    refused(bwd(up=None), b"masked_l1_backward")
    refused(bwd(da=None, db=None), b"no gradient")
    refused(bwd(mask=pm, thr=px), b"both")
    refused(bwd(mask=None, thr=None), b"neither")
    refused(bwd(items=0), b"items")
    refused(bwd(stride=2), b"upstream_stride")
    refused(bwd(scale=float("inf")), b"scale")

    assert lib.mpgan_masked_errors_partials(0) == -1 and lib.mpgan_masked_errors_partials(64) == 3
    for args in ((None, px, pm, 64, 1.0, pw, po), (px, None, pm, 64, 1.0, pw, po), (px, px, None, 64, 1.0, pw, po),
                 (px, px, pm, 64, 1.0, None, po), (px, px, pm, 64, 1.0, pw, None)):
        refused(lib.mpgan_masked_image_errors(*args, None), b"masked_image_errors")
    refused(lib.mpgan_masked_image_errors(px, px, pm, 0, 1.0, pw, po, None), b"numel")
    torch.cuda.synchronize()
