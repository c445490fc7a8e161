"""The references of the foreground-mask kernels checked against themselves on the CPU (tests/foreground_ref.py), the
conditions the GPU tests place on their inputs, and the argument errors of the Python layer that are raised before the
library is touched."""
import numpy as np
import pytest
import torch

import foreground_ref as R


def test_otsu_of_a_two_level_image_lands_between_the_levels():
    rng = np.random.RandomState(0)
    for bins in R.BINS:
        for low, high, share in ((-0.8, 0.6, 0.3), (-1.0, 1.0, 0.5), (-0.2, 0.1, 0.9)):
            x = np.where(rng.rand(4000) < share, high, low).astype(np.float32)
            thr = float(R.otsu_threshold(x, -1.0, 1.0, bins))
            width = 2.0 / bins
            # var_k is the same for every boundary between the two occupied bins and the FIRST one is taken: the
            # threshold is the centre of the lower level's bin, within half a bin of that level and below the upper one
            assert low - width / 2 <= thr < high, (bins, low, high, thr)
            if low == -1.0:                              # a background at lo (the workload's) lies below its bin's centre
                mask = R.foreground(x[None], [thr])[0]
                assert mask.sum() == (x == np.float32(high)).sum()


def test_otsu_degenerate_cases_of_the_reference():
    assert np.isnan(R.otsu_threshold(np.full(10, 5.0, np.float32), -1.0, 1.0, 64))          # nothing inside the range
    assert np.isnan(R.otsu_threshold(np.full(10, np.nan, np.float32), -1.0, 1.0, 64))
    one = R.otsu_threshold(np.full(10, 0.3, np.float32), -1.0, 1.0, 64)                      # one occupied bin
    k = int(np.floor((np.float32(0.3) + np.float32(1.0)) * np.float32(32.0)))
    assert one == np.float32(R.centre(k, -1.0, 1.0, 64))
    counts = R.histogram(np.array([-1.0, 1.0, 1.5, -1.5, np.nan], np.float32), -1.0, 1.0, 2)
    assert counts.tolist() == [1, 1]                                                         # lo and hi in, the rest out


@pytest.mark.parametrize("bins", R.BINS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_shared_otsu_inputs_have_one_clear_maximum(shape, bins):
    """The condition the GPU test asserts before it asks for equal bits: the two largest var_k are apart."""
    _, counts, thr = R.otsu_case(shape, bins)
    for c in counts:
        assert R.sigma_gap(c, -1.0, 1.0) > R.SIGMA_GAP
    assert np.isfinite(thr).all()
    if shape[0] * shape[1] > 1 and bins > 2:
        assert len(set(thr.tolist())) > 1                # different mixtures, different thresholds


@pytest.mark.parametrize("shape", R.SHAPES)
def test_shared_l1_targets_have_one_clear_maximum_and_mixed_masks(shape):
    pred, target, thr = R.l1_case(shape)
    for row, t in zip(target.reshape(shape[0] * shape[1], -1), thr):
        assert R.sigma_gap(R.histogram(row, -1.0, 1.0, 256), -1.0, 1.0) > R.SIGMA_GAP
        assert 0 < (row > t).sum() < row.size            # both weights are in play
    assert (pred == target).any() and (pred != target).any()


@pytest.mark.parametrize("reduction", R.REDUCTIONS)
@pytest.mark.parametrize("weights", R.WEIGHTS + ((0.0, 0.0),))
def test_closed_form_gradient_equals_autograd(weights, reduction):
    shape = (2, 2, 3, 5, 4)
    rng = np.random.RandomState(7)
    pred, target = rng.randn(*shape), rng.randn(*shape)
    same = rng.rand(*shape) < 0.2
    pred[same] = target[same]
    mask = rng.rand(*shape) < 0.4
    mask[1, 1] = False                                   # an item without foreground: den == 0 when w_bg == 0
    gout = rng.rand(2) + 0.5 if reduction == "none" else np.float64(1.7)
    p = torch.from_numpy(pred).requires_grad_(True)
    t = torch.from_numpy(target).requires_grad_(True)
    loss = R.masked_l1_torch(p, t, torch.from_numpy(mask), *weights, reduction)
    loss.backward(torch.as_tensor(gout, dtype=torch.float64))
    want = R.masked_l1_grad(pred, target, mask, *weights, reduction, gout)
    assert np.abs(p.grad.numpy() - want).max() <= 1e-12
    assert np.abs(t.grad.numpy() + want).max() <= 1e-12
    assert (want[same] == 0).all()
    if weights[1] == 0.0:
        assert (want[1, 1] == 0).all()
        item = R.masked_l1_numpy(pred, target, mask, *weights, "none")
        ref = R.masked_l1_numpy(pred[:, :1], target[:, :1], mask[:, :1], *weights, "none")
        assert item[1] == 0.5 * ref[1]                   # the empty item contributes 0 to its batch entry's mean


def test_box_restatement_equals_brute_force():
    rng = np.random.RandomState(3)
    for shape in ((1, 5, 7), (3, 17, 19), (9, 1, 1), (6, 6, 6)):
        for margin in ((0, 0, 0), (1, 2, 3), (100, 0, 1)):            # the last clips at both faces
            for _ in range(6):
                mask = rng.rand(*shape) < rng.choice([0.01, 0.1, 0.6])
                assert (R.bounding_box(mask, margin) == R.bounding_box_brute(mask, margin)).all()
    mask = np.zeros((4, 5, 6), bool)
    assert (R.bounding_box(mask, (1, 1, 1)) == 0).all()                # empty: start = end = 0
    mask[1, 2, 3] = True
    assert R.bounding_box(mask, (5, 5, 5)).tolist() == [[0, 0, 0], [4, 5, 6]]
    assert R.bounding_box(mask).tolist() == [[1, 2, 3], [2, 3, 4]]


def test_masked_errors_reference():
    a = np.array([0.0, 1.0, 2.0, 3.0], np.float32)
    b = np.array([0.0, 3.0, 2.0, 0.0], np.float32)
    assert R.masked_errors(a, b, [0, 1, 0, 1], 2.0) == (2.5, 6.5, float(10 * np.log10(4.0 / 6.5)), 2)
    assert R.masked_errors(a, b, [1, 0, 1, 0], 2.0)[1:] == (0.0, float("inf"), 2)
    out = R.masked_errors(a, b, [0, 0, 0, 0], 2.0)
    assert np.isnan(out[0]) and np.isnan(out[1]) and np.isnan(out[2]) and out[3] == 0


# ---- the Python layer's argument errors, raised before the library is touched -----------------------------------------
def test_preprocess_argument_errors():
    from mpgan_amd import preprocess as P
    x = torch.zeros(1, 1, 8, 8)                          # a CPU tensor: refused before any launch
    for fn in (P.otsu_threshold, P.foreground_mask, P.foreground_bbox, P.crop_foreground):
        with pytest.raises(ValueError, match="fp32 device tensor"):
            fn(x)
    with pytest.raises(ValueError, match="bins"):
        P.otsu_threshold(x, bins=1)
    with pytest.raises(ValueError, match="bins"):
        P.otsu_threshold(x, bins=257)
    with pytest.raises(ValueError, match="value_range"):
        P.otsu_threshold(x, value_range=(1.0, 1.0))
    for bad in ("mean", None, float("nan"), float("inf"), True, [0.5]):
        with pytest.raises(ValueError, match="threshold"):
            P.check_threshold(bad, "t")
    for good in ("otsu", 0, -0.5, np.float32(0.25), torch.zeros(3)):
        P.check_threshold(good, "t")
    for bad in (-1, 1.5, (1, 2), (0, -1, 0)):
        with pytest.raises(ValueError, match="margin"):
            P._margin3(bad, 3, "m")
    assert P._margin3(2, 2, "m") == (0, 2, 2) and P._margin3((1, 2, 3), 3, "m") == (1, 2, 3)


def test_masked_l1_argument_errors():
    from mpgan_amd import losses as L
    p, t = torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, 4, 4)
    m = torch.zeros(2, 1, 4, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="exactly one of mask and threshold"):
        L.masked_l1_loss(p, t)
    with pytest.raises(ValueError, match="exactly one of mask and threshold"):
        L.masked_l1_loss(p, t, m, threshold="otsu")
    with pytest.raises(ValueError, match="reduction"):
        L.masked_l1_loss(p, t, m, reduction="avg")
    with pytest.raises(ValueError, match="fg_weight"):
        L.masked_l1_loss(p, t, m, fg_weight=-1.0)
    with pytest.raises(ValueError, match="bg_weight"):
        L.masked_l1_loss(p, t, m, bg_weight=float("inf"))
    with pytest.raises(ValueError, match="threshold"):
        L.masked_l1_loss(p, t, threshold="li")
    with pytest.raises(ValueError, match="bool / uint8"):
        L.masked_l1_loss(p, t, m.float())
    with pytest.raises(ValueError, match="shape mismatch"):
        L.masked_l1_loss(p, t[:1], m)
    with pytest.raises(ValueError, match=r"\(B, C, H, W\)"):
        L.masked_l1_loss(p[0], t[0], m[0])
    with pytest.raises(ValueError, match="two fp32 device tensors"):
        L.masked_l1_loss(p, t, m)                        # CPU tensors
    with pytest.raises(ValueError, match="threshold"):
        L.ForegroundL1Loss(threshold="mean")
    with pytest.raises(ValueError, match="bins"):
        L.ForegroundL1Loss(bins=1000)
    with pytest.raises(ValueError, match="reduction"):
        L.MaskedL1Loss(reduction="avg")
    assert L.ForegroundL1Loss().threshold == "otsu" and L.ForegroundL1Loss(0.25).threshold == 0.25


def test_image_errors_mask_argument_errors():
    from mpgan_amd import metrics as M
    a = torch.zeros(4, 4)
    with pytest.raises(ValueError, match="shape mismatch"):
        M.image_errors(a, a[:2], mask=torch.ones(4, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="fp32 device tensors"):
        M.image_errors(a, a, mask=torch.ones(4, 4, dtype=torch.bool))


def test_gan_keyword_validation():
    """Raised beside the other keyword checks, before any network is built (no device is needed to get here)."""
    from mpgan_amd.gan import GAN
    for kw, match in ((dict(fg_weight=-0.5), "fg_weight"), (dict(fg_weight=float("nan")), "fg_weight"),
                      (dict(fg_weight=1.0, fg_threshold="mean"), "fg_threshold"),
                      (dict(fg_weight=1.0, fg_threshold=float("inf")), "fg_threshold"),
                      (dict(fg_threshold=float("nan")), "fg_threshold"),
                      (dict(fg_threshold=torch.zeros(1)), "fg_threshold")):
        with pytest.raises(ValueError, match=match):
            GAN(1, 16, 16, dimensions=2, n_unet_blocks=2, device="cpu", **kw)
