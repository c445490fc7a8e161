"""The torch restatement of the masked SSIM (masked_ssim_ref.py): its closed-form gradient against float64 autograd, the
all-ones and all-zero masks, and the argument checks of mpgan_amd.losses.ssim_loss(mask= / threshold=), of GAN's
fg_ssim_weight and of the C entry points (host side, no device)."""
import ctypes
import inspect
import os

import pytest
import torch

import masked_ssim_ref as MR
import ssim_loss_ref as R

SHAPES = [(2, 1, 9, 39), (1, 2, 17, 45), (1, 1, 9, 10, 40), (2, 1, 13, 21, 37)]       # cases b, c, e, f
RANGE = (-1.0, 1.0)


@pytest.mark.parametrize("shape", SHAPES)
def test_closed_form_equals_autograd_in_fp64(shape):
    pred, target = R.structured_pair(shape, seed=2)
    mask = MR.random_mask(shape, seed=5)
    _, gp, gt = MR.loss_and_gradients(pred, target, mask, value_range=RANGE, reduction="sum")
    ap, at = MR.analytic_gradients(pred, target, mask, RANGE)
    assert float((gp + ap).abs().max()) <= 1e-12                    # loss = 1 - ssim
    assert float((gt + at).abs().max()) <= 1e-12
    assert float(ap.abs().max()) > 1e-6 and float(at.abs().max()) > 1e-6
    # a mask with channel extent 1 is the same mask on every channel
    one = mask[:, :1]
    full = one.expand(shape)
    assert torch.equal(MR.items_and_counts(pred, target, one, RANGE)[0], MR.items_and_counts(pred, target, full, RANGE)[0])


@pytest.mark.parametrize("shape", SHAPES + [(1, 1, 7, 7), (1, 1, 7, 7, 7)])
def test_all_ones_mask_is_the_plain_ssim(shape):
    pred, target = R.structured_pair(shape, seed=3)
    ones = torch.ones(shape, dtype=torch.uint8)
    item, cnt = MR.items_and_counts(pred, target, ones, RANGE)
    plain = R.ssim_items(pred, target, RANGE)
    assert float((item - plain).abs().max()) <= 1e-15
    windowed = [s for s in shape[2:]]
    m = 1
    for s in windowed:
        m *= s - 6
    assert bool((cnt == m).all())
    ga, gb = MR.analytic_gradients(pred, target, ones, RANGE)
    pa, pb = R.analytic_gradients(pred, target, RANGE)
    assert float((ga - pa).abs().max()) <= 1e-15 and float((gb - pb).abs().max()) <= 1e-15


@pytest.mark.parametrize("shape", SHAPES)
def test_all_zero_mask_gives_loss_zero_nan_items_and_zero_gradients(shape):
    pred, target = R.structured_pair(shape, seed=4)
    zeros = torch.zeros(shape, dtype=torch.uint8)
    item, cnt = MR.items_and_counts(pred, target, zeros, RANGE)
    assert bool(torch.isnan(item).all()) and bool((cnt == 0).all())
    for reduction in ("mean", "sum", "none"):
        out, gp, gt = MR.loss_and_gradients(pred, target, zeros, value_range=RANGE, reduction=reduction)
        assert bool((out == 0).all()) and bool((gp == 0).all()) and bool((gt == 0).all())
    ga, gb = MR.analytic_gradients(pred, target, zeros, RANGE)
    assert bool((ga == 0).all()) and bool((gb == 0).all())
    # a mask set only in the 3-wide border ring is empty too: the interior drops those voxels
    ring = torch.ones(shape, dtype=torch.uint8)
    d = 2 if len(shape) == 4 or shape[2] == 1 else 3
    ring[(Ellipsis,) + (slice(3, -3),) * d] = 0
    assert int(ring.sum()) > 0 and bool((MR.items_and_counts(pred, target, ring, RANGE)[1] == 0).all())


def test_the_weight_is_read_at_the_window_centre():
    """One voxel set: exactly the window whose corner is that voxel - 3 is averaged."""
    pred, target = R.structured_pair((1, 1, 12, 15), seed=6)
    mask = torch.zeros((1, 1, 12, 15), dtype=torch.uint8)
    mask[0, 0, 5, 9] = 7
    item, cnt = MR.items_and_counts(pred, target, mask, RANGE)
    assert float(cnt) == 1.0 and float(item) == float(MR.ssim_map(pred, target, RANGE)[0, 0, 2, 6])
    assert tuple(MR.ssim_map(pred, target, RANGE).shape) == (1, 1, 6, 9)


# ---- mpgan_amd.losses / GAN: refused before any launch ------------------------------------------------------------------
def test_ssim_loss_refuses_bad_masks_and_thresholds():
    from mpgan_amd import losses
    x = torch.rand(1, 2, 9, 11)
    ok = torch.ones(1, 2, 9, 11, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at most one of mask and threshold"):
        losses.ssim_loss(x, x, mask=ok, threshold="otsu")
    with pytest.raises(ValueError, match="bool / uint8"):
        losses.ssim_loss(x, x, mask=ok.float())                       # a wrong dtype
    with pytest.raises(ValueError, match="bool / uint8"):
        losses.ssim_loss(x, x, mask=[[1]])
    with pytest.raises(ValueError, match="channel extent 1"):
        losses.ssim_loss(x, x, mask=ok[..., :10])                     # a wrong shape
    with pytest.raises(ValueError, match="channel extent 1"):
        losses.ssim_loss(x, x, mask=ok[:, :, 0])
    with pytest.raises(ValueError, match="inputs' device"):
        losses.ssim_loss(x, x, mask=torch.empty(1, 2, 9, 11, dtype=torch.uint8, device="meta"))    # a wrong device
    for bad in ("mean", float("nan"), float("inf"), None.__class__, [0.5]):
        with pytest.raises(ValueError, match="threshold"):
            losses.ssim_loss(x, x, threshold=bad)
    with pytest.raises(ValueError, match="threshold"):
        losses.SSIMLoss(threshold="median")
    with pytest.raises(ValueError, match="threshold"):
        losses.ForegroundSSIMLoss(threshold=torch.zeros(1))
    with pytest.raises(ValueError, match="bins"):
        losses.ForegroundSSIMLoss(bins=1)
    # a legal mask / threshold on tensors that are not on the device: the plain path's complaint, before any launch
    with pytest.raises(ValueError, match="fp32 device"):
        losses.ssim_loss(x, x, mask=ok[:, :1])
    with pytest.raises(ValueError, match="fp32 device"):
        losses.SSIMLoss(RANGE, threshold=0.0)(x, x)
    with pytest.raises(ValueError, match="fp32 device"):
        losses.ForegroundSSIMLoss()(x, x)
    sig = inspect.signature(losses.ssim_loss).parameters
    assert [k for k, v in sig.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == ["mask", "threshold", "bins"]
    assert list(inspect.signature(losses.SSIMLoss.forward).parameters) == ["self", "pred", "target", "mask"]


def test_trainer_keyword_defaults_to_off_and_refuses_a_negative_weight():
    from mpgan_amd.gan import GAN
    sig = inspect.signature(GAN.__init__).parameters
    assert sig["fg_ssim_weight"].default == 0.0 and sig["fg_ssim_weight"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError, match="fg_ssim_weight"):
        GAN(1, 64, 64, dimensions=2, n_unet_blocks=2, fg_ssim_weight=-0.5)     # checked before any device work
    with pytest.raises(ValueError, match="fg_ssim_weight"):
        GAN(1, 64, 64, dimensions=2, n_unet_blocks=2, fg_ssim_weight=float("nan"))
    from mpgan_amd.gan_patch import GAN as PatchGAN
    assert "fg_ssim_weight" not in inspect.signature(PatchGAN.__init__).parameters       # variant B does not take it


def test_metrics_signatures():
    from mpgan_amd import metrics
    sig = inspect.signature(metrics.ssim).parameters
    assert list(sig) == ["a", "b", "data_range", "mask"] and sig["mask"].default is None
    assert list(inspect.signature(metrics.ssim_map).parameters) == ["a", "b", "data_range"]
    x = torch.rand(9, 9)
    with pytest.raises(ValueError, match="device"):
        metrics.ssim(x, x, mask=torch.ones(9, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="same-shape"):
        metrics.ssim_map(x, torch.rand(9, 8))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def _lib():
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmpgan_hip.so not built (run __graft_entry__.build())")
    return _lib.lib()


def _dhw(*v):
    return (ctypes.c_int32 * 3)(*v)


def test_workspace_query():
    lib = _lib()
    coef = ctypes.c_int64(-5)
    ws = lib.mpgan_masked_ssim_loss_workspace(_dhw(1, 7, 7), 1, 0, ctypes.byref(coef))
    assert ws == 24 and coef.value == 0                             # one partial, one count, one item
    for grads, maps in ((0, 0), (1, 3), (2, 3), (3, 4)):
        plain = lib.mpgan_ssim_loss_workspace(_dhw(13, 21, 37), 2, grads, None)
        ws = lib.mpgan_masked_ssim_loss_workspace(_dhw(13, 21, 37), 2, grads, ctypes.byref(coef))
        assert ws == 2 * plain - 2 * 8 and coef.value == maps * 2 * (7 * 15 * 31) * 8
    for bad in ((_dhw(1, 6, 9), 1, 0), (_dhw(3, 9, 9), 1, 0), (_dhw(0, 9, 9), 1, 0), (_dhw(1, 9, 9), 0, 0),
                (_dhw(1, 9, 9), 1, 4), (None, 1, 0)):
        assert lib.mpgan_masked_ssim_loss_workspace(*bad, None) == -1


def test_entry_points_refuse_bad_arguments_on_the_host():
    lib = _lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    assert p % 8 == 0

    def fwd(**k):
        return lib.mpgan_masked_ssim_loss_forward(
            k.get("a", p), k.get("b", p), k.get("dhw", _dhw(1, 9, 9)), k.get("items", 1), k.get("ch", 1), 0.0,
            k.get("hi", 1.0), k.get("mask", p), k.get("thr", None), k.get("grads", 1), k.get("wsp", p),
            k.get("ws", 1 << 16), k.get("coefp", p), k.get("coef", 1 << 16), k.get("stats", p), k.get("smap", None),
            k.get("reduction", 0), k.get("loss", p), None)

    for name in ("a", "b", "wsp", "stats", "loss"):
        assert fwd(**{name: None}) == -1 and b"masked_ssim_loss_forward: null pointer" in lib.mpgan_last_error(), name
    assert fwd(thr=p) == -1 and b"masked_ssim_loss_forward" in lib.mpgan_last_error() and b"both" in lib.mpgan_last_error()
    assert fwd(dhw=None) == -1 and b"null dhw" in lib.mpgan_last_error()
    assert fwd(dhw=_dhw(1, 6, 9)) == -1 and b"below the 7-wide window" in lib.mpgan_last_error()
    assert fwd(dhw=_dhw(3, 9, 9)) == -2 and b"depth 3" in lib.mpgan_last_error()
    assert fwd(hi=0.0) == -1 and b"hi > lo" in lib.mpgan_last_error()
    assert fwd(items=0) == -1 and b"items" in lib.mpgan_last_error()
    assert fwd(items=3, ch=2) == -1 and b"channels" in lib.mpgan_last_error()
    assert fwd(ch=0) == -1 and b"channels" in lib.mpgan_last_error()
    assert fwd(grads=4) == -1 and b"grad_mask" in lib.mpgan_last_error()
    assert fwd(grads=-1) == -1 and b"grad_mask" in lib.mpgan_last_error()
    assert fwd(reduction=3) == -1 and b"reduction" in lib.mpgan_last_error()
    assert fwd(ws=16) == -1 and b"workspace too small" in lib.mpgan_last_error()     # the plain form's size: one short
    assert fwd(wsp=p + 4) == -1 and b"workspace must be 8-byte aligned" in lib.mpgan_last_error()
    assert fwd(coef=16) == -1 and b"coef" in lib.mpgan_last_error()
    assert fwd(coefp=None) == -1 and b"coef" in lib.mpgan_last_error()
    assert fwd(stats=p + 4) == -1 and b"aligned" in lib.mpgan_last_error()

    def bwd(**k):
        return lib.mpgan_masked_ssim_loss_backward(
            k.get("a", p), k.get("b", p), k.get("dhw", _dhw(1, 9, 9)), k.get("items", 1), k.get("ch", 1), 0.0,
            k.get("grads", 1), k.get("coefp", p), k.get("coef", 1 << 16), k.get("stats", p), k.get("up", p),
            k.get("stride", 0), -1.0, k.get("wrt", 0), k.get("grad", p), None)

    for name in ("a", "b", "coefp", "stats", "up", "grad"):
        assert bwd(**{name: None}) == -1 and b"masked_ssim_loss_backward: null pointer" in lib.mpgan_last_error(), name
    assert bwd(dhw=_dhw(3, 9, 9)) == -2 and b"depth 3" in lib.mpgan_last_error()
    assert bwd(dhw=_dhw(1, 9, 6)) == -1 and b"below the 7-wide window" in lib.mpgan_last_error()
    assert bwd(items=70000) == -1 and b"items" in lib.mpgan_last_error()
    assert bwd(items=3, ch=2) == -1 and b"channels" in lib.mpgan_last_error()
    assert bwd(wrt=2) == -1 and b"wrt" in lib.mpgan_last_error()
    assert bwd(grads=1, wrt=1) == -1 and b"no maps" in lib.mpgan_last_error()
    assert bwd(grads=0) == -1 and b"grad_mask" in lib.mpgan_last_error()
    assert bwd(stride=2) == -1 and b"upstream_stride" in lib.mpgan_last_error()
    assert bwd(coef=16) == -1 and b"coef too small" in lib.mpgan_last_error()
