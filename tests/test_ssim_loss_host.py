"""The torch restatement of the SSIM loss (ssim_loss_ref.py): its forward against the metrics oracle, its closed-form
gradient against float64 autograd, the argument checks of mpgan_amd.losses, of GAN's ssim_weight and of the C entry
points (host side, no device)."""
import ctypes
import os

import pytest
import torch

import ssim_loss_ref as R
from oracle import metrics_ref

SHAPES = [(1, 1, 7, 7), (2, 1, 9, 39), (1, 2, 17, 45), (1, 1, 7, 7, 7), (1, 1, 9, 10, 40), (2, 1, 13, 21, 37)]


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_equals_the_metrics_oracle_per_item(shape):
    pred, target = R.structured_pair(shape, seed=1)
    for value_range in ((-1.0, 1.0), (-2.0, 3.0)):
        lo, hi = value_range
        got = R.ssim_items(pred, target, value_range)
        for b in range(shape[0]):
            for c in range(shape[1]):
                want = metrics_ref.structural_similarity(pred[b, c].double().numpy() - lo,
                                                         target[b, c].double().numpy() - lo, data_range=hi - lo)
                assert abs(float(got[b, c]) - want) <= 1e-12, (shape, b, c)


@pytest.mark.parametrize("shape", SHAPES)
def test_analytic_gradient_equals_autograd_in_fp64(shape):
    pred, target = R.structured_pair(shape, seed=2)
    _, gp, gt = R.loss_and_gradients(pred, target, value_range=(-1.0, 1.0), reduction="sum")
    ap, at = R.analytic_gradients(pred, target, value_range=(-1.0, 1.0))
    assert float((gp + ap).abs().max()) <= 1e-12                    # loss = 1 - ssim
    assert float((gt + at).abs().max()) <= 1e-12
    assert float(ap.abs().max()) > 1e-6 and float(at.abs().max()) > 1e-6


def test_structured_pair_has_background_and_a_flat_block():
    pred, target = R.structured_pair((2, 1, 13, 21, 37), seed=3)
    assert float(pred.min()) >= -1 and float(pred.max()) <= 1 and float(target.min()) >= -1 and float(target.max()) <= 1
    both = (pred == -1) & (target == -1)
    assert 0.2 <= float(both.float().mean()) <= 0.4
    assert bool((pred[:, :, 2:11, 6:15, 14:23] == 0.8).all()) and bool((target[:, :, 2:11, 6:15, 14:23] == 0.8).all())
    x = pred.double().reshape(2, 1, 13, 21, 37) + 1.0
    var = R._box(x * x, 3) / 343 - (R._box(x, 3) / 343) ** 2
    assert int((var.abs() <= 1e-12).sum()) >= 27                    # windows inside the block: zero variance


def test_reductions_of_the_restatement():
    pred, target = R.structured_pair((2, 3, 9, 11), seed=4)
    items = 1.0 - R.ssim_items(pred, target, (-1.0, 1.0))
    assert tuple(items.shape) == (2, 3)
    assert torch.equal(R.loss(pred, target, (-1.0, 1.0), "none"), items.mean(dim=1))
    assert abs(float(R.loss(pred, target, (-1.0, 1.0), "sum")) - float(items.sum())) <= 1e-14
    assert abs(float(R.loss(pred, target, (-1.0, 1.0), "mean")) - float(items.mean())) <= 1e-14
    assert abs(float(R.loss(pred, pred, (-1.0, 1.0)))) <= 1e-14


@pytest.mark.parametrize("kwargs,match", [
    ({"reduction": "median"}, "reduction"),
    ({"value_range": (1.0, 1.0)}, "hi > lo"),
    ({"value_range": (1.0, -1.0)}, "hi > lo"),
    ({"value_range": ((0.0, 1.0), (0.0, 1.0))}, "value_range"),
])
def test_configuration_errors_raise_before_any_launch(kwargs, match):
    from mpgan_amd import losses
    x = torch.rand(1, 1, 9, 9)
    with pytest.raises(ValueError, match=match):
        losses.SSIMLoss(**kwargs)
    with pytest.raises(ValueError, match=match):
        losses.ssim_loss(x, x, **kwargs)


def test_tensor_errors_raise_on_cpu_tensors():
    from mpgan_amd import losses
    x = torch.rand(1, 1, 9, 9)
    mod = losses.SSIMLoss()
    with pytest.raises(ValueError, match="shape mismatch"):
        mod(x, torch.rand(1, 1, 9, 8))
    with pytest.raises(ValueError, match="fp32 device"):
        mod(x, x)                                                   # fp32, but not on the device
    with pytest.raises(ValueError, match="fp32 device"):
        mod(x.double(), x.double())
    with pytest.raises(ValueError, match="below the 7-wide window"):
        mod(torch.rand(1, 1, 6, 9), torch.rand(1, 1, 6, 9))
    with pytest.raises(ValueError, match="below the 7-wide window"):
        mod(torch.rand(1, 1, 3, 9, 9), torch.rand(1, 1, 3, 9, 9))   # a 3-D depth in 2..6
    with pytest.raises(ValueError, match="expects"):
        mod(torch.rand(9, 9), torch.rand(9, 9))


def test_trainer_keyword_defaults_to_off_and_refuses_a_negative_weight():
    import inspect
    from mpgan_amd.gan import GAN
    sig = inspect.signature(GAN.__init__).parameters
    assert sig["ssim_weight"].default == 0.0 and sig["ssim_weight"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError, match="ssim_weight"):
        GAN(1, 64, 64, dimensions=2, n_unet_blocks=2, ssim_weight=-0.5)     # checked before any device work


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
    ws = lib.mpgan_ssim_loss_workspace(_dhw(1, 7, 7), 1, 0, ctypes.byref(coef))
    assert ws == 16 and coef.value == 0                             # one tile partial + one item
    sizes = []
    for mask, maps in ((0, 0), (1, 3), (2, 3), (3, 4)):
        ws = lib.mpgan_ssim_loss_workspace(_dhw(13, 21, 37), 2, mask, ctypes.byref(coef))
        assert ws > 0 and coef.value == maps * 2 * (7 * 15 * 31) * 8
        sizes.append(ws)
    assert len(set(sizes)) == 1                                     # the workspace does not depend on the mask
    assert lib.mpgan_ssim_loss_workspace(_dhw(128, 128, 128), 4, 1, None) > 0
    for bad in ((_dhw(1, 6, 9), 1, 0), (_dhw(3, 9, 9), 1, 0), (_dhw(0, 9, 9), 1, 0), (_dhw(1, 9, 9), 0, 0),
                (_dhw(1, 9, 9), 1, 4), (None, 1, 0)):
        assert lib.mpgan_ssim_loss_workspace(*bad, None) == -1


def test_entry_points_refuse_bad_arguments_on_the_host():
    lib = _lib()
    rc = lib.mpgan_ssim_loss_forward(None, None, _dhw(1, 9, 9), 1, 1, 0.0, 1.0, 0, None, 0, None, 0, 0, None, None)
    assert rc == -1 and b"ssim_loss_forward" in lib.mpgan_last_error()
    rc = lib.mpgan_ssim_loss_backward(None, None, _dhw(1, 9, 9), 1, 1, 0.0, 1, None, 0, None, 0, -1.0, 0, None, None)
    assert rc == -1 and b"ssim_loss_backward" in lib.mpgan_last_error()
    # non-null (host) pointers: every check below fails before anything would be launched or dereferenced
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    fwd = lambda **k: lib.mpgan_ssim_loss_forward(p, p, k.get("dhw", _dhw(1, 9, 9)), k.get("items", 1), k.get("ch", 1), 0.0,
                                                  k.get("hi", 1.0), k.get("mask", 1), p, k.get("ws", 1 << 16), p,
                                                  k.get("coef", 1 << 16), k.get("reduction", 0), p, None)
    assert fwd(dhw=_dhw(1, 6, 9)) == -1 and b"below the 7-wide window" in lib.mpgan_last_error()
    assert fwd(dhw=_dhw(3, 9, 9)) == -2 and b"depth 3" in lib.mpgan_last_error()
    assert fwd(hi=0.0) == -1 and b"hi > lo" in lib.mpgan_last_error()
    assert fwd(items=0) == -1 and b"items" in lib.mpgan_last_error()
    assert fwd(items=3, ch=2) == -1 and b"channels" in lib.mpgan_last_error()
    assert fwd(mask=4) == -1 and b"grad_mask" in lib.mpgan_last_error()
    assert fwd(reduction=3) == -1 and b"reduction" in lib.mpgan_last_error()
    assert fwd(ws=8) == -1 and b"workspace too small" in lib.mpgan_last_error()
    assert fwd(coef=16) == -1 and b"coef" in lib.mpgan_last_error()
    bwd = lambda **k: lib.mpgan_ssim_loss_backward(p, p, k.get("dhw", _dhw(1, 9, 9)), 1, 1, 0.0, k.get("mask", 1), p,
                                                   k.get("coef", 1 << 16), p, 0, -1.0, k.get("wrt", 0), p, None)
    assert bwd(dhw=_dhw(3, 9, 9)) == -2 and b"depth 3" in lib.mpgan_last_error()
    assert bwd(wrt=2) == -1 and b"wrt" in lib.mpgan_last_error()
    assert bwd(mask=1, wrt=1) == -1 and b"no maps" in lib.mpgan_last_error()
    assert bwd(coef=16) == -1 and b"coef too small" in lib.mpgan_last_error()
