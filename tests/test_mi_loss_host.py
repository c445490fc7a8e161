"""The torch restatement of the Parzen-window mutual-information loss (mi_loss_ref.py): its closed-form gradient
against autograd, its properties, the argument checks of mpgan_amd.losses and of the C entry points (host side, no
device)."""
import ctypes
import os

import pytest
import torch

import mi_loss_ref as R

SHAPE = (2, 1, 5, 7, 9)


def test_analytic_gradient_equals_autograd_in_fp64():
    """Values outside [0, 1] and values equal to 0.0 and 1.0 are planted: the clamp's closed-interval rule counts."""
    pred, target = R.correlated_pair(SHAPE, seed=1)
    target.reshape(-1)[5] = 0.0
    target.reshape(-1)[6] = 1.0
    target.reshape(-1)[7] = 1.25
    for kw in ({}, {"num_bins": 16, "sigma_ratio": 1.0}, {"value_range": ((-0.5, 1.5), (0.0, 1.0))}):
        _, gp, gt = R.loss_and_gradients(pred, target, reduction="sum", **kw)
        ap, at = R.analytic_gradients(pred, target, **kw)
        assert float((gp + ap).abs().max()) <= 1e-12, kw           # loss = -mi
        assert float((gt + at).abs().max()) <= 1e-12, kw
        assert float(ap.abs().max()) > 1e-4 and float(at.abs().max()) > 1e-4
    ap, _ = R.analytic_gradients(pred, target)
    flat = ap[0].reshape(-1)
    (i0, _), (i1, _), (ilo, _), (ihi, _) = R.PLANTED
    assert flat[i0] != 0 and flat[i1] != 0 and flat[ilo] == 0 and flat[ihi] == 0


def test_marginals_are_the_joints_row_and_column_sums():
    pred, target = R.correlated_pair(SHAPE, seed=2)
    pab, pa, pb = R.joint(pred, target)
    assert float((pab.sum(dim=2) - pa).abs().max()) <= 1e-15
    assert float((pab.sum(dim=1) - pb).abs().max()) <= 1e-15
    assert float((pab.sum(dim=(1, 2)) - 1.0).abs().max()) <= 1e-14


def test_loss_orders_constant_identical_and_independent_pairs():
    const = torch.full(SHAPE, 0.37)
    assert abs(float(R.loss(const, const))) <= 1e-5                 # one bin pair holds everything: mi ~ 0
    x, y = R.independent_pair((2, 1, 16, 16, 16), seed=3)
    same, indep = float(R.loss(x, x)), float(R.loss(x, y))
    assert same < -1.0 and indep > -0.05 and same < indep - 1.0


def test_fp32_peer_is_close_to_the_yardstick():
    pred, target = R.correlated_pair(SHAPE, seed=4)
    l64, g64, _ = R.loss_and_gradients(pred, target)
    l32, g32, _ = R.loss_and_gradients(pred, target, dtype=torch.float32)
    assert abs(float(l64) - float(l32)) <= 1e-5
    assert float((g64 - g32.double()).abs().max()) <= 1e-4 * float(g64.abs().max())


@pytest.mark.parametrize("kwargs,match", [
    ({"num_bins": 33}, "num_bins"),
    ({"num_bins": 1}, "num_bins"),
    ({"reduction": "median"}, "reduction"),
    ({"value_range": (1.0, 1.0)}, "hi > lo"),
    ({"value_range": ((0.0, 1.0), (2.0, -2.0))}, "hi > lo"),
])
def test_configuration_errors_raise_before_any_launch(kwargs, match):
    from mpgan_amd import losses
    x = torch.rand(SHAPE)
    with pytest.raises(ValueError, match=match):
        losses.GlobalMutualInformationLoss(**kwargs)
    with pytest.raises(ValueError, match=match):
        losses.global_mutual_information_loss(x, x, **kwargs)


def test_tensor_errors_raise_on_cpu_tensors():
    from mpgan_amd import losses
    x = torch.rand(SHAPE)
    mod = losses.GlobalMutualInformationLoss()
    with pytest.raises(ValueError, match="shape mismatch"):
        mod(x, torch.rand(2, 1, 5, 7, 8))
    with pytest.raises(ValueError, match="fp32 device"):
        mod(x, x)                                                   # fp32, but not on the device
    with pytest.raises(ValueError, match="fp32 device"):
        mod(x.double(), x.double())
    with pytest.raises(ValueError, match="shape mismatch"):
        losses.parzen_joint_histogram(x, x[:1])
    with pytest.raises(ValueError, match="fp32 device"):
        losses.parzen_joint_histogram(x, x)
    with pytest.raises(ValueError, match="num_bins"):
        losses.parzen_joint_histogram(x, x, num_bins=40)


def test_trainer_keywords_exist_and_default_to_off():
    import inspect
    from mpgan_amd.gan import GAN
    sig = inspect.signature(GAN.__init__).parameters
    assert sig["mi_weight"].default == 0.0 and sig["mi_weight"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["mi_bins"].default == 23 and sig["mi_bins"].kind is inspect.Parameter.KEYWORD_ONLY


def _lib():
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmpgan_hip.so not built (run __graft_entry__.build())")
    return _lib.lib()


def test_workspace_query():
    lib = _lib()
    sizes = [lib.mpgan_parzen_mi_workspace(b, 65536, 23) for b in (1, 2, 4, 16)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert lib.mpgan_parzen_mi_workspace(1, 1, 2) > 0
    assert lib.mpgan_parzen_mi_workspace(4, 128 ** 3, 32) >= lib.mpgan_parzen_mi_workspace(4, 128 ** 3 - 1, 32)
    for bad in ((0, 10, 23), (1, 0, 23), (1, 10, 1), (1, 10, 33)):
        assert lib.mpgan_parzen_mi_workspace(*bad) == -1


def test_entry_points_refuse_bad_arguments_on_the_host():
    lib = _lib()
    rc = lib.mpgan_parzen_mi_forward(None, None, 10, 1, 0.0, 1.0, 0.0, 1.0, 23, 0.5, 1e-7, 1e-7, None, 0, None, None,
                                     None, 0, None, None)
    assert rc == -1 and b"parzen_mi_forward" in lib.mpgan_last_error()
    rc = lib.mpgan_parzen_mi_backward(None, None, 10, 1, 0.0, 1.0, 0.0, 1.0, 23, 0.5, None, None, 0, -1.0, 0, None, None)
    assert rc == -1 and b"parzen_mi_backward" in lib.mpgan_last_error()
    # non-null (host) pointers: every check below fails before anything would be launched or dereferenced
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    fwd = lambda **k: lib.mpgan_parzen_mi_forward(p, p, k.get("n", 10), k.get("batch", 1), 0.0, k.get("hi", 1.0), 0.0, 1.0,
                                                  k.get("bins", 23), 0.5, 1e-7, 1e-7, p, k.get("ws", 1 << 16), None, p, p,
                                                  k.get("reduction", 0), p, None)
    assert fwd(bins=33) == -1 and b"bins 33" in lib.mpgan_last_error()
    assert fwd(bins=1) == -1 and b"bins 1" in lib.mpgan_last_error()
    assert fwd(hi=0.0) == -1 and b"hi > lo" in lib.mpgan_last_error()
    assert fwd(batch=0) == -1 and b"batch" in lib.mpgan_last_error()
    assert fwd(reduction=3) == -1 and b"reduction" in lib.mpgan_last_error()
    assert fwd(ws=16) == -1 and b"workspace too small" in lib.mpgan_last_error()
    bwd = lambda **k: lib.mpgan_parzen_mi_backward(p, p, 10, 1, 0.0, 1.0, 0.0, 1.0, k.get("bins", 23), 0.5, p, p, 0, -1.0,
                                                   k.get("wrt", 0), p, None)
    assert bwd(bins=33) == -1 and b"bins 33" in lib.mpgan_last_error()
    assert bwd(wrt=2) == -1 and b"wrt" in lib.mpgan_last_error()
