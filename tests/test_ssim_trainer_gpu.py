"""The trainer's opt-in SSIM term (variant A, GAN(..., ssim_weight=...)) at the smallest 2-D and 3-D shapes the trainer
tests use: what it logs, that it composes with mi_weight, that validation_step touches no state, and that the default
trainer is bit for bit what it was."""
import functools

import numpy as np
import pytest
import torch

from mpgan_amd import losses

pytestmark = pytest.mark.gpu

SPATIAL = {"2d": (64, 64), "3d": (32, 32, 32)}


def _gan(dims, **kw):
    from mpgan_amd.gan import GAN
    torch.manual_seed(0)
    return GAN(1, *SPATIAL[dims], dimensions=len(SPATIAL[dims]), n_unet_blocks=2, **kw)


@functools.lru_cache(maxsize=None)
def _batch(dims):
    g = torch.Generator().manual_seed(5)
    return {k: (torch.rand(2, 1, *SPATIAL[dims], generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}


def _fit(dims, **kw):
    m = _gan(dims, **kw)
    opts, _ = m.configure_optimizers()
    log = {k: v.clone() for k, v in m.fit_batch(_batch(dims), 0, opts).items()}
    return m, log, opts


def _sum_within_two_ulps(total, terms):
    """total against the float64 sum of the fp32 terms, within 2 fp32 ulps of that sum."""
    want = float(sum(terms))
    ulp = float(np.spacing(np.float32(abs(want))))
    assert abs(float(total) - want) <= 2 * ulp, (float(total), want, ulp)


@pytest.mark.parametrize("dims", list(SPATIAL))
def test_weight_adds_the_logged_term(dims):
    m, log, _ = _fit(dims, ssim_weight=0.5)
    assert "g_ssim_loss" in log and "g_mi_loss" not in log
    assert 0.0 < float(log["g_ssim_loss"]) < 2.0
    # the logged term is the loss of the generator's output (kept by training_step) over the tanh range
    direct = losses.ssim_loss(m.generated_imgs.detach(), _batch(dims)["t2w"], (-1.0, 1.0))
    assert torch.equal(direct, log["g_ssim_loss"])
    _sum_within_two_ulps(log["g_loss"], [float(log["g_adv_loss"]), float(log["g_recon_loss"]),
                                         0.5 * float(log["g_ssim_loss"])])
    assert bool(torch.isfinite(m.generator.store.flat_grad).all())


@pytest.mark.parametrize("dims", list(SPATIAL))
def test_validation_step_logs_the_term_and_touches_no_state(dims):
    m, _, opts = _fit(dims, ssim_weight=0.5)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt_before = [(o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_count) for o in opts]
    grads_before = [net.store.flat_grad.clone() for net in (m.generator, m.discriminator)]
    val = m.validation_step(_batch(dims), 0)
    assert "val_g_ssim_loss" in val and "val_g_ssim_loss" in m.logged and not val["val_g_ssim_loss"].requires_grad
    _sum_within_two_ulps(val["val_g_loss"], [float(val["val_g_adv_loss"]), float(val["val_g_recon_loss"]),
                                             0.5 * float(val["val_g_ssim_loss"])])
    after = m.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    for o, (avg, avg_sq, steps) in zip(opts, opt_before):
        assert torch.equal(o.exp_avg, avg) and torch.equal(o.exp_avg_sq, avg_sq) and o.step_count == steps
    for net, grad in zip((m.generator, m.discriminator), grads_before):
        assert torch.equal(net.store.flat_grad, grad)


def test_composes_with_the_mutual_information_term():
    m, log, _ = _fit("2d", ssim_weight=0.5, mi_weight=0.5)
    assert "g_ssim_loss" in log and "g_mi_loss" in log
    want = (float(log["g_adv_loss"]) + float(log["g_recon_loss"]) + 0.5 * float(log["g_mi_loss"])
            + 0.5 * float(log["g_ssim_loss"]))
    assert abs(float(log["g_loss"]) - want) <= 4 * 2.0 ** -23 * max(abs(want), 1.0)
    val = m.validation_step(_batch("2d"), 0)
    assert "val_g_ssim_loss" in val and "val_g_mi_loss" in val


@pytest.mark.parametrize("dims", list(SPATIAL))
def test_default_trainer_is_unchanged(dims):
    base, log0, _ = _fit(dims)
    zero, log1, _ = _fit(dims, ssim_weight=0.0)
    assert set(log0) == {"g_adv_loss", "g_recon_loss", "g_loss", "d_loss"} == set(log1)
    for k in log0:
        assert torch.equal(log0[k], log1[k]), k
    assert torch.equal(base.generator.store.flat_grad, zero.generator.store.flat_grad)
    for a, b in ((base.generator, zero.generator), (base.discriminator, zero.discriminator)):
        assert torch.equal(a.store.flat, b.store.flat)
    assert "val_g_ssim_loss" not in base.validation_step(_batch(dims), 0)
    assert base.ssim_loss is None and zero.ssim_loss is None
