"""The trainer's opt-in edge term (variant A, GAN(..., edge_weight=...)) at the smallest 2-D and 3-D shapes the trainer
tests use: what it logs, that it composes with ssim_weight, mi_weight, pair_augment and a DiffAugment policy, that
validation_step touches no state, that the option adds no state_dict key, and that the default trainer is bit for bit what
it was."""
import functools

import numpy as np
import pytest
import torch

from mpgan_amd import losses

pytestmark = pytest.mark.gpu

SPATIAL = {"2d": (64, 64), "3d": (32, 32, 32)}
BASE_LOG = {"g_adv_loss", "g_recon_loss", "g_loss", "d_loss"}


def _gan(dims, **kw):
    from mpgan_amd.gan import GAN
    torch.manual_seed(0)
    return GAN(1, *SPATIAL[dims], dimensions=len(SPATIAL[dims]), n_unet_blocks=2, **kw)


@functools.lru_cache(maxsize=None)
def _batch(dims):
    g = torch.Generator().manual_seed(5)
    return {k: (torch.rand(2, 1, *SPATIAL[dims], generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}


def _fit(dims, aug_seed=None, **kw):
    m = _gan(dims, **kw)
    if aug_seed is not None:
        m.aug_generator = torch.Generator(device="cuda").manual_seed(aug_seed)
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
    m, log, _ = _fit(dims, edge_weight=0.5)
    assert set(log) == BASE_LOG | {"g_edge_loss"}
    assert 0.0 < float(log["g_edge_loss"]) < 2.0
    # the logged term is the loss of the generator's output (kept by training_step) against the target
    direct = losses.edge_loss(m.generated_imgs.detach(), _batch(dims)["t2w"])
    assert torch.equal(direct, log["g_edge_loss"])
    _sum_within_two_ulps(log["g_loss"], [float(log["g_adv_loss"]), float(log["g_recon_loss"]),
                                         0.5 * float(log["g_edge_loss"])])
    flat = m.generator.store.flat_grad
    assert bool(torch.isfinite(flat).all())
    base, _, _ = _fit(dims)                                        # the same seed, batch and weights without the term
    assert not torch.equal(flat, base.generator.store.flat_grad)


def test_edge_eps_reaches_the_loss():
    m, log, _ = _fit("2d", edge_weight=0.5, edge_eps=1e-2)
    direct = losses.edge_loss(m.generated_imgs.detach(), _batch("2d")["t2w"], eps=1e-2)
    assert torch.equal(direct, log["g_edge_loss"])
    assert not torch.equal(direct, losses.edge_loss(m.generated_imgs.detach(), _batch("2d")["t2w"]))


@pytest.mark.parametrize("dims", list(SPATIAL))
def test_validation_step_logs_the_term_and_touches_no_state(dims):
    m, _, opts = _fit(dims, edge_weight=0.5)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt_before = [(o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_count) for o in opts]
    grads_before = [net.store.flat_grad.clone() for net in (m.generator, m.discriminator)]
    val = m.validation_step(_batch(dims), 0)
    assert "val_g_edge_loss" in val and "val_g_edge_loss" in m.logged and not val["val_g_edge_loss"].requires_grad
    _sum_within_two_ulps(val["val_g_loss"], [float(val["val_g_adv_loss"]), float(val["val_g_recon_loss"]),
                                             0.5 * float(val["val_g_edge_loss"])])
    after = m.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    for o, (avg, avg_sq, steps) in zip(opts, opt_before):
        assert torch.equal(o.exp_avg, avg) and torch.equal(o.exp_avg_sq, avg_sq) and o.step_count == steps
    for net, grad in zip((m.generator, m.discriminator), grads_before):
        assert torch.equal(net.store.flat_grad, grad)


def test_composes_with_the_ssim_and_mutual_information_terms():
    m, log, _ = _fit("2d", edge_weight=0.5, ssim_weight=0.25, mi_weight=0.5)
    assert set(log) == BASE_LOG | {"g_edge_loss", "g_ssim_loss", "g_mi_loss"}
    want = (float(log["g_adv_loss"]) + float(log["g_recon_loss"]) + 0.5 * float(log["g_mi_loss"])
            + 0.25 * float(log["g_ssim_loss"]) + 0.5 * float(log["g_edge_loss"]))
    assert abs(float(log["g_loss"]) - want) <= 4 * 2.0 ** -23 * max(abs(want), 1.0)
    assert torch.equal(log["g_edge_loss"], losses.edge_loss(m.generated_imgs.detach(), _batch("2d")["t2w"]))
    val = m.validation_step(_batch("2d"), 0)
    assert {"val_g_edge_loss", "val_g_ssim_loss", "val_g_mi_loss"} <= set(val)
    want = (float(val["val_g_adv_loss"]) + float(val["val_g_recon_loss"]) + 0.5 * float(val["val_g_mi_loss"])
            + 0.25 * float(val["val_g_ssim_loss"]) + 0.5 * float(val["val_g_edge_loss"]))
    assert abs(float(val["val_g_loss"]) - want) <= 4 * 2.0 ** -23 * max(abs(want), 1.0)


def test_the_term_sees_the_warped_pair_and_never_the_discriminators_augmentation():
    from mpgan_amd import augment as A
    options = dict(rotate=0.4, scale=0.15, shift=0.1, flip=(0, 1), noise_std=0.1, mode="constant", fill=-1.0)
    m, log, _ = _fit("2d", aug_seed=11, edge_weight=0.5, pair_augment=options, diff_augment="color,translation,cutout",
                     diff_augment_fill=-1.0)
    batch, mod = _batch("2d"), m.pair_augment
    p, field = mod.last_params, mod.last_noise
    _, t2 = A.affine_warp(batch["t1w"], p.theta, batch["t2w"], mode=mod.mode, fill=mod.fill,
                          noise=None if field is None else field[0], sigma=None if field is None else p.sigma)
    assert not torch.equal(t2, batch["t2w"])
    # generated_imgs is G of the warped input, before DiffAugment; the target is the warped T2
    assert torch.equal(log["g_edge_loss"], losses.edge_loss(m.generated_imgs.detach(), t2))
    assert not torch.equal(log["g_edge_loss"], losses.edge_loss(m.generated_imgs.detach(), batch["t2w"]))


@pytest.mark.parametrize("dims", list(SPATIAL))
def test_default_trainer_is_unchanged_and_the_option_adds_no_key(dims):
    base, log0, _ = _fit(dims)
    zero, log1, _ = _fit(dims, edge_weight=0.0)
    assert set(log0) == BASE_LOG == set(log1)
    for k in log0:
        assert torch.equal(log0[k], log1[k]), k
    assert torch.equal(base.generator.store.flat_grad, zero.generator.store.flat_grad)
    for a, b in ((base.generator, zero.generator), (base.discriminator, zero.discriminator)):
        assert torch.equal(a.store.flat, b.store.flat)
    assert "val_g_edge_loss" not in base.validation_step(_batch(dims), 0)
    assert base.edge_loss is None and zero.edge_loss is None
    assert not any(isinstance(mod, losses.EdgeLoss) for mod in base.modules())
    on = _gan(dims, edge_weight=0.5)
    assert isinstance(on.edge_loss, losses.EdgeLoss) and on.edge_weight == 0.5
    assert list(on.state_dict()) == list(base.state_dict())
