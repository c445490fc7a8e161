"""The trainer's opt-in foreground SSIM term (variant A, GAN(..., fg_ssim_weight=...)) at the smallest 2-D shape the
trainer tests use: what it logs, its place in g_loss, that validation_step touches no state, that it composes with
fg_weight, ssim_weight and pair_augment, and that with the default 0 the trainer is bit for bit what it is without the
keyword."""
import functools

import numpy as np
import pytest
import torch

from mpgan_amd import losses
from mpgan_amd.gan import scalar_axpby

pytestmark = pytest.mark.gpu

SPATIAL = (64, 64)
BASE_LOG = {"g_adv_loss", "g_recon_loss", "g_loss", "d_loss"}


def _gan(**kw):
    from mpgan_amd.gan import GAN
    torch.manual_seed(0)
    return GAN(1, *SPATIAL, dimensions=2, n_unet_blocks=2, **kw)


@functools.lru_cache(maxsize=None)
def _batch():
    """A head-like pair: a blob of tissue values on a background at -1, so that Otsu has two classes to part."""
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, SPATIAL[0]), torch.linspace(-1, 1, SPATIAL[1]), indexing="ij")
    inside = ((yy / 0.6) ** 2 + (xx / 0.45) ** 2 < 1.0)[None, None]
    out = {}
    for k in ("t1w", "t2w"):
        tissue = torch.rand(2, 1, *SPATIAL, generator=g) * 0.8 + 0.1
        out[k] = torch.where(inside, tissue, torch.full_like(tissue, -1.0)).cuda()
    return out


def _fit(aug_seed=None, **kw):
    m = _gan(**kw)
    if aug_seed is not None:
        m.aug_generator = torch.Generator(device="cuda").manual_seed(aug_seed)
    opts, _ = m.configure_optimizers()
    log = {k: v.clone() for k, v in m.fit_batch(_batch(), 0, opts).items()}
    return m, log, opts


def test_zero_weight_is_the_trainer_without_the_keyword():
    base, log0, _ = _fit()
    zero, log1, _ = _fit(fg_ssim_weight=0.0, fg_threshold=0.25)
    assert set(log0) == BASE_LOG == set(log1)
    for k in log0:
        assert torch.equal(log0[k], log1[k]), k
    assert list(zero.state_dict()) == list(base.state_dict())
    assert torch.equal(base.generator.store.flat_grad, zero.generator.store.flat_grad)
    for a, b in ((base.generator, zero.generator), (base.discriminator, zero.discriminator)):
        assert torch.equal(a.store.flat, b.store.flat)                  # the weights after the step
    assert zero.fg_ssim_loss is None and not any(isinstance(mod, losses.ForegroundSSIMLoss) for mod in zero.modules())
    assert [name for name, _, _ in zero._generator_terms] == []
    assert vars(zero.hparams) == vars(base.hparams) and not hasattr(zero.hparams, "fg_ssim_weight")
    assert "val_g_fg_ssim_loss" not in zero.validation_step(_batch(), 0)
    on = _gan(fg_ssim_weight=0.5)
    assert isinstance(on.fg_ssim_loss, losses.ForegroundSSIMLoss) and on.fg_ssim_weight == 0.5
    assert list(on.state_dict()) == list(base.state_dict())        # the option adds no key


def test_weight_adds_the_logged_term_to_g_loss():
    m, log, _ = _fit(fg_ssim_weight=0.5)
    assert set(log) == BASE_LOG | {"g_fg_ssim_loss"}
    t2w = _batch()["t2w"]
    direct = losses.ForegroundSSIMLoss()(m.generated_imgs.detach(), t2w)
    assert torch.equal(direct, log["g_fg_ssim_loss"]) and 0.0 < float(direct) < 2.0
    # the term scores the tissue alone: it differs from the whole-image SSIM loss, which the air pulls towards 0
    whole = losses.SSIMLoss((-1.0, 1.0))(m.generated_imgs.detach(), t2w)
    assert not torch.equal(direct, whole)
    # g_loss: the parent's sum, then 0.5 * g_fg_ssim_loss through scalar_axpby's arithmetic
    parent = scalar_axpby(log["g_adv_loss"], 1.0, log["g_recon_loss"], 1.0)
    assert torch.equal(scalar_axpby(parent, 1.0, log["g_fg_ssim_loss"], 0.5), log["g_loss"])
    flat = m.generator.store.flat_grad
    assert bool(torch.isfinite(flat).all())
    base, _, _ = _fit()
    assert not torch.equal(flat, base.generator.store.flat_grad)
    # a number as the threshold reaches the loss
    m2, log2, _ = _fit(fg_ssim_weight=0.5, fg_threshold=0.5)
    assert torch.equal(log2["g_fg_ssim_loss"], losses.ForegroundSSIMLoss(0.5)(m2.generated_imgs.detach(), t2w))
    assert not torch.equal(log2["g_fg_ssim_loss"], log["g_fg_ssim_loss"])


def test_validation_step_logs_the_term_and_touches_no_state():
    m, _, opts = _fit(fg_ssim_weight=0.5)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt_before = [(o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_count) for o in opts]
    grads_before = [net.store.flat_grad.clone() for net in (m.generator, m.discriminator)]
    val = m.validation_step(_batch(), 0)
    assert "val_g_fg_ssim_loss" in val and "val_g_fg_ssim_loss" in m.logged
    assert not val["val_g_fg_ssim_loss"].requires_grad
    parent = scalar_axpby(val["val_g_adv_loss"], 1.0, val["val_g_recon_loss"], 1.0)
    assert torch.equal(scalar_axpby(parent, 1.0, val["val_g_fg_ssim_loss"], 0.5), val["val_g_loss"])
    after = m.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    for o, (avg, avg_sq, steps) in zip(opts, opt_before):
        assert torch.equal(o.exp_avg, avg) and torch.equal(o.exp_avg_sq, avg_sq) and o.step_count == steps
    for net, grad in zip((m.generator, m.discriminator), grads_before):
        assert torch.equal(net.store.flat_grad, grad)


def test_composes_with_the_other_terms_and_the_paired_augmentation():
    from mpgan_amd import augment as A
    options = dict(rotate=0.4, scale=0.15, shift=0.1, flip=(0, 1), mode="constant", fill=-1.0)
    m, log, _ = _fit(aug_seed=11, fg_ssim_weight=0.5, fg_weight=0.75, ssim_weight=0.25, pair_augment=options)
    assert set(log) == BASE_LOG | {"g_fg_ssim_loss", "g_fg_loss", "g_ssim_loss"}
    batch, mod = _batch(), m.pair_augment
    _, t2 = A.affine_warp(batch["t1w"], mod.last_params.theta, batch["t2w"], mode=mod.mode, fill=mod.fill)
    assert not torch.equal(t2, batch["t2w"])
    # like every generator term it sees the pair fit_batch hands over: the warped target
    fake = m.generated_imgs.detach()
    assert torch.equal(log["g_fg_ssim_loss"], losses.ForegroundSSIMLoss()(fake, t2))
    assert torch.equal(log["g_fg_loss"], losses.ForegroundL1Loss()(fake, t2))
    assert torch.equal(log["g_ssim_loss"], losses.SSIMLoss((-1.0, 1.0))(fake, t2))
    g = scalar_axpby(log["g_adv_loss"], 1.0, log["g_recon_loss"], 1.0)
    g = scalar_axpby(g, 1.0, log["g_ssim_loss"], 0.25)                # the list's order: ssim, fg, then fg_ssim
    g = scalar_axpby(g, 1.0, log["g_fg_loss"], 0.75)
    assert torch.equal(scalar_axpby(g, 1.0, log["g_fg_ssim_loss"], 0.5), log["g_loss"])
    want = (float(log["g_adv_loss"]) + float(log["g_recon_loss"]) + 0.25 * float(log["g_ssim_loss"])
            + 0.75 * float(log["g_fg_loss"]) + 0.5 * float(log["g_fg_ssim_loss"]))
    assert abs(float(log["g_loss"]) - want) <= 4 * 2.0 ** -23 * max(abs(want), 1.0)
    assert np.isfinite(float(log["d_loss"]))
