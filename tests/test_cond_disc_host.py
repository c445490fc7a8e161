"""Host checks of the conditional discriminator (no GPU): the float64 restatement of tests/cond_disc_ref.py against the
oracle's unconditional discriminator, its bf16-storage restatement against the oracle's, and the argument errors
Discriminator / GAN raise before the HIP library is touched."""
import pytest
import torch

import cond_disc_ref as R


def _pair(spatial):
    """The oracle's discriminator and the conditional restatement carrying its conv1 as weight[:, 0], weight[:, 1] = 0."""
    from oracle import refmodel as O
    plain = O.Discriminator((1, *spatial), dimensions=len(spatial))
    O.closed_form_fill_(plain)
    cond_d = R.CondDiscriminator(spatial)
    sd = {k: v.clone() for k, v in plain.state_dict().items()}
    w = torch.zeros_like(cond_d.model_conv[0].weight)
    w[:, :1] = sd["model_conv.0.weight"]
    sd["model_conv.0.weight"] = w
    cond_d.load_state_dict(sd)
    return plain, cond_d


@pytest.mark.parametrize("spatial", [(20, 22), (20, 20, 21)], ids=str)
def test_zero_condition_weight_equals_the_oracle_discriminator(spatial):
    plain, cond_d = _pair(spatial)
    plain, cond_d = plain.double().train(), cond_d.double().train()
    gen = torch.Generator().manual_seed(3)
    img = (torch.rand(2, 1, *spatial, generator=gen) * 2 - 1).double()
    cond = (torch.rand(2, 1, *spatial, generator=gen) * 2 - 1).double()
    x1, x2 = img.clone().requires_grad_(True), img.clone().requires_grad_(True)
    a, b = plain(x1), cond_d(x2, cond)
    assert a.shape == b.shape == (2, 1)
    torch.testing.assert_close(b, a, rtol=1e-12, atol=1e-14)
    a.sum().backward()
    b.sum().backward()
    torch.testing.assert_close(x2.grad, x1.grad, rtol=1e-10, atol=1e-14)
    for k, v in plain.state_dict().items():
        if "running_" in k:
            torch.testing.assert_close(cond_d.state_dict()[k], v, rtol=1e-12, atol=1e-14)


def test_bf16_restatement_equals_the_oracles_on_the_unconditional_network():
    """cond_disc_ref.bf16_step states oracle/bf16_emul.disc_step's contract for two input channels and either head: on
    the same network (a zero condition weight) the two give the same numbers."""
    from oracle import bf16_emul as E
    spatial = (20, 22)
    plain, cond_d = _pair(spatial)
    gen = torch.Generator().manual_seed(4)
    img, cond = torch.rand(2, 1, *spatial, generator=gen) * 2 - 1, torch.rand(2, 1, *spatial, generator=gen)
    want = E.disc_step(plain.train(), img, 0.9)
    got = R.bf16_step(cond_d.train(), torch.cat([img, cond], 1), 0.9)
    torch.testing.assert_close(got["validity"], want["validity"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(got["loss"], want["loss"], rtol=1e-5, atol=1e-6)
    for a, b in zip(got["zs"][1:], want["zs"][1:]):
        assert ((a - b).norm() / b.norm()).item() <= 1e-3        # (bf16 ties: a few elements one ulp apart)
    rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-30)).item()
    assert rel(got["grads"]["model_linear.1.weight"], want["grads"]["model_linear.1.weight"]) <= 1e-3
    assert rel(got["grads"]["model_conv.0.weight"][:, :1], want["grads"]["model_conv.0.weight"]) <= 5e-2
    assert rel(got["grad_x"][:, :1], want["grad_x"]) <= 5e-2


def test_markovian_restatement_has_the_modules_keys():
    from mpgan_amd.networks import Discriminator
    for head in ("linear", "markovian"):
        ours = Discriminator((1, 32, 32), dimensions=2, head=head, conditional=True)
        ref = R.CondDiscriminator((32, 32), head=head)
        assert list(ours.state_dict()) == list(ref.state_dict())
        assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        plain = Discriminator((1, 32, 32), dimensions=2, head=head)
        assert list(plain.state_dict()) == list(ours.state_dict())          # only conv1's weight shape differs
        diff = [k for k, v in plain.state_dict().items() if v.shape != ours.state_dict()[k].shape]
        assert diff == ["model_conv.0.weight"] and ours.state_dict()[diff[0]].shape[1] == 2


def test_argument_errors_come_before_the_library():
    """The ValueErrors of forward: a missing condition, one given to an unconditional D, one that requires grad, one of
    another shape -- on CPU tensors, where anything later would fail for another reason."""
    from mpgan_amd.networks import Discriminator
    img, cond = torch.zeros(2, 1, 32, 32), torch.zeros(2, 1, 32, 32)
    d = Discriminator((1, 32, 32), dimensions=2, conditional=True)
    with pytest.raises(ValueError, match="needs the condition"):
        d(img)
    with pytest.raises(ValueError, match="no gradient"):
        d(img, cond.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="must match img"):
        d(img, torch.zeros(2, 1, 32, 31))
    with pytest.raises(ValueError, match="unconditional"):
        Discriminator((1, 32, 32), dimensions=2)(img, cond)
    for mode in (True, False):                                 # the same in eval mode
        d.train(mode)
        with pytest.raises(ValueError, match="needs the condition"):
            d(img)


def test_gan_hparams_list_conditional_only_when_set():
    from mpgan_amd.gan import GAN
    plain = GAN(1, 32, 32, dimensions=2, device="cpu", n_unet_blocks=1)
    assert "conditional" not in vars(plain.hparams) and plain.hparams.conditional is False
    assert plain.discriminator.model_conv[0].in_channels == 1
    cond = GAN(1, 32, 32, dimensions=2, device="cpu", n_unet_blocks=1, conditional=True, d_head="markovian", adv_loss="lsgan")
    assert vars(cond.hparams)["conditional"] is True and cond.discriminator.conditional
    assert cond.discriminator.model_conv[0].in_channels == 2 and cond.discriminator.output == "logit"
