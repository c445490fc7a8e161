"""GAN(ema_decay=..., grad_clip=..., log_grad_norm=...) and FusedAdam's options (variant A): a default GAN
launches and names nothing new; the averaged generator follows the fp64 recurrence of the live weights and buffers, is
evaluated from fresh packs, takes no gradient and round-trips through checkpoints; clipping steps by the fp64 clipped
Adam; the norms are logged as snapshots; validation_step scores the averaged generator and touches nothing."""
import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

POLICY = "color,translation,cutout"
SMALL_GEN = dict(n_unet_blocks=1, unet_channels=(16, 32), unet_strides=(2,))
CASES = {
    "2d": (dict(args=(1, 32, 32), dimensions=2, n_unet_blocks=1), (2, 1, 32, 32)),
    "3d-markovian-conditional-lsgan-bf16": (dict(args=(1, 26, 26, 26), dimensions=3, d_head="markovian", conditional=True,
                                                 adv_loss="lsgan", storage_dtype="bf16", **SMALL_GEN), (1, 1, 26, 26, 26)),
}
NEW_HPARAMS = ("ema_decay", "ema_warmup", "grad_clip", "log_grad_norm")
BASE_LOGGED = {"g_adv_loss", "g_recon_loss", "g_loss", "d_loss"}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _make(cid, **kw):
    from mpgan_amd.gan import GAN
    cfg, shape = CASES[cid]
    cfg = dict(cfg)
    args = cfg.pop("args")
    torch.manual_seed(0)
    gan = GAN(*args, **cfg, **kw)
    g = torch.Generator().manual_seed(5)
    batch = {k: (torch.rand(*shape, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}
    return gan, batch


def _float_buffers(net):
    return [b for b in net.buffers() if b.dtype.is_floating_point]


def _int_buffers(net):
    return [b for b in net.buffers() if not b.dtype.is_floating_point]


def _record_g_steps(opt_g, net):
    """The live buffers as opt_g.step() saw them (the D step's generator pass moves the running statistics again, so a
    snapshot after fit_batch is one update ahead of what the average was fed)."""
    seen, step = [], opt_g.step

    def spy(*a, **k):
        out = step(*a, **k)
        seen.append(([b.detach().clone() for b in _float_buffers(net)], [b.detach().clone() for b in _int_buffers(net)]))
        return out

    opt_g.step = spy
    return seen


def _within(got, want64, scale, steps):
    err = (got.cpu().double() - want64.cpu()).abs()
    bound = R.ema_bound(scale.cpu(), scale.cpu(), steps=steps)
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("cid", list(CASES))
def test_a_default_gan_launches_and_names_nothing_new(cid, monkeypatch):
    from mpgan_amd import ops
    gan, batch = _make(cid)

    def refuse(*a, **k):
        raise AssertionError("a default GAN launched an optimiser extra")

    for name in ("grad_norm", "adam_step_ex", "ema_buffers"):
        monkeypatch.setattr(ops, name, refuse)
    opts, _ = gan.configure_optimizers()
    for i in range(2):
        log = gan.fit_batch(batch, i, opts)
        assert set(log) == BASE_LOGGED
    assert not set(NEW_HPARAMS) & set(vars(gan.hparams))
    assert gan.generator_ema is None and opts[0].grad_norm is None and opts[1].grad_norm is None
    assert not [k for k in gan.state_dict() if "ema" in k]
    assert [n for n, _ in gan.named_children()] == ["generator", "discriminator"]
    assert (gan.hparams.ema_decay, gan.hparams.ema_warmup, gan.hparams.grad_clip, gan.hparams.log_grad_norm) == \
        (0.0, True, 0.0, False)


def test_the_average_follows_the_recurrence_and_is_evaluated_from_fresh_packs():
    from mpgan_amd.networks import CasNetGenerator
    gan, batch = _make("2d", ema_decay=0.9, ema_warmup=False)
    assert vars(gan.hparams)["ema_decay"] == 0.9 and vars(gan.hparams)["ema_warmup"] is False
    assert "grad_clip" not in vars(gan.hparams)
    twin, live = gan.generator_ema, gan.generator
    assert not twin.training and not any(p.requires_grad for p in twin.parameters())
    assert any(k.startswith("generator_ema.") for k in gan.state_dict())
    with torch.no_grad():
        y_init = twin(batch["t1w"])                              # packs the twin's initial weights
        assert torch.equal(_bits(y_init), _bits(live.eval()(batch["t1w"])))
    gan.train()
    assert live.training and not twin.training                   # the average is only ever evaluated
    assert torch.equal(_bits(twin.store.flat), _bits(live.store.flat))
    w = float(np.float32(1.0 - 0.9))
    e64 = twin.store.flat.double()
    b64 = [b.double() for b in _float_buffers(twin)]
    scale, bscale = e64.abs(), [b.abs() for b in b64]
    opts, _ = gan.configure_optimizers()
    seen = _record_g_steps(opts[0], live)
    for i in range(3):
        gan.fit_batch(batch, i, opts)
        p = live.store.flat.double()
        e64 = R.lerp(e64, p, w)
        scale = torch.maximum(scale, torch.maximum(p.abs(), e64.abs()))
        fbufs, ibufs = seen[i]
        b64 = [R.lerp(b, s.double(), w) for b, s in zip(b64, fbufs)]
        bscale = [torch.maximum(m, torch.maximum(s.abs().double(), b.abs())) for m, s, b in zip(bscale, fbufs, b64)]
    assert len(seen) == 3 and fbufs
    _within(twin.store.flat, e64, scale, steps=3)
    assert not torch.equal(_bits(twin.store.flat), _bits(live.store.flat))
    for got, want, m in zip(_float_buffers(twin), b64, bscale):
        _within(got, want, m, steps=3)
    assert ibufs and all(torch.equal(a, b) for a, b in zip(_int_buffers(twin), ibufs))
    assert all(int(b) == 5 for b in ibufs)                       # the third G step: 2 passes per fit_batch, then one
    assert all(p.grad is None for p in twin.parameters())
    # the stale-pack check: what the twin computes is what a fresh module loaded from its state_dict computes
    fresh = CasNetGenerator((1, 32, 32), 1, dimensions=2, device="cuda").eval()
    fresh.load_state_dict(twin.state_dict())
    with torch.no_grad():
        y_twin, y_fresh = twin(batch["t1w"]), fresh(batch["t1w"])
    assert torch.equal(_bits(y_twin), _bits(y_fresh))
    assert not torch.equal(_bits(y_twin), _bits(y_init))


def test_warm_up_starts_the_average_at_a_decay_of_one_tenth():
    gan, batch = _make("2d", ema_decay=0.9)
    assert "ema_warmup" not in vars(gan.hparams)
    init = gan.generator_ema.store.flat.double()
    opts, _ = gan.configure_optimizers()
    gan.fit_batch(batch, 0, opts)
    p1 = gan.generator.store.flat.double()
    want = R.lerp(init, p1, float(np.float32(1.0 - 0.1)))
    _within(gan.generator_ema.store.flat, want, torch.maximum(init.abs(), p1.abs()), steps=1)
    assert float((want - init).abs().max()) > 0


def test_clipping_steps_by_the_clipped_adam():
    from mpgan_amd.gan import FusedAdam
    gan, batch = _make("2d")
    net, h = gan.generator, gan.hparams
    for p in gan.discriminator.parameters():                     # the G step of fit_batch, by hand
        p.requires_grad_(False)
    FusedAdam(net).zero_grad()
    gan.training_step(batch, 0, 0).backward()
    g = net.store.flat_grad.detach().clone().cpu()
    p0 = net.store.flat.detach().clone().cpu()
    ref_norm = R.grad_norm(g, 1.0)
    assert ref_norm > 0
    opt = FusedAdam(net, lr=h.g_lr, betas=(h.b1, h.b2), max_grad_norm=0.1 * ref_norm)
    opt.step()
    got = float(opt.grad_norm)
    print(f"norm {got!r} ref {ref_norm!r}")
    assert opt.grad_norm.is_cuda and opt.grad_norm.dim() == 0
    assert abs(got - float(np.float32(ref_norm))) <= R.ulp32(ref_norm)
    coef = R.clip_coef(ref_norm, 0.1 * ref_norm)
    zeros = torch.zeros_like(p0, dtype=torch.float64)
    p64, m64, v64 = R.adam_step_coef(p0.double(), g.double(), zeros, zeros, h.g_lr, h.b1, h.b2, 1e-8, 1, coef=coef)
    for name, a, b in (("p", net.store.flat, p64), ("m", opt.exp_avg, m64), ("v", opt.exp_avg_sq, v64)):
        err = (a.cpu().double() - b).abs()
        assert bool((err <= 1e-7 + 1e-6 * b.abs()).all()), (name, float(err.max()))
    assert torch.equal(net.store.flat_grad.cpu(), g)             # clipping scales on load: the buffer keeps the gradient
    # the unclipped step would have moved m ten times as far
    assert float((opt.exp_avg.cpu().double() - 10 * m64).abs().max()) > float(m64.abs().max())


@pytest.mark.parametrize("kw", [dict(grad_clip=1.0), dict(log_grad_norm=True)], ids=["clip", "measure"])
def test_fit_batch_logs_the_norms_as_snapshots(kw):
    gan, batch = _make("2d", **kw)
    assert set(kw) <= set(vars(gan.hparams)) and gan.generator_ema is None
    opts, _ = gan.configure_optimizers()
    log1 = gan.fit_batch(batch, 0, opts)
    assert set(log1) == BASE_LOGGED | {"g_grad_norm", "d_grad_norm"}
    first = {}
    for name in ("g_grad_norm", "d_grad_norm"):
        t = log1[name]
        assert t.is_cuda and t.dim() == 0 and t.dtype == torch.float32
        first[name] = float(t)
        assert np.isfinite(first[name]) and first[name] > 0
    log2 = gan.fit_batch(batch, 1, opts)
    for name, value in first.items():
        assert float(log1[name]) == value                        # not overwritten by the next step's norm
        assert float(log2[name]) != value
        assert float(log2[name]) == float(opts[("g_grad_norm", "d_grad_norm").index(name)].grad_norm)


def _everything(gan, opts):
    out = {}
    for name in ("generator", "discriminator", "generator_ema"):
        net = getattr(gan, name)
        out[name + ".flat"] = net.store.flat
        for k, b in net.named_buffers():
            out[f"{name}.{k}"] = b
    for i, o in enumerate(opts):
        out[f"opt{i}.m"], out[f"opt{i}.v"] = o.exp_avg, o.exp_avg_sq
    return out


def test_validation_step_scores_the_average_and_touches_nothing():
    from mpgan_amd.gan import reconstruction_loss
    gan, batch = _make("2d", ema_decay=0.9, ema_warmup=False)
    opts, _ = gan.configure_optimizers()
    gan.fit_batch(batch, 0, opts)
    before = {k: v.detach().clone() for k, v in _everything(gan, opts).items()}
    out = gan.validation_step(batch, 0)
    assert set(out) == {"val_g_adv_loss", "val_g_recon_loss", "val_g_loss", "val_d_loss", "val_ema_g_recon_loss"}
    assert gan.logged["val_ema_g_recon_loss"] is not None
    with torch.no_grad():
        want = reconstruction_loss(gan.generator_ema(batch["t1w"]), batch["t2w"])
    assert torch.equal(_bits(out["val_ema_g_recon_loss"]), _bits(want))
    assert float(out["val_ema_g_recon_loss"]) != float(out["val_g_recon_loss"])
    after = _everything(gan, opts)
    changed = [k for k, v in before.items() if not torch.equal(v, after[k])]
    assert not changed, changed
    assert gan.generator.training and not gan.generator_ema.training


def test_checkpoints_carry_the_average(tmp_path):
    from mpgan_amd.gan import load_reference_checkpoint
    gan, batch = _make("2d", ema_decay=0.9, ema_warmup=False)
    opts, _ = gan.configure_optimizers()
    for i in range(2):
        gan.fit_batch(batch, i, opts)
    sd = {k: v.detach().clone() for k, v in gan.state_dict().items()}
    other, _ = _make("2d", ema_decay=0.9, ema_warmup=False)
    other.load_state_dict(sd)
    assert torch.equal(_bits(other.generator_ema.store.flat), _bits(gan.generator_ema.store.flat))
    assert torch.equal(_bits(other.generator.store.flat), _bits(gan.generator.store.flat))
    plain, _ = _make("2d")
    res = plain.load_state_dict(sd, strict=False)
    assert not res.missing_keys and res.unexpected_keys and all(k.startswith("generator_ema.") for k in res.unexpected_keys)
    assert torch.equal(_bits(plain.generator.store.flat), _bits(gan.generator.store.flat))
    # a checkpoint without an average: the twin restarts from the loaded generator
    path = str(tmp_path / "plain.ckpt")
    torch.save({"state_dict": {k: v.cpu() for k, v in sd.items() if not k.startswith("generator_ema.")}}, path)
    third, _ = _make("2d", ema_decay=0.9)
    load_reference_checkpoint(third, path)
    assert torch.equal(_bits(third.generator.store.flat), _bits(gan.generator.store.flat))
    assert torch.equal(_bits(third.generator_ema.store.flat), _bits(third.generator.store.flat))
    for a, b in zip(third.generator_ema.buffers(), third.generator.buffers()):
        assert torch.equal(a, b)
    # ... and one with an average keeps it
    path2 = str(tmp_path / "ema.ckpt")
    torch.save({"state_dict": {k: v.cpu() for k, v in sd.items()}}, path2)
    fourth, _ = _make("2d", ema_decay=0.9)
    load_reference_checkpoint(fourth, path2)
    assert torch.equal(_bits(fourth.generator_ema.store.flat), _bits(gan.generator_ema.store.flat))
    gan.reset_ema()
    assert torch.equal(_bits(gan.generator_ema.store.flat), _bits(gan.generator.store.flat))


def test_3d_bf16_with_average_clipping_and_augmentation_together():
    gan, batch = _make("3d-markovian-conditional-lsgan-bf16", ema_decay=0.99, grad_clip=1.0, diff_augment=POLICY)
    gan.aug_generator = torch.Generator(device="cuda").manual_seed(11)
    init = gan.generator_ema.store.flat.double()
    opts, _ = gan.configure_optimizers()
    log = gan.fit_batch(batch, 0, opts)
    assert set(log) == BASE_LOGGED | {"g_grad_norm", "d_grad_norm"}
    assert all(bool(torch.isfinite(v).all()) for v in log.values()), log
    p1 = gan.generator.store.flat.double()
    assert bool(torch.isfinite(p1).all()) and bool(torch.isfinite(gan.discriminator.store.flat).all())
    want = R.lerp(init, p1, float(np.float32(1.0 - R.ema_decay_at(1, 0.99, True))))
    _within(gan.generator_ema.store.flat, want, torch.maximum(init.abs(), p1.abs()), steps=1)
    with torch.no_grad():
        assert bool(torch.isfinite(gan.generator_ema(batch["t1w"])).all())


def test_option_validation():
    from mpgan_amd.gan import GAN, FusedAdam
    from mpgan_amd.networks import CasNetGenerator
    with pytest.raises(ValueError):
        GAN(1, 32, 32, dimensions=2, n_unet_blocks=1, ema_decay=1.0)
    with pytest.raises(ValueError):
        GAN(1, 32, 32, dimensions=2, n_unet_blocks=1, grad_clip=-0.5)
    net = CasNetGenerator((1, 32, 32), 1, dimensions=2, device="cuda")
    wrong = CasNetGenerator((1, 32, 32), 2, dimensions=2, device="cuda")
    opt = FusedAdam(net, ema=wrong)
    before = net.store.flat.clone()
    with pytest.raises(ValueError):
        opt.step()
    assert opt.step_count == 0 and torch.equal(before, net.store.flat)
    with pytest.raises(ValueError):
        FusedAdam(net, max_grad_norm=0.0)
    with pytest.raises(ValueError):
        FusedAdam(net, ema=net)
