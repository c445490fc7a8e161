"""GAN(pair_augment=...) (variant A): fit_batch warps the training pair once, under one draw that a second
generator with the same seed reproduces, and both steps train on that pair -- the logged losses and the updated weights
are those of a GAN without the option that is fed affine_warp of the batch; training_step and validation_step never
augment; DiffAugment, when it is on too, draws after it and sees the augmented pair."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL_GEN = dict(n_unet_blocks=1, unet_channels=(16, 32), unet_strides=(2,))
CASES = {
    "2d": (dict(args=(1, 32, 32), dimensions=2, n_unet_blocks=1), (2, 1, 32, 32)),
    "3d-markovian-conditional-lsgan-bf16": (dict(args=(1, 26, 26, 26), dimensions=3, d_head="markovian", conditional=True,
                                                 adv_loss="lsgan", storage_dtype="bf16", **SMALL_GEN), (1, 1, 26, 26, 26)),
}
OPTIONS = dict(rotate=0.4, scale=0.15, shift=0.1, flip=(0, 1), noise_std=0.1, mode="constant", fill=-1.0)
POLICY = "color,translation,cutout"


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


def _fit(gan, batch, steps=1):
    opts, _ = gan.configure_optimizers()
    return [gan.fit_batch(batch, i, opts) for i in range(steps)]


def _same_run(a, logs_a, b, logs_b):
    for la, lb in zip(logs_a, logs_b):
        assert set(la) == set(lb) == {"g_adv_loss", "g_recon_loss", "g_loss", "d_loss"}
        for k in la:
            assert torch.equal(_bits(la[k]), _bits(lb[k])), k
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


def _warped(batch, module):
    from mpgan_amd import augment as A
    p, field = module.last_params, module.last_noise
    t1, t2 = A.affine_warp(batch["t1w"], p.theta, batch["t2w"], mode=module.mode, fill=module.fill,
                           noise=None if field is None else field[0], sigma=None if field is None else p.sigma)
    return {"t1w": t1, "t2w": t2}


@pytest.mark.parametrize("cid", list(CASES))
def test_fit_batch_trains_on_the_warped_pair(cid):
    from mpgan_amd import augment as A
    gan, batch = _make(cid, pair_augment=OPTIONS)
    assert isinstance(gan.pair_augment, A.PairAugment) and gan.hparams.pair_augment == OPTIONS
    gan.aug_generator = torch.Generator(device="cuda").manual_seed(11)
    kept = {k: v.clone() for k, v in batch.items()}
    logs = _fit(gan, batch)
    assert all(torch.equal(batch[k], kept[k]) for k in batch)           # the caller's batch is untouched
    # the draw replays from the seed, in the documented order: the parameters, then the noise field
    replay = torch.Generator(device="cuda").manual_seed(11)
    n, spatial = batch["t1w"].shape[0], tuple(batch["t1w"].shape[2:])
    p = A.sample_affine_params(n, spatial, generator=replay, device="cuda", noise_planes=[0], **gan.pair_augment.options)
    field = torch.randn((1, *batch["t1w"].shape), generator=replay, device="cuda")
    last = gan.pair_augment.last_params
    assert torch.equal(p.theta, last.theta) and torch.equal(p.sigma, last.sigma) and torch.equal(field, gan.pair_augment.last_noise)
    eye = torch.eye(3, 4, dtype=torch.float64, device="cuda").reshape(1, 12)
    assert not bool((last.theta == eye).all(1).any()) and bool((last.sigma[:, 0] > 0).all())
    warped = _warped(batch, gan.pair_augment)
    assert not torch.equal(warped["t1w"], batch["t1w"]) and not torch.equal(warped["t2w"], batch["t2w"])
    plain, _ = _make(cid)
    assert plain.pair_augment is None
    _same_run(gan, logs, plain, _fit(plain, warped))


@pytest.mark.parametrize("cid", list(CASES))
def test_a_gated_off_module_is_no_option_at_all(cid):
    gan, batch = _make(cid, pair_augment=dict(rotate=0.4, flip=(0,), prob=0.0, noise_std=0.0))
    gan.aug_generator = torch.Generator(device="cuda").manual_seed(11)
    state = gan.aug_generator.get_state()
    logs = _fit(gan, batch, 2)
    assert torch.equal(gan.aug_generator.get_state(), state)            # nothing was drawn
    assert gan.pair_augment.last_noise is None
    plain, _ = _make(cid)
    _same_run(gan, logs, plain, _fit(plain, batch, 2))


@pytest.mark.parametrize("cid", list(CASES))
def test_the_steps_themselves_never_augment(cid, monkeypatch):
    from mpgan_amd import augment as A
    from mpgan_amd import ops
    gan, batch = _make(cid, pair_augment=OPTIONS)

    def refuse(*a, **k):
        raise AssertionError("a step augmented the pair on its own")

    monkeypatch.setattr(ops, "affine_warp", refuse)
    monkeypatch.setattr(A, "sample_affine_params", refuse)
    out = gan.validation_step(batch, 0)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    for p in gan.discriminator.parameters():
        p.requires_grad_(False)
    assert bool(torch.isfinite(gan.training_step(batch, 0, 0)))
    for p in gan.discriminator.parameters():
        p.requires_grad_(True)
    assert bool(torch.isfinite(gan.training_step(batch, 0, 1)))
    assert gan.pair_augment.last_params is None
    # a default GAN: no module anywhere, and fit_batch launches nothing of it
    plain, _ = _make(cid)
    assert plain.pair_augment is None and "pair_augment" not in vars(plain.hparams)
    assert not any(isinstance(m, A.PairAugment) for m in plain.modules())
    log = _fit(plain, batch)[0]
    assert all(bool(torch.isfinite(v).all()) for v in log.values())


@pytest.mark.parametrize("cid", list(CASES))
def test_diff_augment_sees_the_augmented_pair_and_draws_after_it(cid):
    from mpgan_amd import augment as A
    gan, batch = _make(cid, pair_augment=OPTIONS, diff_augment=POLICY, diff_augment_fill=-1.0)
    gan.aug_generator = torch.Generator(device="cuda").manual_seed(13)
    judged, fed = [], []
    judge, forward = gan._judge, gan.discriminator.forward

    def spy_judge(images, t1w_images, augment=False):
        judged.append((images, t1w_images, augment))
        return judge(images, t1w_images, augment=augment)

    def spy_forward(img, cond=None):
        fed.append((img, cond))
        return forward(img, cond)

    gan._judge, gan.discriminator.forward = spy_judge, spy_forward
    log = _fit(gan, batch)[0]
    assert all(bool(torch.isfinite(v).all()) for v in log.values())
    assert len(judged) == len(fed) == 3                                 # G step fake, D step real, D step fake
    warped = _warped(batch, gan.pair_augment)
    replay = torch.Generator(device="cuda").manual_seed(13)
    n, spatial = batch["t1w"].shape[0], tuple(batch["t1w"].shape[2:])
    p = A.sample_affine_params(n, spatial, generator=replay, device="cuda", noise_planes=[0], **gan.pair_augment.options)
    torch.randn((1, *batch["t1w"].shape), generator=replay, device="cuda")
    assert torch.equal(p.theta, gan.pair_augment.last_params.theta)
    assert torch.equal(_bits(judged[1][0]), _bits(warped["t2w"]))       # the real pass judges the warped t2w
    for (images, t1w, flag), (img, cond) in zip(judged, fed):
        assert flag and torch.equal(_bits(t1w), _bits(warped["t1w"]))
        q = A.sample_params(n, spatial, POLICY, generator=replay, device="cuda")
        assert torch.equal(_bits(img), _bits(A.diff_augment(images.detach(), q, fill=-1.0)))
        if gan.hparams.conditional:
            assert torch.equal(_bits(cond), _bits(A.diff_augment(warped["t1w"], q, color=False, fill=-1.0)))
