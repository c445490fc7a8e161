"""GAN(diff_augment="color,affine,translation,cutout") (variant A), on the two configurations of
test_diffaug_trainer_gpu.py: what the discriminator is fed in training_step is the warp, then the old augmentation, of
what the trainer judged, under parameters that a second generator with the same seed and the documented draw order
(per call: color, translation, cutout, then the affine map; G step: one draw; D step: the real pass, then the fake pass)
reproduces; a conditional discriminator's T1 input gets the same map and no gradient; the generator's gradient is the two
backward kernels' composition; validation_step never augments."""
import pytest
import torch

pytestmark = pytest.mark.gpu

POLICY = "color,affine,translation,cutout"
AFFINE = dict(rotate=0.4, scale=0.2, shift=0.05, flip=(1,))
SMALL_GEN = dict(n_unet_blocks=1, unet_channels=(16, 32), unet_strides=(2,))
CASES = {
    "2d": (dict(args=(1, 32, 32), dimensions=2, n_unet_blocks=1), (2, 1, 32, 32)),
    "3d-markovian-conditional-lsgan-bf16": (dict(args=(1, 26, 26, 26), dimensions=3, d_head="markovian", conditional=True,
                                                 adv_loss="lsgan", storage_dtype="bf16", **SMALL_GEN), (1, 1, 26, 26, 26)),
}


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


def _spy(gan):
    """Record what _judge was asked to judge and what the discriminator was fed."""
    judged, fed = [], []
    judge, forward = gan._judge, gan.discriminator.forward

    def spy_judge(images, t1w_images, augment=False):
        judged.append((images, t1w_images, augment))
        return judge(images, t1w_images, augment=augment)

    def spy_forward(img, cond=None):
        if img.requires_grad:
            img.retain_grad()
        fed.append((img, cond))
        return forward(img, cond)

    gan._judge, gan.discriminator.forward = spy_judge, spy_forward
    return judged, fed


def _two_steps(x, p, fill, color=True):
    """The documented composition from the public pieces: the constant warp, then the old kernel without the AFFINE bit."""
    from mpgan_amd import augment as A
    warped = A.affine_warp(x.detach(), p.theta, mode="constant", fill=fill)
    return A.diff_augment(warped, p._replace(ops=p.ops & ~A.AFFINE, theta=None), color=color, fill=fill)


@pytest.mark.parametrize("cid", list(CASES))
def test_discriminator_inputs_replay_from_the_seed(cid):
    from mpgan_amd import augment as A
    gan, batch = _make(cid, diff_augment=POLICY, diff_augment_fill=-1.0, diff_augment_affine=AFFINE)
    assert gan.hparams.diff_augment == POLICY and gan.hparams.diff_augment_affine == AFFINE
    assert isinstance(gan.augment, A.DiffAugment) and gan.augment.ops == 31
    gan.aug_generator = torch.Generator(device="cuda").manual_seed(11)
    replay = torch.Generator(device="cuda").manual_seed(11)
    judged, fed = _spy(gan)
    opts, _ = gan.configure_optimizers()
    before = {k: v.detach().clone() for k, v in gan.named_parameters()}
    logs = [gan.fit_batch(batch, i, opts) for i in range(2)]
    assert len(judged) == len(fed) == 6                        # per fit_batch: G step fake, D step real, D step fake
    n, spatial = batch["t1w"].shape[0], tuple(batch["t1w"].shape[2:])
    seen = []
    for (images, t1w, flag), (img, cond) in zip(judged, fed):
        assert flag and t1w is batch["t1w"]
        # the draw order, piece by piece: the three old words as before the word existed, then the map
        old = A.sample_params(n, spatial, "color,translation,cutout", generator=replay, device="cuda")
        theta = A.sample_affine_params(n, spatial, generator=replay, device="cuda", **AFFINE).theta
        p = A.DiffAugParams(old.color, old.geom, old.ops | A.AFFINE, theta)
        seen.append(p)
        assert torch.equal(_bits(img), _bits(_two_steps(images, p, -1.0)))
        assert torch.equal(_bits(img), _bits(A.diff_augment(images.detach(), p, fill=-1.0)))
        assert not torch.equal(_bits(img), _bits(A.diff_augment(images.detach(), old, fill=-1.0)))      # the warp took part
        if gan.hparams.conditional:
            assert not cond.requires_grad and cond.grad_fn is None
            assert torch.equal(_bits(cond), _bits(_two_steps(t1w, p, -1.0, color=False)))
        else:
            assert cond is None
    assert judged[1][0] is batch["t2w"] and judged[4][0] is batch["t2w"]
    assert not any(torch.equal(a.theta, b.theta) for i, a in enumerate(seen) for b in seen[:i])     # a new draw per call
    assert torch.equal(gan.augment.last_params.theta, seen[-1].theta)
    assert torch.equal(gan.augment.last_params.geom, seen[-1].geom)
    for log in logs:
        assert set(log) == {"g_adv_loss", "g_recon_loss", "g_loss", "d_loss"}
        assert all(bool(torch.isfinite(v).all()) for v in log.values()), log
    still = [k for k, v in gan.named_parameters() if torch.equal(v.detach(), before[k])]
    assert not still, still


@pytest.mark.parametrize("cid", list(CASES))
def test_generator_gradient_is_the_two_backward_kernels(cid):
    from mpgan_amd import augment as A
    from mpgan_amd import ops
    gan, batch = _make(cid, diff_augment=POLICY)
    assert gan.hparams.diff_augment_affine == A.DEFAULT_AFFINE
    gan.aug_generator = torch.Generator(device="cuda").manual_seed(12)
    judged, fed = _spy(gan)
    for p in gan.discriminator.parameters():                   # the G step of fit_batch
        p.requires_grad_(False)
    loss = gan.training_step(batch, 0, 0)
    gen = gan.generated_imgs
    assert judged[0][0] is gen and gen.requires_grad
    gen.retain_grad()
    loss.backward(retain_graph=True)
    img, cond = fed[0]
    g_in = img.grad                                            # the gradient at D's input
    assert g_in is not None and float(g_in.abs().max()) > 0
    if gan.hparams.conditional:
        assert not cond.requires_grad and batch["t1w"].grad is None
    arrived = gen.grad.clone()                                 # (the retain_grad hook fires again in the call below)
    (g_gen,) = torch.autograd.grad(img, gen, g_in)             # the graph between the two is the augmentation alone
    p = gan.augment.last_params
    ws = torch.empty(ops.diffaug_workspace(gen.shape[0], tuple(gen.shape[2:])) // 8, dtype=torch.float64, device="cuda")
    inner = ops.diffaug_backward(g_in.contiguous(), p.ops & ~A.AFFINE, p.color, p.geom, ws, torch.empty_like(g_in))
    want = ops.affine_warp_backward(inner, p.theta, ops.WARP_CONSTANT, torch.empty_like(g_in))
    assert torch.equal(_bits(g_gen), _bits(want)) and bool(torch.isfinite(want).all())
    assert not torch.equal(_bits(want), _bits(inner))          # the warp's backward took part
    # ... and what arrives at generated_imgs is that plus the reconstruction loss's own gradient (unaugmented images)
    recon = torch.sign(gen.detach() - batch["t2w"]) / gen.numel()
    assert torch.allclose(arrived, want + recon, rtol=1e-5, atol=1e-9)
    assert float((arrived - recon).abs().max()) > 0


@pytest.mark.parametrize("cid", list(CASES))
def test_validation_step_launches_nothing_of_it(cid, monkeypatch):
    from mpgan_amd import ops
    gan, batch = _make(cid, diff_augment=POLICY)

    def refuse(*a, **k):
        raise AssertionError("validation_step launched the augmentation")

    for name in ("affine_warp", "affine_warp_backward", "diffaug_forward", "diffaug_backward"):
        monkeypatch.setattr(ops, name, refuse)
    judged, fed = _spy(gan)
    out = gan.validation_step(batch, 0)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    assert len(judged) == len(fed) == 2 and not any(flag for _, _, flag in judged)
    for (images, t1w, _), (img, cond) in zip(judged, fed):
        assert torch.equal(_bits(img), _bits(images))
        if gan.hparams.conditional:
            assert torch.equal(_bits(cond), _bits(batch["t1w"]))
    assert torch.equal(_bits(fed[1][0]), _bits(batch["t2w"]))
    assert gan.augment.last_params is None


@pytest.mark.parametrize("cid", list(CASES))
def test_without_the_word_nothing_new_is_launched(cid, monkeypatch):
    from mpgan_amd import augment as A
    from mpgan_amd import ops
    gan, batch = _make(cid, diff_augment="color,translation,cutout")
    assert "diff_augment_affine" not in vars(gan.hparams) and gan.augment.affine is None

    def refuse(*a, **k):
        raise AssertionError("a GAN without the word 'affine' used the warp")

    for mod, name in ((ops, "affine_warp"), (ops, "affine_warp_backward"), (A, "sample_affine_params"),
                      (A, "diff_affine_warp")):
        monkeypatch.setattr(mod, name, refuse)
    gan.aug_generator = torch.Generator(device="cuda").manual_seed(1)
    opts, _ = gan.configure_optimizers()
    log = gan.fit_batch(batch, 0, opts)
    assert all(bool(torch.isfinite(v).all()) for v in log.values())
    assert gan.augment.last_params.theta is None and gan.augment.last_params.ops == 15
