"""GAN(pair_augment=dict(elastic=..., bias_field=..., gamma=...)) (variant A): fit_batch deforms the
training pair once, under draws that a second generator with the same seed reproduces, and both steps train on that
pair -- the logged losses and the updated weights are those of a GAN without the option that is fed deform_warp of the
batch; t2w gets the spatial map and no intensity change; validation_step never augments."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL_GEN = dict(n_unet_blocks=1, unet_channels=(16, 32), unet_strides=(2,))
CASES = {
    "2d": (dict(args=(1, 32, 32), dimensions=2, n_unet_blocks=1), (2, 1, 32, 32)),
    "3d-markovian-conditional-lsgan-bf16": (dict(args=(1, 26, 26, 26), dimensions=3, d_head="markovian", conditional=True,
                                                 adv_loss="lsgan", storage_dtype="bf16", **SMALL_GEN), (1, 1, 26, 26, 26)),
}
OPTIONS = dict(rotate=0.3, elastic=0.3, bias_field=0.3, gamma=0.3, noise_std=0.05)


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


@pytest.mark.parametrize("cid", list(CASES))
def test_fit_batch_trains_on_the_deformed_pair(cid):
    from mpgan_amd import augment as A
    gan, batch = _make(cid, pair_augment=OPTIONS)
    module = gan.pair_augment
    assert isinstance(module, A.PairAugment) and gan.hparams.pair_augment == OPTIONS and module.deforms
    gan.aug_generator = torch.Generator(device="cuda").manual_seed(11)
    kept = {k: v.clone() for k, v in batch.items()}
    logs = _fit(gan, batch)
    assert all(torch.equal(batch[k], kept[k]) for k in batch)           # the caller's batch is untouched
    # the draws replay from the seed, in the documented order: the affine parameters, the lattices, the noise field
    replay = torch.Generator(device="cuda").manual_seed(11)
    n, spatial = batch["t1w"].shape[0], tuple(batch["t1w"].shape[2:])
    p = A.sample_affine_params(n, spatial, generator=replay, device="cuda", noise_planes=[0], **module.options)
    q = A.sample_deform_params(n, spatial, generator=replay, device="cuda", intensity_planes=[0], **module.deform_options)
    field = torch.randn((1, *batch["t1w"].shape), generator=replay, device="cuda")
    assert torch.equal(p.theta, module.last_params.theta) and torch.equal(p.sigma, module.last_params.sigma)
    assert all(torch.equal(a, b) for a, b in zip(q, module.last_deform)) and torch.equal(field, module.last_noise)
    assert q.ctrl.shape == (n, len(spatial), *[6] * len(spatial)) and q.gain.shape == (n, *[4] * len(spatial))
    assert bool(q.ctrl.any()) and bool(q.gain.any()) and bool((q.gamma[:, 0] != 1.0).all()) and bool((q.gamma[:, 1] == 1.0).all())
    t1, t2 = A.deform_warp(batch["t1w"], p.theta, batch["t2w"], ctrl=q.ctrl, gain=q.gain, gamma=q.gamma, noise=field[0],
                           sigma=p.sigma)
    assert not torch.equal(t1, batch["t1w"]) and not torch.equal(t2, batch["t2w"])
    # t2w: the spatial map and no intensity change -- the warp without gain and gamma; t1w is not that warp
    spatial_only = A.deform_warp(batch["t1w"], p.theta, batch["t2w"], ctrl=q.ctrl, noise=field[0], sigma=p.sigma)
    assert torch.equal(_bits(t2), _bits(spatial_only[1])) and not torch.equal(t1, spatial_only[0])
    assert not torch.equal(t2, A.affine_warp(batch["t2w"], p.theta))    # the lattice moved it
    plain, _ = _make(cid)
    assert plain.pair_augment is None
    _same_run(gan, logs, plain, _fit(plain, {"t1w": t1, "t2w": t2}))


@pytest.mark.parametrize("cid", list(CASES))
def test_validation_never_deforms(cid, monkeypatch):
    from mpgan_amd import augment as A
    from mpgan_amd import ops
    gan, batch = _make(cid, pair_augment=OPTIONS)

    def refuse(*a, **k):
        raise AssertionError("a step augmented the pair on its own")

    for name in ("affine_warp", "deform_warp"):
        monkeypatch.setattr(ops, name, refuse)
    for name in ("sample_affine_params", "_sample_affine", "sample_deform_params"):
        monkeypatch.setattr(A, name, refuse)
    out = gan.validation_step(batch, 0)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    assert gan.pair_augment.last_params is None and gan.pair_augment.last_deform is None
    plain, _ = _make(cid)
    want = plain.validation_step(batch, 0)
    assert set(out) == set(want) and all(torch.equal(_bits(out[k]), _bits(want[k])) for k in out)
