"""Variant A's discriminator with the Markovian (PatchGAN) head behind the module and trainer API, at the smallest
inputs the head admits (last feature map 4 x 6 / 4 x 4 x 5), against the float64 restatement of tests/map_head_ref.py
loaded with the same state_dict.  Bounds and helper of the train-mode checks are those tests/test_networks_gpu.py
applies to the Linear-head discriminator at its small shapes (test_discriminator_forward_backward_matches_oracle)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import map_head_ref as M
from gpu_helpers import assert_close, from_cl
from test_networks_gpu import _check_param_grads, _pre_norm_bias

pytestmark = pytest.mark.gpu

SHAPES = {"2d": ((26, 34), (1, 3)), "3d": ((26, 26, 30), (1, 1, 2))}
N = 2


def _ref(dims):
    """The restatement with closed-form weights: fp32 values held in float64."""
    from oracle import refmodel as R
    ref = M.MarkovianDiscriminator(dims)
    R.closed_form_fill_(ref)
    return ref.double().train()


def _ours(ref, spatial, **kw):
    from mpgan_amd.networks import Discriminator
    ours = Discriminator((1, *spatial), dimensions=len(spatial), head="markovian", **kw)
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return ours.cuda().train()


def _x(spatial, seed=17):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(N, 1, *spatial, generator=gen) * 2 - 1


@pytest.mark.parametrize("which", list(SHAPES))
def test_train_mode_matches_the_restatement(which):
    from mpgan_amd.gan import adversarial_loss
    spatial, map_size = SHAPES[which]
    dims = len(spatial)
    ref = _ref(dims)
    ours = _ours(ref, spatial)
    x = _x(spatial).double().requires_grad_(True)
    acts = {}
    hooks = [ref.model_conv[i].register_forward_hook(lambda m, a, out, i=i: acts.__setitem__(i, out.detach()))
             for i in (1, 4, 7, 10)]
    p_ref = ref(x)
    for h in hooks:
        h.remove()
    loss_ref = F.binary_cross_entropy(p_ref, torch.full_like(p_ref, 0.9))
    loss_ref.backward()
    xc = x.detach().float().cuda().requires_grad_(True)
    p = ours(xc)
    assert p.shape == (N, 1, *map_size) == p_ref.shape
    assert_close(p, p_ref, rtol=1e-4, atol=1e-6, what="validity map")
    loss = adversarial_loss(p, torch.full_like(p, 0.9))
    assert_close(loss.reshape(1), loss_ref.reshape(1), rtol=1e-5, what="bce against a 0.9 map")
    loss.backward()
    # LeakyReLU kinks, counted as test_discriminator_forward_backward_matches_oracle counts them
    plan = [pl for pool in ours._plans.values() for pl in pool][0]
    assert type(plan.head).__name__ == "MapHead"
    flips = 0
    for k, i in enumerate((1, 4, 7, 10)):
        z = plan.zs[k].squeeze(1) if dims == 2 else plan.zs[k]
        a = (z * plan.nbs[k].scale + plan.nbs[k].shift).cpu()
        a = a.permute(0, 3, 1, 2) if dims == 2 else a.permute(0, 4, 1, 2, 3)
        flips += int(((a > 0) != (acts[i] > 0)).sum())
    assert flips <= 4, flips
    if flips == 0:
        assert_close(xc.grad, x.grad, rtol=5e-3, atol=5e-3 * x.grad.abs().max().item(), what="dL/dx", outliers=0.005)
        _check_param_grads(ours, ref, rtol=5e-3)
    else:
        l2 = lambda a, b: ((a.double().cpu() - b).norm() / (b.norm() + 1e-30)).item()
        assert l2(xc.grad, x.grad) < 1e-1, (flips, l2(xc.grad, x.grad))
        rp = dict(ref.named_parameters())
        for name, q in ours.named_parameters():
            if not _pre_norm_bias(name, set(rp)):
                assert l2(q.grad, rp[name].grad) < 1e-1, (name, flips, l2(q.grad, rp[name].grad))
    for forwards in (1, 2):
        if forwards == 2:
            x2 = _x(spatial, seed=18)
            ref(x2.double())
            ours(x2.cuda())
        sd, sr = ours.state_dict(), ref.state_dict()
        assert list(sd) == list(sr)
        for k in sr:
            if "running_" in k:
                assert_close(sd[k], sr[k], rtol=1e-4, atol=1e-6, what=f"{k} after {forwards}")
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == int(sr[k]) == forwards, (k, int(sd[k]), int(sr[k]))


def test_frozen_parameters_only_input_grad():
    """The G step: D's parameters are toggled off, only dL/d(input) flows (maphead_backward with g_a alone)."""
    spatial, map_size = SHAPES["2d"]
    d = _ours(_ref(2), spatial)
    for p in d.parameters():
        p.requires_grad_(False)
    x = _x(spatial).cuda().requires_grad_(True)
    d(x).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    assert all(p.grad is None or p.grad.abs().sum() == 0 for p in d.parameters())


def test_bf16_storage_head_on_the_plans_own_activation():
    """The head is fp32 in every plan: prob is the conv + sigmoid of the plan's own stored fp32 last activation, and the
    gradient it leaves the transposed conv of the dlogit it was given -- whatever the bf16 stack rounded before."""
    spatial, map_size = SHAPES["2d"]
    ref = _ref(2)
    ours = _ours(ref, spatial, storage_dtype="bf16")
    x = _x(spatial).cuda().requires_grad_(True)
    p = ours(x)
    assert p.shape == (N, 1, *map_size)
    gen = torch.Generator().manual_seed(3)
    (p * (torch.rand(p.shape, generator=gen) - 0.5).cuda()).sum().backward()
    plan = [pl for pool in ours._plans.values() for pl in pool][0]
    assert type(plan).__name__ == "DiscPlanBF16" and type(plan.head).__name__ == "MapHead"
    a3 = plan.acts[3]
    assert a3.dtype == torch.float32 and plan.gas[-1].dtype == torch.float32
    a64 = from_cl(a3, 2).double()
    w, b = ref.model_head[0].weight.detach(), ref.model_head[0].bias.detach()
    logit, prob = M.head_forward(a64, w, b)
    assert_close(plan.prob.cpu(), prob.reshape(-1), what="prob of the stored a_3")
    assert_close(p, prob, what="module output")
    dl = plan.head.dlogit.double().cpu().reshape(N, 1, *map_size)
    assert dl.abs().max() > 0
    g_a, dw, db = M.head_backward(a64, w, dl)
    assert_close(from_cl(plan.gas[-1], 2), g_a, what="gas[-1]")
    assert_close(ours.model_head[0].weight.grad, dw, what="head weight gradient")
    assert_close(ours.model_head[0].bias.grad, db, what="head bias gradient")
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_eval_mode(storage):
    spatial, map_size = SHAPES["2d"]
    ref = _ref(2)
    ref(_x(spatial, seed=4).double())                                   # running statistics away from (0, 1)
    ours = _ours(ref, spatial, storage_dtype=storage)
    ours.eval()
    ref.eval()
    before = {k: v.clone() for k, v in ours.state_dict().items()}
    x = _x(spatial)
    y = ours(x.cuda().requires_grad_(True))
    assert y.shape == (N, 1, *map_size) and not y.requires_grad and y.grad_fn is None
    with torch.no_grad():
        want = ref(x.double())
    if storage == "f32":
        assert_close(y, want, rtol=1e-4, atol=1e-6, what="eval validity map")
    else:
        assert torch.isfinite(y).all() and (y - want.float().cuda()).abs().max().item() < 0.05
    after = ours.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    plan = [pl for key, pool in ours._plans.items() if key[0] == "eval" for pl in pool][0]
    assert not plan.training and type(plan.head).__name__ == "MapHead"
    assert "maphead_forward" in plan.fwd.names and not plan.bwd.names


# ---- trainer -------------------------------------------------------------------------------------------------------
# GAN(1, 26, 34, dimensions=2, d_head="markovian") with a generator that takes 26 x 34: the default U-Net halves its
# input three times and needs sides that are multiples of 8 (the oracle's fails alike at 26), one stride-2 level does not
GEN_KW = dict(n_unet_blocks=2, unet_channels=(16, 32), unet_strides=(2,))


@functools.lru_cache(maxsize=None)
def _batch():
    g = torch.Generator().manual_seed(5)
    return {k: torch.rand(N, 1, 26, 34, generator=g) * 2 - 1 for k in ("t1w", "t2w")}


def _gan(**kw):
    from mpgan_amd.gan import GAN
    from oracle import refmodel as R
    ref_g = R.CasNetGenerator((1, 26, 34), 2, dimensions=2, channels=(16, 32), strides=(2,))
    R.closed_form_fill_(ref_g)
    ref_d = _ref(2)
    ours = GAN(1, 26, 34, dimensions=2, d_head="markovian", **GEN_KW, **kw)
    ours.generator.load_state_dict(ref_g.state_dict())
    ours.discriminator.load_state_dict({k: v.float() for k, v in ref_d.state_dict().items()})
    return ours, ref_g.double().train(), ref_d


def test_trainer_step_matches_a_restated_step():
    """One fit_batch against the restated step, as __graft_entry__.smoke() holds the default trainer at its small shape:
    the generator's losses before any update, then OUR updated generator into the restatement so that both D steps
    start level, each logged scalar within 2e-3 relative + 1e-5."""
    ours, ref_g, ref_d = _gan()
    assert ours.hparams.d_head == "markovian"
    opts, _ = ours.configure_optimizers()
    before = {k: v.detach().clone() for k, v in ours.named_parameters()}
    cuda_batch = {k: v.cuda() for k, v in _batch().items()}
    log = ours.fit_batch(cuda_batch, 0, opts)
    assert set(log) == {"g_adv_loss", "g_recon_loss", "g_loss", "d_loss"}
    batch64 = {k: v.double() for k, v in _batch().items()}
    for p in ref_d.parameters():
        p.requires_grad_(False)
    want = {k: float(v) for k, v in M.step_losses_g(ref_g, ref_d, batch64).items()}
    with torch.no_grad():
        mine = dict(ours.generator.named_parameters())
        for name, p in ref_g.named_parameters():
            p.copy_(mine[name].detach().cpu().double())
        want["d_loss"] = float(M.step_loss_d(ref_g, ref_d, batch64))
    for k in ("g_adv_loss", "g_recon_loss", "g_loss", "d_loss"):
        got = float(log[k])
        print(f"{k}: got {got:.7f} want {want[k]:.7f}")
        assert torch.isfinite(log[k]).all()
        assert abs(got - want[k]) <= 2e-3 * abs(want[k]) + 1e-5, (k, got, want[k])
    still = [k for k, v in ours.named_parameters() if torch.equal(v.detach(), before[k])]
    assert not still, still
    assert any(k.startswith("discriminator.model_head.0") for k in before)

    # validation_step: the val_ keys, and nothing written
    state = {k: v.clone() for k, v in ours.state_dict().items()}
    opt_state = [(o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_count) for o in opts]
    grads = [net.store.flat_grad.clone() for net in (ours.generator, ours.discriminator)]
    val = ours.validation_step(cuda_batch, 0)
    assert set(val) == {"val_g_adv_loss", "val_g_recon_loss", "val_g_loss", "val_d_loss"}
    assert all(torch.isfinite(v).all() and not v.requires_grad for v in val.values())
    after = ours.state_dict()
    assert set(after) == set(state)
    for k, v in state.items():
        assert torch.equal(after[k], v), k
    for o, (avg, avg_sq, steps) in zip(opts, opt_state):
        assert torch.equal(o.exp_avg, avg) and torch.equal(o.exp_avg_sq, avg_sq) and o.step_count == steps
    for net, grad in zip((ours.generator, ours.discriminator), grads):
        assert torch.equal(net.store.flat_grad, grad)


def test_trainer_composes_with_the_ssim_term():
    ours, _, _ = _gan(ssim_weight=0.5)
    opts, _ = ours.configure_optimizers()
    log = ours.fit_batch({k: v.cuda() for k, v in _batch().items()}, 0, opts)
    assert set(log) == {"g_adv_loss", "g_recon_loss", "g_ssim_loss", "g_loss", "d_loss"}
    assert all(torch.isfinite(v).all() for v in log.values())
    want = float(log["g_adv_loss"]) + float(log["g_recon_loss"]) + 0.5 * float(log["g_ssim_loss"])
    assert abs(float(log["g_loss"]) - want) <= 4 * 2.0 ** -23 * max(abs(want), 1.0)
