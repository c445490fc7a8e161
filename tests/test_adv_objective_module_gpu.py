"""Discriminator(output="logit") and GAN(adv_loss="bce_logits" | "lsgan") behind the module and trainer API, at the
smallest shapes each head admits (the ones tests/test_networks_gpu.py and tests/test_map_head_module_gpu.py use), against
float64 restatements with closed-form weights and the final Sigmoid left off: oracle.refmodel.Discriminator for the
Linear head, tests/map_head_ref.MarkovianDiscriminator for the Markovian one.  eps = 2^-23."""
import copy
import functools

import pytest
import torch

import adv_loss_ref as A
import map_head_ref as M
from gpu_helpers import assert_close
from test_networks_gpu import _check_param_grads, _pre_norm_bias

pytestmark = pytest.mark.gpu
EPS = A.EPS

#          head         which  spatial        batch
CASES = [("linear", "2d", (32, 40), 3), ("linear", "3d", (28, 28, 32), 2),
         ("markovian", "2d", (26, 34), 2), ("markovian", "3d", (26, 26, 30), 2)]
SMALL = {"linear": ((32, 40), 3), "markovian": ((26, 34), 2)}
IDS = [f"{h}-{w}" for h, w, _, _ in CASES]


def _ref(head, spatial):
    """The float64 restatement with closed-form weights (fp32 values held in float64), train mode."""
    from oracle import refmodel as R
    dims = len(spatial)
    ref = M.MarkovianDiscriminator(dims) if head == "markovian" else R.Discriminator((1, *spatial), dimensions=dims)
    R.closed_form_fill_(ref)
    return ref.double().train()


def _ours(ref, head, spatial, **kw):
    from mpgan_amd.networks import Discriminator
    ours = Discriminator((1, *spatial), dimensions=len(spatial), head=head, **kw)
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return ours.cuda().train()


def _x(n, spatial, seed=17):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(n, 1, *spatial, generator=gen) * 2 - 1


def _plans(d, eval_plans=False):
    return [pl for key, pool in d._plans.items() if (key[0] == "eval") == eval_plans for pl in pool]


@pytest.mark.parametrize("head,which,spatial,n", CASES, ids=IDS)
def test_train_mode_logits_match_the_restatement(head, which, spatial, n):
    """|logit - logit_f64| <= 3 x (the error of the restatement in fp32 on the CPU against itself in fp64) -- the
    project's rule for parity -- plus 4 eps max|logit_f64|, the rounding of the result itself."""
    ref = _ref(head, spatial)
    ref32 = copy.deepcopy(ref).float()
    x = _x(n, spatial)
    with torch.no_grad():
        want = A.disc_logits(ref, x.double())
        cpu32 = A.disc_logits(ref32, x)
    ours = _ours(ref, head, spatial, output="logit")
    z = ours(x.cuda().requires_grad_(True))
    assert z.shape == want.shape == ours.validity_shape(n, spatial) and z.dtype == torch.float32
    assert z.requires_grad and z.grad_fn is not None
    err = (z.detach().double().cpu() - want).abs().max().item()
    err32 = (cpu32.double() - want).abs().max().item()
    bound = 3 * err32 + 4 * EPS * want.abs().max().item()
    print(f"{head} {which}: logit err {err:.3e}, fp32 CPU err {err32:.3e}, max|logit| {want.abs().max().item():.4f}, "
          f"bound {bound:.3e}")
    assert err <= bound, (err, err32, bound)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("head", ["linear", "markovian"])
def test_probability_path_is_the_sigmoid_of_the_logit_path(head, storage, mode):
    """Within one storage mode the two outputs share every launch up to the head: |p - sigma_f64(logit)| <= 4 eps."""
    spatial, n = SMALL[head]
    ref = _ref(head, spatial)
    with torch.no_grad():
        ref(_x(n, spatial, seed=4).double())                            # running statistics away from (0, 1)
    d_logit = _ours(ref, head, spatial, output="logit", storage_dtype=storage)
    d_prob = _ours(ref, head, spatial, storage_dtype=storage)
    assert d_prob.output == "prob"
    if mode == "eval":
        d_logit.eval()
        d_prob.eval()
    x = _x(n, spatial).cuda()
    z, p = d_logit(x), d_prob(x)
    assert z.shape == p.shape == d_logit.validity_shape(n, spatial)
    assert z.requires_grad == p.requires_grad == (mode == "train")
    assert torch.isfinite(z).all() and 0.0 <= p.min().item() and p.max().item() <= 1.0
    err = (p.double() - torch.sigmoid(z.detach().double())).abs().max().item()
    print(f"{head} {storage} {mode}: |p - sigma(logit)| {err:.3e} (4 eps = {4 * EPS:.3e})")
    assert err <= 4 * EPS, err


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("head,which,spatial,n", CASES, ids=IDS)
def test_gradients_match_the_restatement(head, which, spatial, n, kind):
    """The objective against a 0.9 target, backward: dL/dx and parameter gradients with the bounds, the kink-flip
    counting and the helpers of test_discriminator_forward_backward_matches_oracle / test_map_head_module_gpu; running
    statistics and num_batches_tracked after one and two forwards."""
    from mpgan_amd.gan import adversarial_loss
    dims = len(spatial)
    ref = _ref(head, spatial)
    ours = _ours(ref, head, spatial, output="logit")
    x = _x(n, spatial).double().requires_grad_(True)
    acts = {}
    hooks = [ref.model_conv[i].register_forward_hook(lambda m, a, out, i=i: acts.__setitem__(i, out.detach()))
             for i in (1, 4, 7, 10)]
    z_ref = A.disc_logits(ref, x)
    for h in hooks:
        h.remove()
    loss_ref = A.torch_objective(kind, z_ref, torch.full_like(z_ref, 0.9))
    loss_ref.backward()
    xc = x.detach().float().cuda().requires_grad_(True)
    z = ours(xc)
    loss = adversarial_loss(z, torch.full_like(z, 0.9), kind=kind)
    assert_close(loss.reshape(1), loss_ref.reshape(1), rtol=1e-5, what=f"{kind} against 0.9")
    loss.backward()
    plan = _plans(ours)[0]
    assert plan.g_prob is None and plan.g_logit is not None and "sigmoid_backward" not in plan.bwd.names
    flips = 0
    for k, i in enumerate((1, 4, 7, 10)):
        zk = plan.zs[k].squeeze(1) if dims == 2 else plan.zs[k]
        a = (zk * plan.nbs[k].scale + plan.nbs[k].shift).cpu()
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
            x2 = _x(n, spatial, seed=18)
            with torch.no_grad():
                ref(x2.double())
            ours(x2.cuda())
        sd, sr = ours.state_dict(), ref.state_dict()
        assert list(sd) == list(sr)
        for k in sr:
            if "running_" in k:
                assert_close(sd[k], sr[k], rtol=1e-4, atol=1e-6, what=f"{k} after {forwards}")
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == int(sr[k]) == forwards, (k, int(sd[k]), int(sr[k]))


@pytest.mark.parametrize("head", ["linear", "markovian"])
def test_frozen_parameters_only_input_grad(head):
    """The G step: D's parameters are toggled off, only dL/d(input) flows."""
    spatial, n = SMALL[head]
    d = _ours(_ref(head, spatial), head, spatial, output="logit")
    for p in d.parameters():
        p.requires_grad_(False)
    x = _x(n, spatial).cuda().requires_grad_(True)
    d(x).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    assert all(p.grad is None or p.grad.abs().sum() == 0 for p in d.parameters())


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("head", ["linear", "markovian"])
def test_programs(head, storage):
    """output="logit": no sigmoid_backward in the backward program, no prob buffer; the default keeps both.  Eval plans
    have an empty backward program and write nothing of the module."""
    spatial, n = SMALL[head]
    ref = _ref(head, spatial)
    x = _x(n, spatial).cuda()
    outs = {}
    for output in ("logit", "prob"):
        d = _ours(ref, head, spatial, output=output, storage_dtype=storage)
        y = d(x.clone().requires_grad_(True))
        y.sum().backward()
        plan, = _plans(d)
        assert type(plan).__name__ == ("DiscPlanBF16" if storage == "bf16" else "DiscPlan")
        fwd_head = "maphead_forward" if head == "markovian" else "linear1_forward"
        assert fwd_head in plan.fwd.names
        if output == "logit":
            assert "sigmoid_backward" not in plan.bwd.names
            assert plan.prob is None and plan.g_prob is None and plan.g_logit is plan.head.dlogit
        else:
            assert plan.bwd.names.count("sigmoid_backward") == 1
            assert plan.prob is not None and plan.g_prob is not None and plan.g_logit is None
            assert 0.0 <= y.min().item() and y.max().item() <= 1.0
        outs[output] = (d, len(plan.bwd.names))
    assert outs["logit"][1] == outs["prob"][1] - 1
    for output, (d, _) in outs.items():
        d.eval()
        before = {k: v.clone() for k, v in d.state_dict().items()}
        grads = d.store.flat_grad.clone()
        y = d(x.clone().requires_grad_(True))
        assert not y.requires_grad and y.grad_fn is None and torch.isfinite(y).all()
        plan, = _plans(d, eval_plans=True)
        assert not plan.training and not plan.bwd.names and (plan.prob is None) == (output == "logit")
        after = d.state_dict()
        assert list(after) == list(before)
        for k, v in before.items():
            assert torch.equal(after[k], v), k
        assert torch.equal(d.store.flat_grad, grads)


# ---- trainer -------------------------------------------------------------------------------------------------------
GEN_KW = dict(n_unet_blocks=2, unet_channels=(16, 32), unet_strides=(2,))
NAMES = ("g_adv_loss", "g_recon_loss", "g_loss", "d_loss")


@functools.lru_cache(maxsize=None)
def _batch():
    g = torch.Generator().manual_seed(5)
    return {k: torch.rand(2, 1, 26, 34, generator=g) * 2 - 1 for k in ("t1w", "t2w")}


def _gan(kind, head, **kw):
    from mpgan_amd.gan import GAN
    from oracle import refmodel as R
    ref_g = R.CasNetGenerator((1, 26, 34), 2, dimensions=2, channels=(16, 32), strides=(2,))
    R.closed_form_fill_(ref_g)
    ref_d = _ref(head, (26, 34))
    ours = GAN(1, 26, 34, dimensions=2, adv_loss=kind, d_head=head, **GEN_KW, **kw)
    ours.generator.load_state_dict(ref_g.state_dict())
    ours.discriminator.load_state_dict({k: v.float() for k, v in ref_d.state_dict().items()})
    return ours, ref_g.double().train(), ref_d


@pytest.mark.parametrize("head", ["linear", "markovian"])
@pytest.mark.parametrize("kind", A.KINDS)
def test_trainer_step_matches_a_restated_step(kind, head):
    """One fit_batch against the float64 restated step with the same objective, as
    test_map_head_module_gpu.test_trainer_step_matches_a_restated_step holds the default objective: the generator's
    losses before any update, then OUR updated generator into the restatement so that both D steps start level, each
    logged scalar within 2e-3 relative + 1e-5."""
    ours, ref_g, ref_d = _gan(kind, head)
    assert ours.hparams.adv_loss == kind and ours.hparams.d_head == head and ours.discriminator.output == "logit"
    opts, _ = ours.configure_optimizers()
    before = {k: v.detach().clone() for k, v in ours.named_parameters()}
    cuda_batch = {k: v.cuda() for k, v in _batch().items()}
    log = ours.fit_batch(cuda_batch, 0, opts)
    assert set(log) == set(NAMES)
    batch64 = {k: v.double() for k, v in _batch().items()}
    with torch.no_grad():
        want = {k: float(v) for k, v in A.step_losses_g(ref_g, ref_d, batch64, kind, head).items()}
        mine = dict(ours.generator.named_parameters())
        for name, p in ref_g.named_parameters():
            p.copy_(mine[name].detach().cpu().double())
        want["d_loss"] = float(A.step_loss_d(ref_g, ref_d, batch64, kind, head))
    for k in NAMES:
        got = float(log[k])
        print(f"{kind} {head} {k}: got {got:.7f} want {want[k]:.7f}")
        assert torch.isfinite(log[k]).all()
        assert abs(got - want[k]) <= 2e-3 * abs(want[k]) + 1e-5, (k, got, want[k])
    # Every parameter has moved.  Adam's first step moves a parameter by lr * sign(gradient) and leaves it only where the
    # gradient is exactly zero.  That IS the exact gradient of a conv bias that feeds a norm layer (the norm removes the
    # mean; tests/test_networks_gpu.py: _pre_norm_bias), and both sides hold rounding noise there: a one-element bias of
    # this kind (the generator's 1-channel up-convolutions) may hold the exact 0.0 and then stays where it was --
    # measured: generator.model.1.model.2.0.conv.bias under lsgan with the Linear head.  Such a parameter is held to
    # that instead: pre-norm bias, one element, gradient exactly 0.0.  (The generator's gradients of the G step are
    # still in place: the D step runs the generator without autograd.)
    named = dict(ours.named_parameters())
    keys = {k[len("generator."):] for k in named if k.startswith("generator.")}
    still = [k for k, v in named.items() if torch.equal(v.detach(), before[k])]
    for k in still:
        assert k.startswith("generator.") and _pre_norm_bias(k[len("generator."):], keys), still
        q = named[k]
        assert q.numel() == 1 and q.grad is not None and float(q.grad.abs().max()) == 0.0, (k, q.grad)
    assert len(still) <= 1, still

    # validation_step: finite detached scalars, and nothing written
    state = {k: v.clone() for k, v in ours.state_dict().items()}
    opt_state = [(o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_count) for o in opts]
    grads = [net.store.flat_grad.clone() for net in (ours.generator, ours.discriminator)]
    val = ours.validation_step(cuda_batch, 0)
    assert set(val) == {"val_" + k for k in NAMES}
    assert all(torch.isfinite(v).all() and not v.requires_grad and v.grad_fn is None for v in val.values())
    after = ours.state_dict()
    assert set(after) == set(state)
    for k, v in state.items():
        assert torch.equal(after[k], v), k
    for o, (avg, avg_sq, steps) in zip(opts, opt_state):
        assert torch.equal(o.exp_avg, avg) and torch.equal(o.exp_avg_sq, avg_sq) and o.step_count == steps
    for net, grad in zip((ours.generator, ours.discriminator), grads):
        assert torch.equal(net.store.flat_grad, grad)


def test_unknown_objective_is_refused():
    from mpgan_amd.gan import GAN
    with pytest.raises(ValueError, match="adv_loss"):
        GAN(1, 26, 34, dimensions=2, adv_loss="bogus", **GEN_KW)


@pytest.mark.parametrize("kind,head,extra", [("bce_logits", "markovian", dict(storage_dtype="bf16")),
                                             ("lsgan", "linear", dict(ssim_weight=0.5))],
                         ids=["bf16-storage", "ssim-term"])
def test_trainer_composes(kind, head, extra):
    ours, _, _ = _gan(kind, head, **extra)
    opts, _ = ours.configure_optimizers()
    log = ours.fit_batch({k: v.cuda() for k, v in _batch().items()}, 0, opts)
    ssim = "ssim_weight" in extra
    assert set(log) == set(NAMES) | ({"g_ssim_loss"} if ssim else set())
    assert all(torch.isfinite(v).all() for v in log.values())
    want = float(log["g_adv_loss"]) + float(log["g_recon_loss"]) + (0.5 * float(log["g_ssim_loss"]) if ssim else 0.0)
    assert abs(float(log["g_loss"]) - want) <= 4 * EPS * max(abs(want), 1.0)
