"""Eval-mode discriminators on the device: the bf16 forward conv with the BatchNorm + LeakyReLU epilogue per launch, the
four eval plans against the REFERENCE'S OWN eval-mode classes (tests/golden/disc_eval.npz) and against the bf16
emulation (tests/disc_eval_ref.py), train -> eval -> train -> eval, that an eval pass and validation_step write nothing,
validation_step's scalars against the CPU oracle, and the eval rule (no gradients offered).

Bounds (none is derived from what the code under test returns):
  * bf16 store: one rounding to 8 significand bits is <= 2^-9 relative; 4e-3 * |ref| + 2e-3 (x max|scale| once an affine
    follows the accumulator) is what tests/test_bf16_gpu.py holds the plain bf16 forward to;
  * fp32 result of bf16 operands: 1e-4 * |ref| + 1e-4 * max|ref| (test_bf16_gpu.py, weight gradient);
  * fp32 networks against the reference fixture: validity 2e-6, tap summaries 2e-4 / 2e-4 (test_variant_b_gpu.py,
    test_fullsize_gpu.py hold the train-mode passes of the same tensors to these);
  * bf16 networks: validity 2e-2 (test_bf16_gpu.py);
  * logged scalars against the CPU oracle: 2e-3 relative (test_networks_gpu.py, test_fullsize_gpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from disc_eval_ref import conv_act_ref, disc_eval_bf16, eval_affine, lrelu
from gpu_helpers import from_cl, t3, to_cl
from test_bf16_gpu import CASES, _sparse_int

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# (n, spatial, cin, cout, k, stride, pad, min_blocks): test_bf16_gpu.py's forward geometries, then D's dense layers at a
# reduced spatial size (A: 64 -> 128 k3, 128 -> 256 k4 s2, 256 -> 256 k4 s2; B: 128 -> 256 k3, 256 -> 512 k3), then what
# it takes to reach every forward form (min_blocks = 1 lets a small shape onto the wide forms, as test_bf16_gpu.py does)
LAUNCH_CASES = [c + (0,) for c in CASES] + [
    (1, (18, 18, 18), 64, 128, 3, 1, 0, 0),       # A.conv2, 16^3 outputs: the 8 x 8 x 8 patch form
    (1, (16, 16, 16), 128, 256, 4, 2, 0, 0),      # A.conv3: 64 taps, stride 2
    (2, (8, 8, 8), 256, 256, 4, 2, 0, 1),         # A.conv4 on 256 x 256 tiles
    (2, (12, 12, 12), 128, 256, 3, 1, 0, 0),      # B.conv3
    (2, (10, 10, 10), 256, 512, 3, 1, 0, 0),      # B.conv4
    (2, (22, 20), 128, 256, 4, 2, 0, 1),          # 256 x 256 tiles, ragged last tile
    (3, (21, 19), 64, 128, 3, 1, 1, 1),           # 512 x 128 tiles, masked
]
FORMS = {0: "Narrow", 1: "Patch", 2: "Wide256", 3: "Wide512", 5: "Patch8"}


def _geom(n, spatial, cin, cout, k, s, p, mb=0):
    from mpgan_amd import ops
    dims = len(spatial)
    return ops.ConvGeom(n, t3(spatial, dims, 1), cin, cout, t3(k, dims, 1), t3(s, dims, 1), t3(p, dims, 0), min_blocks=mb)


def _variant(g):
    from mpgan_amd._lib import lib
    gc = g.c()
    return int(lib().mpgan_conv_variant_bf16(C.byref(gc), 0))


def _operands(n, spatial, cin, cout, k, exact, gen):
    """x, w, bias, scale, shift, slope of one launch in the two regimes of test_bf16_gpu.py."""
    dims = len(spatial)
    if exact:
        x = _sparse_int((n, cin, *spatial), gen)
        w = _sparse_int((cout, cin, *([k] * dims)), gen)
        b = torch.randint(-3, 4, (cout,), generator=gen).float()
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=gen)]
        shift = torch.randint(-3, 4, (cout,), generator=gen).float()
        slope = torch.where(torch.arange(cout) % 2 == 0, 0.5, 1.0)
    else:
        x = (torch.rand(n, cin, *spatial, generator=gen) - 0.5).to(BF).float()
        w = ((torch.rand(cout, cin, *([k] * dims), generator=gen) - 0.5) * 0.2).to(BF).float()
        b = torch.rand(cout, generator=gen) - 0.5
        scale = torch.rand(cout, generator=gen) * 1.5 + 0.5
        shift = torch.rand(cout, generator=gen) - 0.5
        slope = torch.full((cout,), 0.2)
    return x, w, b, scale, shift, slope


def _vec(t):
    """A 16-byte aligned device copy (fresh allocations are 256-byte aligned)."""
    return t.contiguous().cuda()


@pytest.mark.parametrize("n,spatial,cin,cout,k,s,p,mb", LAUNCH_CASES, ids=lambda v: str(v))
def test_conv_forward_act_bf16_exact_random_and_against_the_unfused_pair(n, spatial, cin, cout, k, s, p, mb):
    from mpgan_amd import ops
    g = _geom(n, spatial, cin, cout, k, s, p, mb)
    dims = len(spatial)
    form = _variant(g)
    assert form in FORMS, form
    gen = torch.Generator().manual_seed(31)
    for exact in (True, False):
        x, w, b, scale, shift, slope = _operands(n, spatial, cin, cout, k, exact, gen)
        ref, zref = conv_act_ref(x, w, b, scale, shift, slope, stride=s, padding=p)
        sh_total = shift + b * scale                                   # the conv bias folded into the shift (exact in the exact regime)
        xd, wd = to_cl(x).to(BF), ops.pack_weight_bf16(w.cuda())
        vs, vh, vl = _vec(scale), _vec(sh_total), _vec(slope)
        y16 = torch.full((n, *g.out_dhw, cout), float("nan"), device="cuda", dtype=BF)
        y32 = torch.full((n, *g.out_dhw, cout), float("nan"), device="cuda")
        ops.conv_forward_act_bf16(g, xd, wd, vs, vh, vl, y16)
        ops.conv_forward_act_bf16(g, xd, wd, vs, vh, vl, y32)
        got16, got32 = from_cl(y16.float(), dims), from_cl(y32, dims)
        if exact:
            assert torch.equal(ref, ref.to(BF).float()), "test construction: a reference value is not a bf16 number"
            assert torch.equal(got16, ref), (FORMS[form], (got16 - ref).abs().max().item())
            assert torch.equal(got32, ref), (FORMS[form], (got32 - ref).abs().max().item())
            continue
        smax = scale.abs().max().item()
        e16, e32 = (got16 - ref).abs(), (got32 - ref).abs()
        print(f"{FORMS[form]:8s} {cin}->{cout} k{k}s{s}: bf16 out max err {e16.max().item():.3e}, fp32 out {e32.max().item():.3e}"
              f" (max|ref| {ref.abs().max().item():.3f})")
        assert (e16 <= 4e-3 * ref.abs() + 2e-3 * smax).all(), (FORMS[form], e16.max().item())
        assert (e32 <= 1e-4 * ref.abs() + 1e-4 * ref.abs().max()).all(), (FORMS[form], e32.max().item())
        # the unfused pair rounds twice (z, then a), the fused launch once
        z = torch.empty(n, *g.out_dhw, cout, device="cuda", dtype=BF)
        ops.conv_forward_bf16(g, xd, wd, b.cuda(), z)
        a = torch.empty_like(z)
        ops.norm_act_bf16(z, vs, _vec(shift), 0.2, a)
        unf = from_cl(a.float(), dims)
        shp = [1, -1] + [1] * dims
        d = (got16 - unf).abs()
        print(f"{'':8s} fused vs unfused: {(d > 0).float().mean().item() * 100:.2f} % of the elements differ, max {d.max().item():.3e}")
        assert (d <= 4e-3 * ((zref * scale.view(shp)).abs() + ref.abs()) + 2e-3 * smax).all(), (FORMS[form], d.max().item())


def test_the_launch_cases_cover_every_forward_form():
    """All five forms choose_bf16 can pick for a forward launch are among the cases above (each case asserts the form
    it was launched on through the same query)."""
    forms = {_variant(_geom(*c)) for c in LAUNCH_CASES}
    print("forms of the launch cases:", sorted(FORMS[f] for f in forms))
    assert forms == set(FORMS), {FORMS[k] for k in set(FORMS) - forms}


@pytest.mark.parametrize("n,spatial,cout", [(2, (20, 22), 64), (1, (12, 14, 13), 64), (2, (9, 9, 9), 32), (1, (20, 20, 20), 64)],
                         ids=lambda v: str(v))
def test_first_layer_act_f32_to_bf16(n, spatial, cout):
    """The 1-input-channel layer (fp32 image in, activated bf16 out): the row-walking kernel (64 channels, k3) and the
    all-channel kernel, exact and random."""
    from mpgan_amd import ops
    g = _geom(n, spatial, 1, cout, 3, 1, 0)
    dims = len(spatial)
    gen = torch.Generator().manual_seed(32)
    for exact in (True, False):
        x, w, b, scale, shift, slope = _operands(n, spatial, 1, cout, 3, exact, gen)
        if exact:
            x = _sparse_int((n, 1, *spatial), gen, density=0.5)
            w = _sparse_int((cout, 1, *([3] * dims)), gen, density=0.5)
        else:
            x, w = torch.rand(n, 1, *spatial, generator=gen) * 2 - 1, (torch.rand(cout, 1, *([3] * dims), generator=gen) - 0.5)
        ref, _ = conv_act_ref(x, w, b, scale, shift, slope)
        y = torch.full((n, *g.out_dhw, cout), float("nan"), device="cuda", dtype=BF)
        ops.conv_forward_act_f32_to_bf16(g, to_cl(x), ops.pack_weight(w.cuda()), _vec(scale), _vec(shift + b * scale),
                                         _vec(slope), y)
        got = from_cl(y.float(), dims)
        if exact:
            assert torch.equal(ref, ref.to(BF).float()), "test construction: a reference value is not a bf16 number"
            assert torch.equal(got, ref), (got - ref).abs().max().item()
        else:
            err = (got - ref).abs()
            print(f"first layer 1->{cout} {spatial}: max err {err.max().item():.3e}")
            assert (err <= 4e-3 * ref.abs() + 2e-3 * scale.abs().max()).all(), err.max().item()


# ---------------------------------------------------------------------------------------------------------------------
# networks against the reference fixture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "disc_eval.npz"))


def _oracle_b(fx):
    """oracle.refmodel.PatchDiscriminator with the closed-form weights and the REFERENCE'S buffers after its train pass."""
    from oracle import refmodel as R
    ref = R.PatchDiscriminator((1, 16, 16, 16))
    R.closed_form_fill_(ref)
    sd = ref.state_dict()
    for name in [k for k in sd if "b_buf__" + k in fx]:
        sd[name] = torch.from_numpy(fx["b_buf__" + name])
    ref.load_state_dict(sd)
    return ref.eval()


def _oracle_a(fx):
    from oracle import refmodel as R
    ref = R.Discriminator((1, 128, 128, 128))
    R.closed_form_fill_(ref)
    sd = ref.state_dict()
    for name in [k for k in sd if "a_buf__" + k in fx]:
        sd[name] = torch.from_numpy(fx["a_buf__" + name])
    ref.load_state_dict(sd)
    return ref.eval()


def _x_a(fx):
    g = torch.Generator().manual_seed(int(fx["a_seed"]))
    torch.rand(1, 1, 128, 128, 128, generator=g)                       # (the train pass's input)
    return torch.rand(1, 1, 128, 128, 128, generator=g) * 2 - 1


def _ours_b(ref, storage="f32", perceptual=True):
    from mpgan_amd.networks import PatchDiscriminator
    d = PatchDiscriminator((1, 16, 16, 16), use_perceptual=perceptual, storage_dtype=storage)
    d.load_state_dict(ref.state_dict())
    return d.cuda().eval()


def _state(mod):
    """Everything of a module an eval pass must leave alone."""
    st = {"flat": mod.store.flat.clone(), "flat_grad": mod.store.flat_grad.clone()}
    st.update({"buf:" + n: b.clone() for n, b in mod.named_buffers()})
    st.update({"mode:" + n: torch.tensor(m.training) for n, m in mod.named_modules()})
    return st


def _assert_untouched(before, after, what):
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k].cpu(), after[k].cpu()), (what, k)


def _logit(v):
    v = v.double()
    return torch.log(v / (1 - v))


def test_patch_discriminator_eval_fp32_matches_the_reference_fixture(fx):
    """Both eval programs of variant B (fp32) against the reference's eval pass: validity 2e-6, logit 1e-4 relative,
    every tap summary 2e-4 / 2e-4; the fused and the tap-keeping program agree on the validity to 2e-6."""
    from oracle.make_golden import summarize
    ref = _oracle_b(fx)
    x = torch.from_numpy(fx["b_x_eval"]).cuda()
    vals = {}
    for perceptual in (True, False):
        d = _ours_b(ref, perceptual=perceptual)
        before = _state(d)
        val, taps = d(x)
        _assert_untouched(before, _state(d), f"PatchDiscriminator eval (perceptual={perceptual})")
        vals[perceptual] = val.cpu()
        dv = np.abs(val.cpu().numpy() - fx["b_validity"]).max()
        lg = _logit(val.cpu()).numpy()
        dl = np.abs(lg - fx["b_logit"]).max()
        print(f"B fp32 eval ({'tap-keeping' if perceptual else 'fused'}): |validity - fixture| {dv:.3e}, |logit - fixture| {dl:.3e}")
        np.testing.assert_allclose(val.cpu().numpy(), fx["b_validity"], rtol=0, atol=2e-6)
        if not perceptual:
            assert taps == {}
            # (the logit through the validity: sigmoid halves the relative resolution near 0.5 -- 2e-6 of validity is
            #  8e-6 of logit, 2.7e-4 of a 0.03 logit; the plan's own logit is the one held to 1e-4)
            plan = next(iter(d._plans.values()))[0]
            np.testing.assert_allclose(plan.logit.reshape(-1, 1).cpu().double().numpy(), fx["b_logit"], rtol=1e-4, atol=0)
            continue
        assert sorted(taps.keys()) == list(range(16))
        for k in range(16):
            t = taps.tapset.materialize(k)
            assert not t.requires_grad
            assert tuple(t.shape) == tuple(fx[f"b_tap{k}_shape"]), k
            np.testing.assert_allclose(summarize(t.cpu()), fx[f"b_tap{k}"], rtol=2e-4, atol=2e-4, err_msg=f"tap {k}")
        np.testing.assert_allclose(taps[14].cpu().double().numpy(), fx["b_logit"], rtol=1e-4, atol=0)
        assert not taps[5].requires_grad                               # through the TapDict too: detached in eval mode
    np.testing.assert_allclose(vals[True].numpy(), vals[False].numpy(), rtol=0, atol=2e-6)


def test_perceptual_loss_on_eval_taps_matches_the_oracle(fx):
    """The fused perceptual loss runs unchanged on two tap-keeping eval passes (value only)."""
    from mpgan_amd.gan_patch import perceptual_loss
    from oracle import refmodel as R
    ref = _oracle_b(fx)
    d = _ours_b(ref)
    xa, xb = torch.from_numpy(fx["b_x_eval"]), torch.from_numpy(fx["b_x_train"][:3])
    _, ta = d(xa.cuda())
    _, tb = d(xb.cuda())
    out = perceptual_loss(ta, tb)
    with torch.no_grad():
        want = R.perceptual_loss(ref(xa)[1], ref(xb)[1])
    assert out.shape == (1,) and not out.requires_grad
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=2e-4)


def test_discriminator_128cubed_eval_fp32_matches_the_reference_fixture(fx):
    from mpgan_amd.networks import Discriminator
    ref = _oracle_a(fx)
    d = Discriminator((1, 128, 128, 128))
    d.load_state_dict(ref.state_dict())
    d.cuda().eval()
    before = _state(d)
    v = d(_x_a(fx).cuda())
    _assert_untouched(before, _state(d), "Discriminator eval")
    print(f"A fp32 eval at 128^3: validity {v.item():.7f}, fixture {fx['a_validity'].item():.7f}, "
          f"|logit - fixture| {abs(_logit(v.cpu()).item() - fx['a_logit'].item()):.3e}")
    np.testing.assert_allclose(v.cpu().numpy(), fx["a_validity"], rtol=0, atol=2e-6)


def _last_act_bound(got, want, scale, what):
    err = (got - want).abs()
    bound = 4e-3 * want.abs() + 2e-3 * scale.abs().max()
    print(f"{what}: last activation max err {err.max().item():.3e} (max|ref| {want.abs().max().item():.3f}), "
          f"{(err > bound).sum().item()} of {err.numel()} beyond the per-store bound")
    assert (err <= bound).all(), (what, err.max().item())


def test_patch_discriminator_eval_bf16(fx):
    """Variant B in bf16 storage, both programs: validity within 2e-2 of the reference fixture; against the emulation of
    the same contract the last layer's activation within the per-store bound."""
    ref = _oracle_b(fx)
    x = torch.from_numpy(fx["b_x_eval"])
    scale3, _ = eval_affine(ref.model_conv[10])
    for perceptual in (False, True):
        d = _ours_b(ref, storage="bf16", perceptual=perceptual)
        before = _state(d)
        val, taps = d(x.cuda())
        _assert_untouched(before, _state(d), f"PatchDiscriminator bf16 eval (perceptual={perceptual})")
        emu = disc_eval_bf16(ref, x, fused=not perceptual)
        plan = next(iter(d._plans.values()))[0]
        what = f"B bf16 eval ({'tap-keeping' if perceptual else 'fused'})"
        print(f"{what}: |validity - fixture| {np.abs(val.cpu().numpy() - fx['b_validity']).max():.3e}, "
              f"|validity - emulation| {(val.cpu() - emu['validity']).abs().max().item():.3e}")
        np.testing.assert_allclose(val.cpu().numpy(), fx["b_validity"], rtol=0, atol=2e-2)
        np.testing.assert_allclose(val.cpu().numpy(), emu["validity"].numpy(), rtol=0, atol=2e-2)
        assert plan.acts[3].dtype == torch.float32 and plan.acts[2].dtype == BF
        _last_act_bound(from_cl(plan.acts[3], 3), emu["acts"][3], scale3, what)
        if perceptual:
            assert sorted(taps.keys()) == list(range(16)) and not taps[2].requires_grad
            with torch.no_grad():
                want = lrelu(ref.model_conv[:2](x), 0.2)
            got = taps.tapset.materialize(2).cpu()                    # LeakyReLU(BN_running(z_0)) of the stored bf16 z_0
            assert (got - want).abs().max().item() <= 4e-3 * want.abs().max().item() + 2e-3
        else:
            assert taps == {} and len(plan.zs) == 0                   # no raw z in the fused program


def test_discriminator_128cubed_eval_bf16(fx):
    from mpgan_amd.networks import Discriminator
    ref = _oracle_a(fx)
    d = Discriminator((1, 128, 128, 128), storage_dtype="bf16")
    d.load_state_dict(ref.state_dict())
    d.cuda().eval()
    x = _x_a(fx)
    before = _state(d)
    v = d(x.cuda())
    _assert_untouched(before, _state(d), "Discriminator bf16 eval")
    emu = disc_eval_bf16(ref, x, fused=True)
    plan = next(iter(d._plans.values()))[0]
    print(f"A bf16 eval at 128^3: validity {v.item():.6f}, fixture {fx['a_validity'].item():.6f}, emulation {emu['validity'].item():.6f}")
    np.testing.assert_allclose(v.cpu().numpy(), fx["a_validity"], rtol=0, atol=2e-2)
    np.testing.assert_allclose(v.cpu().numpy(), emu["validity"].numpy(), rtol=0, atol=2e-2)
    scale3, _ = eval_affine(ref.model_conv[10])
    _last_act_bound(from_cl(plan.acts[3], 3), emu["acts"][3], scale3, "A bf16 eval at 128^3")


# ---------------------------------------------------------------------------------------------------------------------
# modes on a live trainer
# ---------------------------------------------------------------------------------------------------------------------
def _gan_a(spatial=(64, 64), bs=2, seed=3, **kw):
    from mpgan_amd.gan import GAN
    from oracle import refmodel as R
    dims = len(spatial)
    ref = R.GAN((1, *spatial), dimensions=dims, n_unet_blocks=2)
    R.closed_form_fill_(ref.generator)
    R.closed_form_fill_(ref.discriminator)
    ours = GAN(1, *spatial, dimensions=dims, n_unet_blocks=2, **kw)
    ours.generator.load_state_dict(ref.generator.state_dict())
    ours.discriminator.load_state_dict(ref.discriminator.state_dict())
    ours.train()
    g = torch.Generator().manual_seed(seed)
    batch = {k: torch.rand(bs, 1, *spatial, generator=g) * 2 - 1 for k in ("t1w", "t2w")}
    return ours, ref, batch


_B_KW = dict(n_unet_blocks=1, num_samples=3, crop_seed=5)


def _gan_b(seed=4, use_perceptual=True, **kw):
    from mpgan_amd.gan_patch import GAN
    from oracle import refmodel as R
    ref = R.PatchGAN((1, 32, 32, 32), channels=(8, 16, 32), strides=(2, 2), use_perceptual=use_perceptual, **_B_KW)
    R.closed_form_fill_(ref.generator)
    R.closed_form_fill_(ref.discriminator)
    ours = GAN(1, 32, 32, 32, unet_channels=(8, 16, 32), unet_strides=(2, 2), use_perceptual=use_perceptual, **_B_KW, **kw)
    ours.generator.load_state_dict(ref.generator.state_dict())
    ours.discriminator.load_state_dict(ref.discriminator.state_dict())
    ours.train()
    g = torch.Generator().manual_seed(seed)
    batch = {k: torch.rand(2, 1, 32, 32, 32, generator=g) * 2 - 1 for k in ("t1w", "t2w")}
    return ours, ref, batch


def _cuda(batch):
    return {k: v.cuda() for k, v in batch.items()}


def test_train_eval_train_eval_sees_the_live_statistics():
    """After a real fit_batch the eval result changes and equals the oracle's eval pass on the device's post-step
    state_dict; the eval plan cached before the step is the one reused after it (nothing was baked in)."""
    from oracle import refmodel as R
    ours, _, batch = _gan_a()
    opts, _ = ours.configure_optimizers()
    d = ours.discriminator
    x = batch["t2w"]
    seen = []
    for it in range(3):
        ours.eval()
        v = d(x.cuda())
        ref = R.Discriminator((1, 64, 64), dimensions=2)
        ref.load_state_dict({k: t.detach().cpu() for k, t in d.state_dict().items()})
        ref.eval()
        with torch.no_grad():
            want = ref(x)
        print(f"eval after {it} steps: validity {v.flatten().tolist()}, |ours - oracle| {(v.cpu() - want).abs().max().item():.3e}")
        np.testing.assert_allclose(v.cpu().numpy(), want.numpy(), rtol=0, atol=2e-6)
        seen.append(v.cpu())
        ours.train()
        ours.fit_batch(_cuda(batch), it, opts)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    eval_pools = {k: p for k, p in d._plans.items() if k[0] == "eval"}
    assert len(eval_pools) == 1 and all(len(p) == 1 for p in eval_pools.values()), {k: len(p) for k, p in d._plans.items()}


def _trainer_state(gan, opts):
    st = {}
    for name, net in (("G", gan.generator), ("D", gan.discriminator)):
        st.update({f"{name}.{k}": v for k, v in _state(net).items()})
    for i, o in enumerate(opts):
        st[f"adam{i}.m"], st[f"adam{i}.v"] = o.exp_avg.clone(), o.exp_avg_sq.clone()
        st[f"adam{i}.step"] = torch.tensor(o.step_count)
    return st


@pytest.mark.parametrize("variant", ["A", "B", "B-bf16"])
def test_eval_forward_and_validation_step_write_nothing(variant):
    """store.flat, store.flat_grad, every buffer, both Adam states and every module's training flag are bit-identical
    around an eval forward and around validation_step; a fit_batch after a validation_step gives bit-identical
    parameters to a fit_batch without one (variant B: its training crop stream is untouched)."""
    make = _gan_a if variant == "A" else (lambda: _gan_b(storage_dtype="bf16" if variant == "B-bf16" else "f32"))
    finals = []
    for with_validation in (False, True):
        ours, _, batch = make()
        opts, _ = ours.configure_optimizers()
        cb = _cuda(batch)
        ours.fit_batch(cb, 0, opts)                                   # Adam states and gradients exist from here on
        if with_validation:
            before = _trainer_state(ours, opts)
            out = ours.validation_step(cb, 0)
            _assert_untouched(before, _trainer_state(ours, opts), "validation_step")
            assert set(out) >= {"val_g_adv_loss", "val_g_recon_loss", "val_g_loss", "val_d_loss"}
            assert all(ours.logged[k] is not None and ours.logged[k].is_cuda for k in out)
            again = ours.validation_step(cb, 0)                       # same batch_idx: same crops, bit-identical scalars
            assert all(torch.equal(out[k], again[k]) for k in out), {k: (out[k].item(), again[k].item()) for k in out}
            ours.eval()
            before = _trainer_state(ours, opts)
            x = cb["t2w"] if variant == "A" else cb["t2w"][:, :, :16, :16, :16].contiguous()
            ours.discriminator(x)
            _assert_untouched(before, _trainer_state(ours, opts), "eval forward")
            ours.train()
        ours.fit_batch(cb, 1, opts)
        finals.append(torch.cat([ours.generator.store.flat, ours.discriminator.store.flat]).cpu())
    assert torch.equal(finals[0], finals[1]), (finals[0] - finals[1]).abs().max().item()


def _check_scalars(out, want, what):
    for k, w in want.items():
        got = float(out[k])
        print(f"{what} {k}: ours {got:.7f} oracle {w:.7f} rel diff {abs(got - w) / abs(w):.3e}")
    for k, w in want.items():
        assert abs(float(out[k]) - w) <= 2e-3 * abs(w), (what, k, float(out[k]), w)
    assert set(out) == set(want), (sorted(out), sorted(want))


def _oracle_validation_a(ref, batch, label=0.9):
    from oracle import refmodel as R
    ref.eval()
    with torch.no_grad():
        fake = ref.generator(batch["t1w"])
        d_fake, d_real = ref.discriminator(fake), ref.discriminator(batch["t2w"])
        g_adv = R.adversarial_loss(d_fake, torch.ones_like(d_fake))
        g_rec = R.reconstruction_loss(fake, batch["t2w"])
        d_loss = (R.adversarial_loss(d_real, torch.full_like(d_real, label)) + R.adversarial_loss(d_fake, torch.zeros_like(d_fake))) / 2
    return {"val_g_adv_loss": g_adv.item(), "val_g_recon_loss": g_rec.item(), "val_g_loss": (g_adv + g_rec).item(),
            "val_d_loss": d_loss.item()}


def _warm(ref, batch):
    """One train-mode forward of both oracle networks: non-trivial running statistics for the eval passes."""
    ref.train()
    with torch.no_grad():
        ref.discriminator(batch["t2w"]) if not hasattr(ref, "roi") else ref.discriminator(batch["t2w"][:, :, :16, :16, :16])
        ref.generator(batch["t1w"])


@pytest.mark.parametrize("spatial,bs", [((128, 128), 1), ((128, 128), 2), ((32, 32, 32), 2)], ids=str)
def test_validation_step_variant_a_matches_the_oracle(spatial, bs):
    from mpgan_amd.gan import GAN
    from oracle import refmodel as R
    dims = len(spatial)
    nb = 6 if dims == 2 else 2
    ref = R.GAN((1, *spatial), dimensions=dims, n_unet_blocks=nb)
    R.closed_form_fill_(ref.generator)
    R.closed_form_fill_(ref.discriminator)
    g = torch.Generator().manual_seed(7)
    batch = {k: torch.rand(bs, 1, *spatial, generator=g) * 2 - 1 for k in ("t1w", "t2w")}
    _warm(ref, batch)
    ours = GAN(1, *spatial, dimensions=dims, n_unet_blocks=nb)
    ours.generator.load_state_dict(ref.generator.state_dict())
    ours.discriminator.load_state_dict(ref.discriminator.state_dict())
    ours.train()
    out = ours.validation_step(_cuda(batch), 3)
    assert ours.generator.training and ours.discriminator.training
    assert all(not v.requires_grad and v.is_cuda for v in out.values())
    _check_scalars(out, _oracle_validation_a(ref, batch), f"A {spatial} bs {bs}")


@pytest.mark.parametrize("use_perceptual", [True, False])
def test_validation_step_variant_b_matches_the_oracle(use_perceptual):
    from mpgan_amd.gan_patch import PatchSampler
    from oracle import refmodel as R
    ours, ref, batch = _gan_b(use_perceptual=use_perceptual)
    _warm(ref, batch)
    ours.generator.load_state_dict(ref.generator.state_dict())
    ours.discriminator.load_state_dict(ref.discriminator.state_dict())
    stream_before = ours.patch_transform.R.get_state()[1].copy()
    out = ours.validation_step(_cuda(batch), 2)
    assert np.array_equal(stream_before, ours.patch_transform.R.get_state()[1])      # the training crop stream is untouched
    other = ours.validation_step(_cuda(batch), 3)
    assert not torch.equal(out["val_g_recon_loss"], other["val_g_recon_loss"])       # another batch_idx: other crops
    ref.eval()
    corners = PatchSampler((16, 16, 16), 3, [5, 2]).draw(2, (32, 32, 32))
    with torch.no_grad():
        fake = ref.generator(batch["t1w"])
        fp, rp = R.crop_patches(fake, corners, 16), R.crop_patches(batch["t2w"], corners, 16)
        (d_fake, tf), (d_real, tr) = ref.discriminator(fp), ref.discriminator(rp)
        g_adv = R.adversarial_loss(d_fake, torch.ones_like(d_fake))
        g_rec = R.reconstruction_loss(fp, rp)
        g_loss = g_adv + g_rec
        want = {}
        if use_perceptual:
            perc = R.perceptual_loss(tf, tr)
            want["val_g_perceptual_loss"] = perc.item()
            g_loss = g_loss + perc
        d_loss = (R.adversarial_loss(d_real, torch.full_like(d_real, 0.9)) + R.adversarial_loss(d_fake, torch.zeros_like(d_fake))) / 2
    want.update({"val_g_adv_loss": g_adv.item(), "val_g_recon_loss": g_rec.item(), "val_g_loss": g_loss.item(),
                 "val_d_loss": d_loss.item()})
    _check_scalars(out, want, f"B perceptual={use_perceptual}")


def test_eval_rule_and_reference_checkpoint(tmp_path):
    """Eval mode offers no gradients (the generator's rule): with grad enabled and requires_grad inputs the output is
    detached; `gan.eval(); gan.discriminator(x)` works on a GAN filled by load_reference_checkpoint and uses the loaded
    running statistics."""
    from mpgan_amd.gan import GAN, load_reference_checkpoint
    ours, _, batch = _gan_a()
    opts, _ = ours.configure_optimizers()
    ours.fit_batch(_cuda(batch), 0, opts)                             # non-trivial running statistics
    path = os.path.join(tmp_path, "trainer.ckpt")
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in ours.state_dict().items()}}, path)
    ours.eval()
    x = batch["t2w"].cuda().requires_grad_(True)
    assert torch.is_grad_enabled()
    v = ours.discriminator(x)
    assert v.shape == (2, 1) and not v.requires_grad and v.grad_fn is None
    fresh = GAN(1, 64, 64, dimensions=2, n_unet_blocks=2)
    load_reference_checkpoint(fresh, path)
    fresh.eval()
    v2 = fresh.discriminator(batch["t2w"].cuda())
    assert torch.equal(v2, v)
    assert not torch.equal(v2, GAN(1, 64, 64, dimensions=2, n_unet_blocks=2).eval().discriminator(batch["t2w"].cuda()))
    # training mode is what it was: gradients flow again after .train()
    ours.train()
    assert ours.discriminator(x).requires_grad
