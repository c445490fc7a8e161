"""Variant B's bf16 storage mode without a GPU: the CPU restatement (tests/patch_bf16_ref.py) pinned to the fp32 oracle
with its rounding off, the constructors' dtype options, and the precision cost of bf16 storage at the shapes of
tests/test_patch_bf16_gpu.py (the GPU tests' absolute caps against the fp32 oracle were fixed from these figures)."""
import pytest
import torch
import torch.nn.functional as F

import patch_bf16_ref as P

PRE_BN_BIAS = ("model_conv.0.bias", "model_conv.3.bias", "model_conv.6.bias", "model_conv.9.bias")


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def _oracle_pair(n, seed):
    from oracle import refmodel as R
    ref = R.PatchDiscriminator((1, 16, 16, 16))
    R.closed_form_fill_(ref)
    ref.train()
    gen = torch.Generator().manual_seed(seed)
    xf = torch.rand(n, 1, 16, 16, 16, generator=gen) * 2 - 1
    xr = torch.rand(n, 1, 16, 16, 16, generator=gen) * 2 - 1
    return ref, R, xf, xr


def oracle_fp32(ref, R, xf, xr, w_perc=1e6):
    """oracle.refmodel under autograd: validity, taps, perceptual value, loss, parameter and input gradients."""
    ref.zero_grad()
    xf_, xr_ = xf.clone().requires_grad_(True), xr.clone().requires_grad_(True)
    vf, af = ref(xf_)
    _, ar = ref(xr_)
    perc = R.perceptual_loss(af, ar)
    bce = R.adversarial_loss(vf, torch.ones_like(vf))
    loss = w_perc * perc.sum() + bce
    loss.backward()
    return dict(validity=vf.detach(), taps_fake={k: v.detach() for k, v in af.items()},
                taps_real={k: v.detach() for k, v in ar.items()}, perceptual=perc.detach(), bce=bce.detach(),
                loss=loss.detach(), grads={k: p.grad.clone() for k, p in ref.named_parameters()},
                grad_x_fake=xf_.grad, grad_x_real=xr_.grad)


def precision_cost(ref, o, r):
    """L2-relative distance restatement -> fp32 oracle per gradient tensor (pre-BatchNorm biases skipped)."""
    cost = {k: _rel(r["grads"][k], o["grads"][k]) for k in o["grads"] if k not in PRE_BN_BIAS}
    cost["x_fake"] = _rel(r["grad_x_fake"], o["grad_x_fake"])
    cost["x_real"] = _rel(r["grad_x_real"], o["grad_x_real"])
    return cost


def test_restatement_without_rounding_reproduces_the_fp32_oracle():
    """rounding=False: the restatement is the fp32 network -- forward, the 16 taps, the perceptual value and every
    gradient of 1e6*perceptual + BCE (both passes, both inputs) against oracle.refmodel under autograd, at fp32
    noise.  The perceptual value is held to 1e-3: its head terms are means of |logit_real - logit_fake| over two
    elements, differences of nearly equal fp32 dot products.  Gradients to 2e-3 in L2 when no BatchNorm output changes
    sign between the two (seed 7 has none; a LeakyReLU kink flip within fp32 noise of zero moves the input gradient
    by percents, see test_variant_b_gpu._kink_flips), 5e-2 otherwise."""
    ref, R, xf, xr = _oracle_pair(2, 7)
    o = oracle_fp32(ref, R, xf, xr)
    r = P.pair_step(ref, xf, xr, rounding=False)
    torch.testing.assert_close(r["validity"], o["validity"], rtol=1e-5, atol=1e-6)
    for k in range(16):
        assert _rel(r["taps_fake"][k], o["taps_fake"][k]) <= 2e-5, ("fake tap", k)
        assert _rel(r["taps_real"][k], o["taps_real"][k]) <= 2e-5, ("real tap", k)
    assert abs(r["perceptual"].item() - o["perceptual"].item()) <= 1e-3 * abs(o["perceptual"].item())
    assert abs(r["loss"].item() - o["loss"].item()) <= 1e-3 * abs(o["loss"].item())
    flips = sum(int(((r[s][k] > 0) != (o[s][k] > 0)).sum()) for s in ("taps_fake", "taps_real") for k in (1, 4, 7, 10))
    tol = 2e-3 if flips == 0 else 5e-2
    for name, g in o["grads"].items():
        if name in PRE_BN_BIAS:
            assert r["grads"][name].abs().max() <= 1e-3 * max(v.abs().max() for v in o["grads"].values())
            continue
        assert _rel(r["grads"][name], g) <= tol, (name, _rel(r["grads"][name], g), flips)
    assert _rel(r["grad_x_fake"], o["grad_x_fake"]) <= tol
    assert _rel(r["grad_x_real"], o["grad_x_real"]) <= tol


def test_restatement_rounds_where_the_hip_path_stores():
    """rounding=True: every stored z_i is bf16-exact, the taps are defined on it, and the acc64 run (another
    accumulation order of the same contract) stays close on the forward."""
    ref, R, xf, xr = _oracle_pair(2, 4)
    r = P.pair_step(ref, xf, xr)
    for z in r["zs_fake"] + r["zs_real"]:
        assert torch.equal(z, z.to(torch.bfloat16).float())
    for i in range(4):
        assert torch.equal(r["taps_fake"][3 * i], r["zs_fake"][i])
    r64 = P.pair_step(ref, xf, xr, acc64=True)
    assert _rel(r64["validity"], r["validity"]) <= 1e-2
    for a, b in zip(r64["zs_fake"], r["zs_fake"]):
        assert _rel(a, b) <= 5e-3


def test_constructor_dtype_options():
    """With device=None nothing touches a GPU."""
    from mpgan_amd.gan_patch import GAN
    from mpgan_amd.networks import PatchDiscriminator
    with pytest.raises(ValueError):
        PatchDiscriminator((1, 16, 16, 16), storage_dtype="fp16")
    assert PatchDiscriminator((1, 16, 16, 16)).storage_dtype == "f32"
    assert PatchDiscriminator((1, 16, 16, 16), storage_dtype="bf16").storage_dtype == "bf16"
    kw = dict(n_unet_blocks=1, unet_channels=(8, 16, 32), unet_strides=(2, 2), device=None)
    with pytest.raises(ValueError):
        GAN(1, 32, 32, 32, storage_dtype="bf8", **kw)
    with pytest.raises(ValueError):
        GAN(1, 32, 32, 32, matmul_dtype="tf32", **kw)
    g = GAN(1, 32, 32, 32, **kw)
    assert (g.discriminator.storage_dtype, g.generator.matmul_dtype) == ("f32", "f32")
    g = GAN(1, 32, 32, 32, storage_dtype="bf16", **kw)
    assert (g.discriminator.storage_dtype, g.generator.matmul_dtype) == ("bf16", "bf16")
    g = GAN(1, 32, 32, 32, storage_dtype="bf16", matmul_dtype="f32", **kw)
    assert (g.discriminator.storage_dtype, g.generator.matmul_dtype) == ("bf16", "f32")
    g = GAN(1, 32, 32, 32, storage_dtype="f32", matmul_dtype="bf16", **kw)
    assert (g.discriminator.storage_dtype, g.generator.matmul_dtype) == ("f32", "bf16")


def test_precision_cost_of_bf16_storage_at_the_gpu_test_shape():
    """The restatement's distance to the fp32 oracle at the shape of test_patch_bf16_gpu.py's whole-discriminator test
    (n = 6 crops of 16^3, closed-form weights, seed 11, real crops 0.5*sign(x)*sqrt|x|, 1e6*perceptual + BCE).
    Printed; the GPU test's absolute caps against the fp32 oracle (ABS_CAPS there) were set from these figures, about
    2x above them.  The cost is O(1) on the conv gradients: the head taps' sign terms (c up to 1e6/36) flip where a
    fake and a real head output lie within bf16 noise of each other."""
    ref, R, xf, xr = _oracle_pair(6, 11)
    xr = 0.5 * xr.sign() * xr.abs().sqrt()
    o = oracle_fp32(ref, R, xf, xr)
    r = P.pair_step(ref, xf, xr)
    cost = precision_cost(ref, o, r)
    fwd = dict(validity=(r["validity"] - o["validity"]).abs().max().item(),
               perceptual=abs(r["perceptual"].item() / o["perceptual"].item() - 1),
               loss=abs(r["loss"].item() / o["loss"].item() - 1))
    print("bf16 restatement vs fp32 oracle, forward:", {k: f"{v:.2e}" for k, v in fwd.items()})
    print("bf16 restatement vs fp32 oracle, gradients (L2 rel):", {k: round(v, 4) for k, v in cost.items()})
    assert fwd["validity"] <= 2e-3 and fwd["perceptual"] <= 0.2, fwd
    assert max(cost.values()) <= 3.0, cost
