"""Variant B's bf16 storage mode on the GPU: the new kernels (mpgan_tap_l1_bf16, the peer entries of the
bf16 norm backward), the patch discriminator's bf16 plan, variant B's generator in bf16-operand mode and the whole
variant-B step, against the CPU restatement of the same contract (tests/patch_bf16_ref.py) and the fp32 oracle.

Bounds that involve the 16 perceptual taps: the head taps' gradient terms are c*sign(h_fake - h_real) (likewise for
logit and prob) with c up to 1e6/36 at the test shape, so a head output whose fake and real values lie within rounding
of each other moves a gradient by a large step.  Two correct implementations of the same contract (the restatement with
fp32 and with fp64 accumulation, acc64) differ by up to 0.2 in L2 on the head's weight gradient there; that distance is
the yardstick of the head bounds below.  The absolute caps against the fp32 oracle (ABS_CAPS) were fixed, before the
first GPU run, at about twice the restatement's own distance to the fp32 oracle at this shape
(test_patch_bf16_host.py::test_precision_cost_of_bf16_storage_at_the_gpu_test_shape prints it)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import patch_bf16_ref as P
from gpu_helpers import from_cl, to_cl

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PRE_BN_BIAS = ("model_conv.0.bias", "model_conv.3.bias", "model_conv.6.bias", "model_conv.9.bias")
HEAD = ("model_linear.1.weight", "model_linear.1.bias", "model_linear.2.weight", "model_linear.2.bias",
        "model_conv.10.weight", "model_conv.10.bias")
# L2-relative caps against the fp32 oracle at the whole-discriminator test's shape (n = 6, seed 11, real crops
# 0.5*sign(x)*sqrt|x|): about twice the restatement's own distance (CPU figures 0.03 .. 2.9)
ABS_CAPS = {"model_conv.0.weight": 2.1, "model_conv.1.weight": 1.8, "model_conv.1.bias": 2.3,
            "model_conv.3.weight": 2.1, "model_conv.4.weight": 0.7, "model_conv.4.bias": 1.9,
            "model_conv.6.weight": 3.7, "model_conv.7.weight": 5.8, "model_conv.7.bias": 4.4,
            "model_conv.9.weight": 0.45, "model_conv.10.weight": 0.2, "model_conv.10.bias": 0.7,
            "model_linear.1.weight": 0.08, "model_linear.1.bias": 0.08, "model_linear.2.weight": 0.75,
            "model_linear.2.bias": 0.08, "x_fake": 2.1, "x_real": 2.0}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def _dev(t):
    return t.cuda().contiguous()


# ---- 1. mpgan_tap_l1_bf16 -------------------------------------------------------------------------------------
def _tap_ref(za, sa, ha, zb, sb, hb, slope):
    za, zb = za.double(), zb.double()
    ya, yb = za * sa.double() + ha.double(), zb * sb.double() + hb.double()
    aa, ab = torch.where(ya < 0, ya * slope, ya), torch.where(yb < 0, yb * slope, yb)
    return torch.stack([(za - zb).abs().mean(), (ya - yb).abs().mean(), (aa - ab).abs().mean()])


def test_tap_l1_bf16_exact_and_random():
    """bf16-exact inputs (small integers times powers of two, dyadic scale / shift, slope 1/4): every fp32 partial
    sum is exact, so the result equals the fp64 evaluation rounded to fp32 bit for bit.  Random data: 1e-6 relative.
    The result is also reproducible launch to launch (fixed-order reduction)."""
    from mpgan_amd import ops
    gen = torch.Generator().manual_seed(3)
    n, sp, c = 2, (6, 7, 5), 64
    part = torch.empty(ops.tap_l1_partials(), device="cuda")
    za = (torch.randint(-8, 9, (n, *sp, c), generator=gen).float() / 4)
    zb = (torch.randint(-8, 9, (n, *sp, c), generator=gen).float() / 4)
    sa, sb = 2.0 ** torch.randint(-1, 2, (c,), generator=gen).float(), 2.0 ** torch.randint(-1, 2, (c,), generator=gen).float()
    ha, hb = torch.randint(-2, 3, (c,), generator=gen).float() / 4, torch.randint(-2, 3, (c,), generator=gen).float() / 4
    out = torch.empty(3, device="cuda")
    ops.tap_l1_bf16(_dev(za).to(BF), _dev(sa), _dev(ha), _dev(zb).to(BF), _dev(sb), _dev(hb), 0.25, part, out)
    want = _tap_ref(za, sa, ha, zb, sb, hb, 0.25).float()
    assert torch.equal(out.cpu(), want), (out.cpu(), want)
    n, sp, c = 3, (14, 14, 14), 128          # several blocks per channel group, grid capped by the partials size
    za = (torch.randn(n, *sp, c, generator=gen)).to(BF).float()
    zb = (torch.randn(n, *sp, c, generator=gen) * 0.7 + 0.1).to(BF).float()
    sa, sb = torch.rand(c, generator=gen) + 0.5, torch.rand(c, generator=gen) + 0.5
    ha, hb = torch.rand(c, generator=gen) - 0.5, torch.rand(c, generator=gen) - 0.5
    args = (_dev(za).to(BF), _dev(sa), _dev(ha), _dev(zb).to(BF), _dev(sb), _dev(hb), 0.2, part)
    ops.tap_l1_bf16(*args, out)
    want = _tap_ref(za, sa, ha, zb, sb, hb, 0.2)
    np.testing.assert_allclose(out.cpu().double().numpy(), want.numpy(), rtol=1e-6)
    again = torch.empty(3, device="cuda")
    ops.tap_l1_bf16(*args, again)
    assert torch.equal(out, again)


# ---- 2. peer-tap norm backward --------------------------------------------------------------------------------
def _close_bf16(got, ref, what):
    e = (got - ref).abs()
    assert (e <= 8e-3 * ref.abs() + 1e-3 * ref.abs().max()).all(), (what, e.max().item(), ref.abs().max().item())


def _pitched(t_cl, pitch):
    """The channels-last tensor as the first C channels of a `pitch`-channel one (pitch None: as it is)."""
    if pitch is None:
        return t_cl
    wide = torch.zeros(*t_cl.shape[:-1], pitch, dtype=t_cl.dtype, device=t_cl.device)
    wide[..., :t_cl.shape[-1]] = t_cl
    return wide[..., :t_cl.shape[-1]]


def _norm_bwd_gpu(ops, g, z, nbv, peer, slope, g_dtype, coef, pitch=None, bias=True):
    """reduce -> finalize -> apply on the GPU (channels-last); peer None: the entries without peer.  pitch: z, g, the
    peer's z and dz are the leading channels of `pitch`-channel tensors; bias False: apply without bias partials."""
    scale, shift, mean, invstd = (_dev(t) for t in nbv)
    c = z.shape[1]
    rows = z.numel() // c
    brow = ops.norm_bwd_rows_bf16(rows, c)
    part = torch.zeros(brow * 4 * c + c, device="cuda")
    gc, zc = _pitched(to_cl(g).to(g_dtype), pitch), _pitched(to_cl(z).to(BF), pitch)
    if peer is not None:
        pt = ops.PeerTapsBF16(_pitched(to_cl(peer[0]).to(BF), pitch), _dev(peer[1]), _dev(peer[2]),
                              _dev(torch.tensor(coef)))
        ops.norm_bwd_reduce_bf16_peer(gc, zc, scale, shift, mean, invstd, pt, slope, part)
    else:
        ops.norm_bwd_reduce_bf16(gc, zc, scale, shift, mean, invstd, slope, part)
    dgamma, dbeta = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    c1, c2 = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    ops.norm_bwd_finalize(part, 1, brow, c, rows, False, dgamma, dbeta, None, c1, c2)
    dz = _pitched(torch.empty_like(to_cl(z).to(BF)), pitch)
    bias_part = part[brow * 3 * c + c:] if bias else None
    if peer is not None:
        ops.norm_bwd_apply_bf16_peer(gc, zc, scale, shift, mean, invstd, c1, c2, pt, slope, dz, bias_part)
    else:
        ops.norm_bwd_apply_bf16(gc, zc, scale, shift, mean, invstd, c1, c2, slope, dz, bias_part)
    colsum = bias_part.view(brow, c).sum(0).cpu() if bias else None
    return from_cl(dz.float(), 3), dgamma.cpu(), dbeta.cpu(), colsum, dz


# (n, c, spatial, pitch, bias partials).  A block covers R = 256 / (c/8) rows per pass; mpgan_norm_bwd_rows_bf16 gives
# ceil(rows / 32R) blocks.
NORM_BWD_CASES = {
    "c8_3rows": (1, 8, (1, 1, 3), None, True),             # c/8 = 1, R = 256: fewer rows than R
    "c24_R85": (2, 24, (3, 5, 10), None, True),            # c/8 = 3 does not divide 256: R = 85, thread 255 idles
    "c2048_R1": (1, 2048, (1, 5, 7), None, True),          # R = 1, two blocks, the widest the entry admits
    "c64_2blocks": (2, 64, (8, 9, 10), None, True),        # 1440 rows: two blocks, the second only part full
    "c128": (3, 128, (7, 9, 5), None, True),
    "c64_pitch72": (2, 64, (8, 9, 10), 72, True),          # the first 64 channels of 72-channel tensors
    "c64_no_bias": (2, 64, (8, 9, 10), None, False),       # bias_partials=None
}


def _norm_bwd_inputs(n, c, sp, g_dtype):
    """z, the peer's z and g as the kernels read them (g on the grid of its storage dtype), batch statistics of z, an
    affine pair and the peer's scale / shift."""
    gen = torch.Generator().manual_seed(17)
    z = ((torch.rand(n, c, *sp, generator=gen) - 0.4) * 3).to(BF).float()
    zp = ((torch.rand(n, c, *sp, generator=gen) - 0.5) * 3).to(BF).float()
    g = ((torch.rand(n, c, *sp, generator=gen) - 0.5).to(g_dtype).float() * 1e-2).to(g_dtype).float()
    mean = z.transpose(0, 1).reshape(c, -1).mean(1)
    invstd = 1.0 / torch.sqrt(z.transpose(0, 1).reshape(c, -1).var(1, unbiased=False) + 1e-5)
    gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.rand(c, generator=gen) - 0.5
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    sp_, hp_ = torch.rand(c, generator=gen) + 0.5, torch.rand(c, generator=gen) - 0.5
    return z, zp, g, (scale, shift, mean, invstd), (zp, sp_, hp_)


@pytest.mark.parametrize("case", list(NORM_BWD_CASES))
@pytest.mark.parametrize("g_dtype", [BF, torch.float32], ids=["g_bf16", "g_f32"])
def test_peer_norm_backward_bf16(g_dtype, case):
    """The peer entries and the plain entries on bf16 z against the fp64 formula on the same stored tensors, at the
    shapes where their indexing can go wrong (NORM_BWD_CASES): dz within one bf16 ulp (8e-3*|ref| + 1e-3*max|ref|, the
    rule of test_discriminator_bf16_backward_layer_by_layer), dgamma / dbeta within 2e-3 relative L2, the column sums of
    the bias partials against the sum of the stored dz; with all coefficients zero the peer entries' output is
    bit-identical to the entries without peer.  (g is put on the grid of its storage dtype before the reference sees
    it: the reference and the kernels read the same numbers.)"""
    from mpgan_amd import ops
    n, c, sp, pitch, bias = NORM_BWD_CASES[case]
    z, zp, g, nbv, peer = _norm_bwd_inputs(n, c, sp, g_dtype)
    red = [0, 2, 3, 4]
    coef = (3e-3, 2e-3, 4e-3)
    kw = dict(pitch=pitch, bias=bias)
    dz, dgamma, dbeta, colsum, _ = _norm_bwd_gpu(ops, g, z, nbv, peer, 0.2, g_dtype, coef, **kw)
    dz_ref, s1, s2 = P.norm_bwd_peer(g.double(), z, *nbv, 0.2, peer, coef)
    _close_bf16(dz, dz_ref.float(), "dz (peer)")
    assert _rel(dgamma, s2) <= 2e-3 and _rel(dbeta, s1) <= 2e-3, (_rel(dgamma, s2), _rel(dbeta, s1))
    if bias:
        np.testing.assert_allclose(colsum.numpy(), dz.sum(red).numpy(), rtol=1e-3, atol=1e-3)
    # the peer terms are live: the same launch without them is far away
    dz0_ref, s10, s20 = P.norm_bwd_peer(g.double(), z, *nbv, 0.2)
    assert _rel(dz_ref, dz0_ref) > 0.1
    # zero coefficients: bit-identical to the entries without peer
    a = _norm_bwd_gpu(ops, g, z, nbv, peer, 0.2, g_dtype, (0.0, 0.0, 0.0), **kw)
    b = _norm_bwd_gpu(ops, g, z, nbv, None, 0.2, g_dtype, None, **kw)
    assert torch.equal(a[4], b[4]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    if bias:
        assert torch.equal(a[3], b[3])
    # the entries without peer against the formula without peer terms
    _close_bf16(b[0], dz0_ref.float(), "dz (plain)")
    assert _rel(b[1], s20) <= 2e-3 and _rel(b[2], s10) <= 2e-3, (_rel(b[1], s20), _rel(b[2], s10))
    if bias:
        np.testing.assert_allclose(b[3].numpy(), b[0].sum(red).numpy(), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("g_dtype", [BF, torch.float32], ids=["g_bf16", "g_f32"])
@pytest.mark.parametrize("which", ["z", "g", "dz"])
def test_plain_norm_backward_bf16_refuses_misaligned_views(which, g_dtype):
    """The entries without peer read and write z, g and dz with 16-byte accesses like the peer entries, and refuse like
    them: a view offset by one element is a RuntimeError that names the alignment rule, raised before any launch (the
    NaN-filled outputs stay as they were)."""
    from mpgan_amd import ops
    n, c, sp = 2, 24, (1, 5, 7)
    z, _, g, nbv, _ = _norm_bwd_inputs(n, c, sp, g_dtype)
    scale, shift, mean, invstd = (_dev(t) for t in nbv)

    def view(t, shifted):
        base = torch.zeros(t.numel() + 8, dtype=t.dtype, device="cuda")
        v = base[1 if shifted else 0:][:t.numel()].view(t.shape)
        v.copy_(t)
        return v

    zc, gc = view(to_cl(z).to(BF), which == "z"), view(to_cl(g).to(g_dtype), which == "g")
    rows = z.numel() // c
    brow = ops.norm_bwd_rows_bf16(rows, c)
    part = torch.full((brow * 3 * c + c,), float("nan"), device="cuda")
    bias_part = torch.full((brow * c,), float("nan"), device="cuda")
    c1, c2 = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    dz = view(torch.full_like(to_cl(z).to(BF), float("nan")), which == "dz")
    if which != "dz":
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ops.norm_bwd_reduce_bf16(gc, zc, scale, shift, mean, invstd, 0.2, part)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.norm_bwd_apply_bf16(gc, zc, scale, shift, mean, invstd, c1, c2, 0.2, dz, bias_part)
    torch.cuda.synchronize()
    assert torch.isnan(part).all() and torch.isnan(bias_part).all() and torch.isnan(dz.float()).all()
    # the same tensors at aligned addresses are served
    zc, gc, dz = view(zc, False), view(gc, False), view(dz, False)
    ops.norm_bwd_reduce_bf16(gc, zc, scale, shift, mean, invstd, 0.2, part)
    ops.norm_bwd_apply_bf16(gc, zc, scale, shift, mean, invstd, c1, c2, 0.2, dz, bias_part)
    torch.cuda.synchronize()
    assert torch.isfinite(part[:brow * 3 * c]).all() and torch.isfinite(bias_part).all() and torch.isfinite(dz.float()).all()


# ---- 3. / 4. / 7. the whole patch discriminator ----------------------------------------------------------------
def _inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    xf = torch.rand(n, 1, 16, 16, 16, generator=gen) * 2 - 1
    xr = torch.rand(n, 1, 16, 16, 16, generator=gen) * 2 - 1
    return xf, 0.5 * xr.sign() * xr.abs().sqrt()      # real crops of another distribution: head outputs kept apart


def _oracle_disc():
    from oracle import refmodel as R
    ref = R.PatchDiscriminator((1, 16, 16, 16))
    R.closed_form_fill_(ref)
    ref.train()
    return ref, R


def _ours(ref, keep=False):
    from mpgan_amd.networks import PatchDiscriminator
    d = PatchDiscriminator((1, 16, 16, 16), storage_dtype="bf16")
    d.load_state_dict(ref.state_dict())
    d.cuda().train()
    d.debug_keep_intermediates = keep
    return d


def _run_pair(d, xf, xr, w_perc=1e6):
    from mpgan_amd.gan import adversarial_loss
    from mpgan_amd.gan_patch import perceptual_loss
    xfc, xrc = xf.cuda().requires_grad_(True), xr.cuda().requires_grad_(True)
    v, tf = d(xfc)
    _, tr = d(xrc)
    pf, pr = tf.tapset.plan, tr.tapset.plan
    perc = perceptual_loss(tf, tr)
    bce = adversarial_loss(v, torch.ones_like(v))
    loss = w_perc * perc.sum() + bce
    loss.backward()
    return dict(validity=v.detach().cpu(), perceptual=perc.item(), bce=bce.item(), loss=loss.item(), pf=pf, pr=pr,
                grads={k: p.grad.cpu() for k, p in d.named_parameters()}, grad_x_fake=xfc.grad.cpu(),
                grad_x_real=xrc.grad.cpu(), tf=tf, tr=tr)


def test_patch_discriminator_bf16_matches_its_restatement():
    """Fake and real passes (n = 6 crops of 16^3, closed-form weights), backward of 1e6*perceptual + BCE, against the
    restatement: validity and loss within 2e-3, the perceptual value within 2e-3 relative, every stored z_i within
    5e-3 relative L2; the head's and the last BatchNorm's gradients within 1e-2 + 2x the acc64 yardstick (see the
    module docstring), every other gradient within the restatement's distance to the fp32 oracle + 2e-2 -- these two
    with the head taps' sign decisions (sign of fake - real of h, logit, prob) taught to the restatement; and every
    gradient within ABS_CAPS of the fp32 oracle when those decisions agree with the restatement's own."""
    from test_patch_bf16_host import oracle_fp32
    ref, R = _oracle_disc()
    xf, xr = _inputs(6, 11)
    o = oracle_fp32(ref, R, xf, xr)
    ours = _run_pair(_ours(ref), xf, xr)
    # the head taps' sign decisions of OUR passes, taught to the restatement (see the module docstring)
    signs = {k: torch.sign(getattr(ours["pf"], k).reshape(6, -1).cpu() - getattr(ours["pr"], k).reshape(6, -1).cpu())
             for k in ("h", "logit", "prob")}
    r = P.pair_step(ref, xf, xr, head_signs=signs)
    r64 = P.pair_step(ref, xf, xr, acc64=True, head_signs=signs)
    r_own = P.pair_step(ref, xf, xr)
    np.testing.assert_allclose(ours["validity"].numpy(), r["validity"].numpy(), atol=2e-3)
    assert abs(ours["bce"] - r["bce"].item()) <= 2e-3 * abs(r["bce"].item())
    yard_p = abs(r64["perceptual"].item() / r["perceptual"].item() - 1)
    e_p = abs(ours["perceptual"] / r["perceptual"].item() - 1)
    print(f"perceptual: ours vs restatement {e_p:.2e} (acc64 yardstick {yard_p:.2e})")
    assert e_p <= 2e-3 + 2 * yard_p
    assert abs(ours["loss"] / r["loss"].item() - 1) <= 2e-3 + 2 * yard_p
    for i in range(4):
        for plan, zs in ((ours["pf"], r["zs_fake"]), (ours["pr"], r["zs_real"])):
            e = _rel(from_cl(plan.zs[i].float(), 3), zs[i])
            assert e <= 5e-3, (i, e)
    errs, cost, yard = {}, {}, {}
    for name in o["grads"]:
        if name in PRE_BN_BIAS:
            continue
        errs[name] = _rel(ours["grads"][name], r["grads"][name])
        cost[name] = _rel(r["grads"][name], o["grads"][name])
        yard[name] = _rel(r64["grads"][name], r["grads"][name])
    for s in ("fake", "real"):
        k = "grad_x_" + s
        errs["x_" + s], cost["x_" + s], yard["x_" + s] = _rel(ours[k], r[k]), _rel(r[k], o[k]), _rel(r64[k], r[k])
    print("ours vs bf16 restatement:", {k: round(e, 4) for k, e in errs.items()})
    print("acc64 yardstick:", {k: round(e, 4) for k, e in yard.items()})
    print("restatement vs fp32 oracle (precision cost):", {k: round(e, 4) for k, e in cost.items()})
    for name, e in errs.items():
        bound = 1e-2 + 2 * yard[name] if name in HEAD else cost[name] + 2e-2
        assert e <= bound, (name, e, bound)
    # head-tap sign flips between our passes and the restatement's own: a sample whose fake and real logit (or prob)
    # lie within the two sides' forward difference takes the opposite +-1e6/36 step, which moves every gradient by
    # O(1) -- then the fp32 oracle's signs differ from ours as well and its caps do not apply (the kink-flip rule of
    # test_variant_b_gpu.py, applied to the perceptual loss's sign terms)
    flips = sum(int((signs[k] != torch.sign(r_own["taps_fake"][t] - r_own["taps_real"][t]).reshape(6, -1)).sum())
                for k, t in (("logit", 14), ("prob", 15)))
    print("head-tap sign flips against the restatement's own (logit, prob):", flips)
    vs_oracle = {k: _rel(ours["grads"][k], o["grads"][k]) for k in o["grads"] if k not in PRE_BN_BIAS}
    vs_oracle["x_fake"], vs_oracle["x_real"] = _rel(ours["grad_x_fake"], o["grad_x_fake"]), _rel(ours["grad_x_real"], o["grad_x_real"])
    print("ours vs fp32 oracle:", {k: round(e, 4) for k, e in vs_oracle.items()})
    if flips == 0:
        for name, e in vs_oracle.items():
            assert e <= ABS_CAPS[name], (name, e, ABS_CAPS[name])
    assert (ours["validity"] - o["validity"]).abs().max().item() <= 2e-3


def test_patch_discriminator_bf16_backward_layer_by_layer():
    """The backward checked one layer at a time on the tensors the HIP path itself stored (teacher forcing), the peer
    terms included: per layer and pass, the fp64 formula on the GPU's incoming gradient, stored z, statistics, peer z
    and coefficients; dz and the data gradients within one bf16 ulp, the BatchNorm and conv weight gradients (both
    passes summed) within 2e-3 relative L2, the crops' gradients within 2e-3."""
    ref, _ = _oracle_disc()
    xf, xr = _inputs(4, 12)
    d = _ours(ref, keep=True)
    ours = _run_pair(d, xf, xr)
    convs = [ref.model_conv[i] for i in (0, 3, 6, 9)]
    conv_w = [cv.weight.detach() if i == 0 else P.rb(cv.weight.detach()) for i, cv in enumerate(convs)]
    grads = ours["grads"]
    red = [0, 2, 3, 4]
    sums = {}
    for plan, other, x, gx in ((ours["pf"], ours["pr"], xf, ours["grad_x_fake"]), (ours["pr"], ours["pf"], xr, ours["grad_x_real"])):
        for i in range(3, -1, -1):
            nb, pnb = plan.nbs[i], other.nbs[i]
            z = from_cl(plan.zs[i].float(), 3)
            g_in = from_cl(plan.gas[i].float(), 3) if i < 3 else from_cl(plan.gas[3], 3)
            coef = tuple(plan.coef[i][:3].cpu().tolist())
            dz_ref, s1, s2 = P.norm_bwd_peer(g_in.double(), z, *(t.cpu() for t in (nb.scale, nb.shift, nb.mean, nb.invstd)),
                                             0.2, (from_cl(other.zs[i].float(), 3), pnb.scale.cpu(), pnb.shift.cpu()), coef)
            dz = from_cl(plan.dzs[i].float(), 3)
            _close_bf16(dz, dz_ref.float(), f"dz{i}")
            a_in = x if i == 0 else from_cl(plan.acts[i - 1].float(), 3)
            a_req, w_req = a_in.double().requires_grad_(True), conv_w[i].double().requires_grad_(True)
            ga, gw = torch.autograd.grad(F.conv3d(a_req, w_req), (a_req, w_req), dz.double())
            for k, v in ((f"s1_{i}", s1), (f"s2_{i}", s2), (f"w{i}", gw), (f"b{i}", dz.double().sum(red)),
                         (f"m{i}", dz.double().abs().sum(red))):
                sums[k] = sums.get(k, 0) + v
            if i > 0:
                _close_bf16(from_cl(plan.gas[i - 1].float(), 3), P.rb(ga.float()), f"ga{i - 1}")
            else:
                assert _rel(gx, ga) <= 2e-3, ("dx", _rel(gx, ga))
    for i in range(4):
        assert _rel(grads[f"model_conv.{3 * i + 1}.weight"], sums[f"s2_{i}"]) <= 2e-3, i
        assert _rel(grads[f"model_conv.{3 * i + 1}.bias"], sums[f"s1_{i}"]) <= 2e-3, i
        assert _rel(grads[f"model_conv.{3 * i}.weight"], sums[f"w{i}"]) <= 2e-3, i
        if i > 0:     # (pre-BatchNorm biases: sums of the stored dz, which cancel to rounding noise)
            e = (grads[f"model_conv.{3 * i}.bias"].double() - sums[f"b{i}"]).abs()
            assert (e <= 1e-5 * sums[f"m{i}"] + 1e-3 * sums[f"b{i}"].abs().max()).all(), (i, e.max().item())


def test_materialised_taps_in_bf16_mode():
    """TapSet.materialize in bf16 mode: fp32 NC(D)HW tensors of the stored z (z exactly; y and a from the stored z
    within 1e-6), close to the restatement's taps (5e-3 + 3x the acc64 yardstick in relative L2: the head taps are
    differences of 262,144-term dot products of bf16-noisy activations); a gradient deposited into a
    materialised tap raises NotImplementedError naming the fused perceptual loss."""
    ref, _ = _oracle_disc()
    xf, _ = _inputs(3, 13)
    d = _ours(ref)
    _, taps = d(xf.cuda())
    r, r64 = P.forward(ref, xf), P.forward(ref, xf, acc64=True)
    plan = taps.tapset.plan
    for k in range(16):
        t = taps.tapset.materialize(k).cpu()
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(r["taps"][k].shape), k
        e, yard = _rel(t, r["taps"][k]), _rel(r64["taps"][k], r["taps"][k])
        assert e <= 5e-3 + 3 * yard, (k, e, yard)
        if k < 12:
            i, kind = divmod(k, 3)
            z = from_cl(plan.zs[i].float(), 3)
            sc, sh = plan.nbs[i].scale.cpu().view(1, -1, 1, 1, 1), plan.nbs[i].shift.cpu().view(1, -1, 1, 1, 1)
            y = z * sc + sh
            want = z if kind == 0 else (y if kind == 1 else torch.where(y < 0, y * 0.2, y))
            if kind == 0:
                assert torch.equal(t, want)
            else:
                assert (t - want).abs().max().item() <= 1e-6 * want.abs().max().item() + 1e-7, k
    xg = xf.cuda().requires_grad_(True)
    _, taps = d(xg)
    with pytest.raises(NotImplementedError, match="perceptual_loss"):
        taps[4].abs().sum().backward()


# ---- 5. variant B's generator in bf16-operand mode --------------------------------------------------------------
def test_variant_b_generator_bf16_matmul():
    """CasNetGenerator(channels (32, 64, 128, 256), strides (2, 2, 2, 2), matmul_dtype="bf16") at 32^3, forward and
    backward, against oracle.mm16_emul.apply_mm16 of the oracle generator (tests/test_c5_step_gpu.py's rule: output L1
    within 2x the emulation's distance to fp32 + 1e-4, gradients within 2x + 2e-2 in L2)."""
    import copy
    from mpgan_amd.networks import CasNetGenerator
    from oracle import mm16_emul as M
    from oracle import refmodel as R
    kw = dict(dimensions=3, channels=(32, 64, 128, 256), strides=(2, 2, 2, 2))
    rg = R.CasNetGenerator((1, 32, 32, 32), 1, **kw)
    R.closed_form_fill_(rg)
    rg.train()
    pure = copy.deepcopy(rg)
    M.apply_mm16(rg)
    g = CasNetGenerator((1, 32, 32, 32), 1, matmul_dtype="bf16", **kw)
    g.load_state_dict(pure.state_dict())
    g.cuda().train()
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(2, 1, 32, 32, 32, generator=gen) * 2 - 1
    t = torch.rand(2, 1, 32, 32, 32, generator=gen) * 2 - 1
    y_ref, y_pure = rg(x), pure(x)
    F.l1_loss(y_ref, t).backward()
    F.l1_loss(y_pure, t).backward()
    y = g(x.cuda())
    F.l1_loss(y, t.cuda()).backward()
    e_y, cost_y = (y.detach().cpu() - y_ref.detach()).abs().mean().item(), (y_ref - y_pure).abs().mean().item()
    print(f"G output L1: ours vs emulation {e_y:.3e}; emulation vs fp32 {cost_y:.3e}")
    assert e_y <= 2 * cost_y + 1e-4, (e_y, cost_y)
    rp, pp = dict(rg.named_parameters()), dict(pure.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in rp.values())
    for name, p in g.named_parameters():
        e, cost = _rel(p.grad.cpu(), rp[name].grad), _rel(rp[name].grad, pp[name].grad)
        tiny = (p.grad.cpu() - rp[name].grad).abs().max().item() <= 5e-4 * gmax
        assert e <= 2 * cost + 2e-2 or tiny, (name, e, cost)


# ---- 6. the full variant-B step ---------------------------------------------------------------------------------
def test_variant_b_bf16_steps_match_restatement():
    """G step and D step of GAN(storage_dtype="bf16", matmul_dtype="f32") at 2 x 32^3 with 3 crops (the shape of
    test_variant_b_steps_match_oracle) against the fp32 oracle generator + the restatement of the bf16 discriminator
    on the same corners: losses within 2e-3 (the perceptual value within 2e-3 + 2x its acc64 yardstick), the
    discriminator's gradients within 2x the restatement's distance to the fp32 oracle + 2e-2 in L2
    (test_c5_step_gpu.py's rule for gradients through a bf16-storage discriminator), the generator's within 2x (that
    distance + the acc64 yardstick) + 2e-2: they carry the discriminator's input gradient, whose noise between two
    correct orders of the same contract (acc64) is of the size of the precision cost itself at this shape."""
    from mpgan_amd.gan_patch import GAN
    from oracle import refmodel as R
    kw = dict(n_unet_blocks=1, channels=(8, 16, 32), strides=(2, 2))
    ref = R.PatchGAN((1, 32, 32, 32), num_samples=3, crop_seed=5, **kw)
    R.closed_form_fill_(ref.generator)
    R.closed_form_fill_(ref.discriminator)
    ref.train()
    ours = GAN(1, 32, 32, 32, n_unet_blocks=1, unet_channels=(8, 16, 32), unet_strides=(2, 2), num_samples=3,
               crop_seed=5, storage_dtype="bf16", matmul_dtype="f32")
    ours.generator.load_state_dict(ref.generator.state_dict())
    ours.discriminator.load_state_dict(ref.discriminator.state_dict())
    ours.train()
    gen = torch.Generator().manual_seed(8)
    batch = {"t1w": torch.rand(2, 1, 32, 32, 32, generator=gen) * 2 - 1,
             "t2w": torch.rand(2, 1, 32, 32, 32, generator=gen) * 2 - 1}
    cb = {k: v.cuda() for k, v in batch.items()}
    rd = ref.discriminator
    # ---- G step: oracle generator, restatement discriminator (w_perc = 1), same corners
    for p in list(rd.parameters()) + list(ours.discriminator.parameters()):
        p.requires_grad_(False)
    corners = R.draw_corners(np.random.RandomState(5), 2, 3, (32, 32, 32), 16)
    y = ref.generator(batch["t1w"])
    fake_p, real_p = R.crop_patches(y, corners, 16), R.crop_patches(batch["t2w"], corners, 16)
    fpd = fake_p.detach()
    r = P.pair_step(rd, fpd, real_p, w_perc=1.0)
    o = P.pair_step(rd, fpd, real_p, w_perc=1.0, rounding=False)
    r64 = P.pair_step(rd, fpd, real_p, w_perc=1.0, acc64=True)
    recon = F.l1_loss(fake_p, real_p)
    g_fake = torch.autograd.grad(recon, fake_p, retain_graph=True)[0]
    fake_p.backward(r["grad_x_fake"] + g_fake, retain_graph=True)
    g_ref = {k: p.grad.clone() for k, p in ref.generator.named_parameters()}
    ref.generator.zero_grad()
    fake_p.backward(o["grad_x_fake"] + g_fake, retain_graph=True)
    g_f32 = {k: p.grad.clone() for k, p in ref.generator.named_parameters()}
    ref.generator.zero_grad()
    fake_p.backward(r64["grad_x_fake"] + g_fake)
    g_64 = {k: p.grad.clone() for k, p in ref.generator.named_parameters()}
    l = ours.training_step(cb, 0, 0)
    l.backward()
    log = {k: float(v) for k, v in ours.logged.items()}
    assert abs(log["g_adv_loss"] - r["bce"].item()) <= 2e-3 * abs(r["bce"].item())
    assert abs(log["g_recon_loss"] - recon.item()) <= 2e-3 * recon.item()
    yard = abs(r64["perceptual"].item() / r["perceptual"].item() - 1)
    assert abs(log["g_perceptual_loss"] / r["perceptual"].item() - 1) <= 2e-3 + 2 * yard, (log, r["perceptual"].item())
    gmax = max(v.abs().max().item() for v in g_ref.values())
    for name, p in ours.generator.named_parameters():
        e, cost, yard = _rel(p.grad.cpu(), g_ref[name]), _rel(g_ref[name], g_f32[name]), _rel(g_64[name], g_ref[name])
        tiny = (p.grad.cpu() - g_ref[name]).abs().max().item() <= 5e-4 * gmax
        assert e <= 2 * (cost + yard) + 2e-2 or tiny, ("G grad " + name, e, cost, yard)
    # ---- D step
    for p in list(rd.parameters()) + list(ours.discriminator.parameters()):
        p.requires_grad_(True)
    for p in list(ref.generator.parameters()) + list(ours.generator.parameters()):
        p.requires_grad_(False)
    ours.discriminator.zero_grad()
    ours.patch_transform.set_random_state(6)
    corners = R.draw_corners(np.random.RandomState(6), 2, 3, (32, 32, 32), 16)
    with torch.no_grad():
        y = ref.generator(batch["t1w"])
    fake_p, real_p = R.crop_patches(y, corners, 16), R.crop_patches(batch["t2w"], corners, 16)
    steps = {}
    for mode, kwr in (("bf16", {}), ("f32", dict(rounding=False))):
        _, lr_, _, gr = P.bce_step(rd, real_p, 0.9, 0.5, **kwr)
        _, lf_, _, gr = P.bce_step(rd, fake_p, 0.0, 0.5, grads=gr, **kwr)
        steps[mode] = ((lr_ + lf_).item() / 2, gr)
    d = ours.training_step(cb, 0, 1)
    d.backward()
    assert abs(d.item() - steps["bf16"][0]) <= 2e-3 * abs(steps["bf16"][0]), (d.item(), steps["bf16"][0])
    for name, p in ours.discriminator.named_parameters():
        if name in PRE_BN_BIAS:
            continue
        e, cost = _rel(p.grad.cpu(), steps["bf16"][1][name]), _rel(steps["bf16"][1][name], steps["f32"][1][name])
        assert e <= 2 * cost + 2e-2, ("D grad " + name, e, cost)


# ---- 8. reference-scale smoke -----------------------------------------------------------------------------------
def test_variant_b_bf16_reference_scale_smoke():
    """GAN(1, 128, 128, 128, storage_dtype="bf16") on 2 volumes with 128 crops each: two fit_batch steps, every logged
    loss finite and, against the fp32 GAN on the same weights, inputs and corners: g_adv_loss, g_recon_loss and d_loss
    within 5e-2 relative, g_perceptual_loss and g_loss within 0.5 relative (the perceptual value's precision cost is
    5-20 % at the small test shape; the second step also differs by the first step's Adam updates of bf16-storage
    gradients).  Bounds written before the first GPU run.  The step time is printed, not asserted."""
    import time
    from mpgan_amd.gan_patch import GAN
    torch.manual_seed(0)
    sd = None
    logs, times = {}, {}
    gen = torch.Generator().manual_seed(2)
    batch = {"t1w": (torch.rand(2, 1, 128, 128, 128, generator=gen) * 2 - 1).cuda(),
             "t2w": (torch.rand(2, 1, 128, 128, 128, generator=gen) * 2 - 1).cuda()}
    for mode in ("f32", "bf16"):
        torch.manual_seed(0)
        m = GAN(1, 128, 128, 128, storage_dtype=mode, crop_seed=4)
        if sd is None:
            sd = {k: v.clone() for k, v in m.state_dict().items()}
        m.load_state_dict(sd)
        m.train()
        opts, _ = m.configure_optimizers()
        out = []
        for step in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out.append({k: float(v) for k, v in m.fit_batch(batch, step, opts).items()})
            torch.cuda.synchronize()
            times[(mode, step)] = time.perf_counter() - t0
        logs[mode] = out
        del m, opts
    print("step times (s):", {k: round(v, 3) for k, v in times.items()})
    print("losses:", logs)
    for step in range(2):
        a, b = logs["bf16"][step], logs["f32"][step]
        for k, v in a.items():
            assert np.isfinite(v), (step, k, v)
            tol = 0.5 if k in ("g_perceptual_loss", "g_loss") else 5e-2
            assert abs(v - b[k]) <= tol * abs(b[k]) + 1e-6, (step, k, v, b[k])
