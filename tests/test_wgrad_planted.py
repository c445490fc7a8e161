"""The comparison of tests/test_wgrad_forms_gpu.py must be able to fail (host only).  For one K-stepped, one patch and
one thin case of its table, "kernel outputs" are built on the CPU from the fp32 reference: the honest one passes both
tiers of wgrad_cases.check, and each planted fault is rejected by the tier named in PLANTED:

  last-pixel   the last pixel of the last sample left out                          tier X
  split-twice  one split's contribution (the first 256 pixels) counted twice       tier X, tier R
  tap-shift    the last tap's gathered column shifted by one pixel                 tier X, tier R
  trunc        MM16 operands truncated to bf16 instead of rounded to nearest even  tier X (operands that need rounding), tier R
  beta         beta applied to dbias but not to dw                                 tier X
"""
import pytest
import torch

import conv_ref as R
import wgrad_cases as W

CASES = {"k-stepped": "mm16-64x64-pro0", "patch": "patch2d-16x16s1-nopro", "thin": "thin-v4-t9"}
PLANTED = [("last-pixel", ("X",)), ("split-twice", ("X", "R")), ("tap-shift", ("X", "R")), ("beta", ("X",))]


def _fp32(c, a, d):
    g = c.g
    return R.conv_backward_weight(a.float(), d.float(), g.k, g.stride, g.pad, g.transposed)


def _operands(c, o):
    """The matrix operands the kernel contracts (fp64 values; an MM16 instance's rounded) and the unrounded dy."""
    a, _ = W.activated(c, o)
    d = o.dy.double()
    return (R.bf16_rne(a), R.bf16_rne(d), d) if c.mm16 else (a, d, d)


def _outputs(c, o, fault, beta):
    """(dw, dbias) a kernel with this fault would leave (fp32 arithmetic throughout)."""
    a, d, d_bias = _operands(c, o)
    dw = _fp32(c, a, d)
    db = R.bias_grad(d_bias.float())
    if fault == "last-pixel":
        d2, db2 = d.clone(), d_bias.clone()
        d2[-1, -1, -1, -1] = 0
        db2[-1, -1, -1, -1] = 0
        dw, db = _fp32(c, a, d2), R.bias_grad(db2.float())
    elif fault == "split-twice":
        first = torch.zeros_like(d).reshape(-1, d.shape[-1])
        first[:256] = d.reshape(-1, d.shape[-1])[:256]
        dw = dw + _fp32(c, a, first.reshape(d.shape))
    elif fault == "tap-shift":
        shifted = _fp32(c, torch.roll(a, 1, dims=3), d)
        dw = dw.clone()
        dw[..., -1, -1, -1] = shifted[..., -1, -1, -1]
    old_w, old_b = beta * o.old_w, beta * o.old_b
    if fault == "beta":
        old_w = torch.zeros_like(old_w)
    return dw + old_w, db + old_b


@pytest.mark.parametrize("form", list(CASES))
def test_honest_outputs_pass_both_tiers(form):
    c = W.BY_ID[CASES[form]]
    assert c.M >= 512 and c.pro is None
    for tier in ("X", "R"):
        o = W.operands(c, tier)
        ref = W.reference(c, o)
        for beta in (0.0, 1.0):
            dw, db = _outputs(c, o, None, beta)
            assert W.check(c, tier, dw, db, W.with_beta(c, o, ref, beta)) == [], (form, tier, beta)


@pytest.mark.parametrize("form", list(CASES))
@pytest.mark.parametrize("fault,tiers", PLANTED, ids=[f for f, _ in PLANTED])
def test_planted_fault_is_rejected(form, fault, tiers):
    c = W.BY_ID[CASES[form]]
    for tier in tiers:
        o = W.operands(c, tier)
        beta = 1.0 if fault == "beta" else 0.0
        want = W.with_beta(c, o, W.reference(c, o), beta)
        dw, db = _outputs(c, o, fault, beta)
        fails = W.check(c, tier, dw, db, want)
        assert any(" dw: " in f for f in fails), (form, fault, tier, fails)
        if fault == "beta":
            assert not any("dbias" in f for f in fails), fails               # dbias itself was right


def test_truncated_mm16_operands_are_rejected():
    c = W.BY_ID[CASES["k-stepped"]]
    assert c.mm16
    for tier in ("X", "R"):
        o = W.operands(c, tier, rounding=(tier == "X"))
        a, _ = W.activated(c, o)
        d = o.dy.double()
        assert not (R.bf16_rne(a) == a).all() and not (R.bf16_rne(d) == d).all()      # the operands do need rounding
        ref = W.reference(c, o)
        honest = _fp32(c, R.bf16_rne(a), R.bf16_rne(d))
        db = R.bias_grad(d.float())
        assert W.check(c, tier, honest, db, ref) == [], tier
        planted = _fp32(c, R.bf16_trunc(a), R.bf16_trunc(d))
        fails = W.check(c, tier, planted, db, ref)
        assert any(" dw: " in f for f in fails), (tier, fails)
        unrounded = _fp32(c, a, d)                                                     # ... and so is no rounding at all
        assert any(" dw: " in f for f in W.check(c, tier, unrounded, db, ref)), tier
