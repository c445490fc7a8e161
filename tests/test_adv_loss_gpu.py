"""mpgan_adv_loss through ops: both objectives on logits against the float64 restatement of tests/adv_loss_ref.py.

Sizes: one element, a wave boundary (63, 64, 65), a block boundary (257, 1025), several blocks with a ragged tail
(1797) and the workload's own map (4 * 26^3).  Bounds (eps = 2^-23), from the formulas -- one exp, one add and one
divide for sigma, then one or two rounded operations; sums in fp64:

    |loss - loss_f64|     <=  8 eps * mean(1 + |z_i|)            bce_logits      8 eps * mean (z_i - t_i)^2        lsgan
    |grad_i - grad_f64,i| <=  8 eps * (1 + |z_i| + t_i) / n      bce_logits     16 eps * (|z_i| + |t_i|) / n       lsgan
"""
import pytest
import torch

import adv_loss_ref as A

pytestmark = pytest.mark.gpu
EPS = A.EPS


def _run(kind, z, t, want_grad=True):
    from mpgan_amd import ops
    n = z.numel()
    part = torch.zeros(ops.adv_loss_partials(n), device="cuda", dtype=torch.float64)
    loss = torch.full((), float("nan"), device="cuda")
    grad = torch.full_like(z, float("nan")) if want_grad else None
    ops.adv_loss(z, t, kind, part, loss, grad)
    return loss, grad


def _bounds(kind, z, t):
    z, t = z.double(), t.double()
    n = z.numel()
    if kind == "bce_logits":
        return 8 * EPS * float((1 + z.abs()).mean()), 8 * EPS * (1 + z.abs() + t) / n
    return 8 * EPS * float(((z - t) ** 2).mean()), 16 * EPS * (z.abs() + t.abs()) / n


def _check(kind, z_cpu, t_cpu, loss, grad, want_loss, want_grad, what):
    loss_bound, grad_bound = _bounds(kind, z_cpu, t_cpu)
    err = abs(float(loss.double().cpu()) - float(want_loss))
    gerr = (grad.double().cpu() - want_grad).abs()
    some = grad_bound > 0                            # (z = t = 0 under lsgan: bound 0, met with equality)
    worst = (gerr[some] / grad_bound[some]).max().item() if bool(some.any()) else 0.0
    print(f"{what}: loss err {err:.3e} bound {loss_bound:.3e}; worst grad err / bound {worst:.3f}")
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    assert err <= loss_bound, (what, err, loss_bound)
    bad = gerr > grad_bound
    assert not bad.any(), (what, int(bad.sum()), z_cpu[bad][:4], t_cpu[bad][:4], gerr[bad][:4], grad_bound[bad][:4])


@pytest.mark.parametrize("n", A.SIZES)
@pytest.mark.parametrize("kind", A.KINDS)
def test_loss_and_gradient_against_float64(kind, n):
    z_cpu, t_cpu = A.inputs(n)
    want_loss, want_grad = A.reference(kind, n)
    z, t = z_cpu.cuda(), t_cpu.cuda()
    loss, grad = _run(kind, z, t)
    _check(kind, z_cpu, t_cpu, loss, grad, want_loss, want_grad, f"{kind} n={n}")
    if kind == "bce_logits":
        # a discriminator that has won: logit -100 / -88 against target 1 keeps the whole gradient -1/n
        lost = ((z_cpu == -100.0) | (z_cpu == -88.0)) & (t_cpu == 1.0)
        assert int(lost.sum()) == (n >= 3) + (n >= 6)
        if lost.any():
            assert (n * grad.double().cpu()[lost] + 1).abs().max().item() <= EPS
    # without the gradient: the same loss bits
    loss_only, none = _run(kind, z, t, want_grad=False)
    assert none is None and torch.equal(loss_only, loss)
    # a second call: the same bits
    loss2, grad2 = _run(kind, z, t)
    assert torch.equal(loss2, loss) and torch.equal(grad2, grad)


@pytest.mark.parametrize("kind", A.KINDS)
def test_unaligned_views_take_the_element_wise_path(kind):
    """Views that start 4 bytes into an allocation: no 16-byte access is possible; same bounds, and the same loss bits
    as the aligned call up to the order of the sum (both within the bound)."""
    n = 1797
    z_cpu, t_cpu = A.inputs(n)
    want_loss, want_grad = A.reference(kind, n)
    from mpgan_amd import ops
    zb, tb, gb = (torch.zeros(n + 1, device="cuda") for _ in range(3))
    z, t, grad = zb[1:], tb[1:], gb[1:]
    z.copy_(z_cpu)
    t.copy_(t_cpu)
    assert z.data_ptr() % 16 == 4 and z.is_contiguous()
    part = torch.zeros(ops.adv_loss_partials(n), device="cuda", dtype=torch.float64)
    loss = torch.full((), float("nan"), device="cuda")
    ops.adv_loss(z, t, kind, part, loss, grad)
    _check(kind, z_cpu, t_cpu, loss, grad, want_loss, want_grad, f"{kind} unaligned n={n}")
    assert float(gb[0]) == 0.0                       # nothing written in front of the view


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("gout", [0.5, -3.0])
def test_autograd_node_scales_the_stored_gradient(kind, gout):
    """backward = gout * grad through scale_by_device_scalar: one fp32 multiplication per element."""
    from mpgan_amd.gan import adversarial_loss
    n = 1797
    z_cpu, t_cpu = A.inputs(n)
    z, t = z_cpu.cuda().requires_grad_(True), t_cpu.cuda()
    loss = adversarial_loss(z, t, kind=kind)
    ref_loss, grad = _run(kind, z.detach(), t)
    assert torch.equal(loss.detach(), ref_loss)
    loss.backward(torch.tensor(gout, device="cuda"))
    want = (grad.double() * gout).float()            # the correctly rounded product
    assert torch.equal(z.grad, want)
    assert z.grad.abs().max().item() > 0
