"""mpgan_amd.losses.ssim_loss on the MI355X against the float64 torch restatement (ssim_loss_ref.py).

Both kernels tile y-x as 8 x 32 and z as 4 (the forward over window corners, the backward over samples), so the
shapes the definition's issue lists cross every tile edge; case "h" adds a volume that spans two tiles with a ragged
remainder on every axis of both launches (corners 7 x 11 x 35, samples 13 x 17 x 41); case "i" gives an item more
forward tiles than the 256 threads of the block that adds them (the loss alone, under every reduction).

The bound, for the loss and for each gradient (max-abs over the tensor):

    err(ours, f64) <= 4 * err(torch fp32 on the CPU, f64) + 2e-6 * max|f64 reference|

The factor 4 is the margin for a different fp32-or-better summation order; the additive term covers the fp32 rounding
of our outputs where torch's fp32 run happens to land on the fp64 value.  Every case prints both errors under -s."""
import functools

import pytest
import torch

import ssim_loss_ref as R
from mpgan_amd import losses, metrics

pytestmark = pytest.mark.gpu

CASES = {
    "a": (1, 1, 7, 7),             # a single 2-D window, M = 1
    "b": (2, 1, 9, 39),            # crosses the 32-wide x tile by a ragged 1
    "c": (1, 2, 17, 45),           # channel items; two y tiles
    "d": (1, 1, 7, 7, 7),          # a single 3-D window
    "e": (1, 1, 9, 10, 40),        # 3-D, ragged on every axis
    "f": (2, 1, 13, 21, 37),       # 3-D
    "g": (1, 1, 21, 37),           # passed at a storage offset of one element: data_ptr % 16 == 4
    "h": (1, 1, 13, 17, 41),       # two tiles and a ragged remainder on every axis, forward and backward
    "i": (2, 2, 136, 544),         # 17 x 17 = 289 forward tiles per item: the item kernel's 256-stride loop wraps (loss only)
}
GRAD_CASES = [case for case in CASES if case != "i"]
RANGE = (-1.0, 1.0)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return R.structured_pair(CASES[case], seed=20 + ord(case))


def _dev(x, case=""):
    """The tensor on the device; case g as a contiguous view one element into a larger buffer."""
    if case == "g":
        buf = torch.empty(x.numel() + 1, device="cuda")
        view = buf[1:].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view
    return x.cuda()


@functools.lru_cache(maxsize=None)
def _reference(case, reduction="mean"):
    """(loss, grad_pred, grad_target) in fp64 and in fp32, computed once per configuration on the CPU."""
    pred, target = _inputs(case)
    kw = dict(value_range=RANGE, reduction=reduction)
    return (R.loss_and_gradients(pred, target, dtype=torch.float64, **kw),
            R.loss_and_gradients(pred, target, dtype=torch.float32, **kw))


def _bound(name, got, f64, f32):
    got, f64, f32 = got.detach().double().cpu(), f64.double(), f32.double()
    ours, peer = float((got - f64).abs().max()), float((f32 - f64).abs().max())
    scale = float(f64.abs().max())
    limit = 4.0 * peer + 2e-6 * scale
    print(f"{name}: err ours {ours:.3e}  torch-fp32 {peer:.3e}  max|ref| {scale:.3e}  limit {limit:.3e}")
    assert ours <= limit, (name, ours, peer, scale, limit)


def _run(case, reduction="mean", grad=(True, True)):
    pred, target = _inputs(case)
    p, t = _dev(pred, case).requires_grad_(grad[0]), _dev(target, case).requires_grad_(grad[1])
    return p, t, losses.SSIMLoss(RANGE, reduction)(p, t)


@pytest.mark.parametrize("case", GRAD_CASES)
def test_loss_and_both_gradients(case):
    p, t, loss = _run(case)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference(case)
    _bound(f"case {case} loss", loss, l64, l32)
    _bound(f"case {case} grad pred", p.grad, gp64, gp32)
    _bound(f"case {case} grad target", t.grad, gt64, gt32)


@functools.lru_cache(maxsize=None)
def _items_reference(case):
    """ssim of every (b, c) image in fp64 and in fp32, once on the CPU."""
    pred, target = _inputs(case)
    return tuple(R.ssim_items(pred, target, RANGE, dtype) for dtype in (torch.float64, torch.float32))


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_more_than_256_tiles_per_item(reduction):
    """Case i: an item's tile partials outnumber the item kernel's 256 threads.  The kernel's own error is one fp32
    rounding of an fp64 sum (6e-8 relative), inside the bound's additive term."""
    _, _, loss = _run("i", reduction, grad=(False, False))
    assert tuple(loss.shape) == ((2,) if reduction == "none" else ())
    reduce = {"mean": lambda x: x.mean(), "sum": lambda x: x.sum(), "none": lambda x: x.mean(dim=1)}[reduction]
    i64, i32 = _items_reference("i")
    _bound(f"case i {reduction} loss", loss, reduce(1.0 - i64), reduce(1.0 - i32))


@pytest.mark.parametrize("shape", [(23, 41), (9, 17, 35)])
def test_one_minus_loss_is_the_metric(shape):
    """Both are fp32 roundings of a double mean of values <= 1."""
    g = torch.Generator().manual_seed(7)
    a = torch.round(torch.rand(shape, generator=g) * 255).cuda()
    b = torch.round((0.8 * a.cpu() + 0.2 * torch.rand(shape, generator=g) * 255)).cuda()
    want = metrics.ssim(a, b, 256.0)
    got = 1.0 - losses.ssim_loss(a[None, None], b[None, None], value_range=(0.0, 256.0))
    print(f"metric {float(want):.8f}  1 - loss {float(got):.8f}")
    assert 0.0 < float(want) < 1.0 and abs(float(got) - float(want)) <= 1e-6


@pytest.mark.parametrize("case", ["c", "f"])
def test_identical_inputs(case):
    pred, _ = _inputs(case)
    p = pred.cuda().requires_grad_(True)
    loss = losses.ssim_loss(p, pred.cuda(), RANGE)
    loss.backward()
    assert abs(float(loss.detach())) <= 1e-6
    assert float(p.grad.abs().max()) <= 1e-6 / pred.numel()


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_reductions_upstream_and_second_backward(reduction):
    p, t, loss = _run("c", reduction)                              # (1, 2, 17, 45): "none" averages the two channels
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference("c", reduction)
    assert tuple(loss.shape) == ((1,) if reduction == "none" else ())
    _bound(f"{reduction} loss", loss, l64, l32)
    out = loss.sum() if reduction == "none" else loss
    out.backward(retain_graph=True)
    g1p, g1t = p.grad.clone(), t.grad.clone()
    _bound(f"{reduction} grad pred", g1p, gp64, gp32)
    _bound(f"{reduction} grad target", g1t, gt64, gt32)
    p.grad = t.grad = None
    out.backward(retain_graph=True)                                # a second backward reads unscaled saved state
    assert torch.equal(p.grad, g1p) and torch.equal(t.grad, g1t)
    p.grad = t.grad = None
    (3 * out).backward()                                           # the upstream scalar enters as one more factor
    assert float((p.grad - 3 * g1p).abs().max()) <= 4 * 2.0 ** -23 * 3 * float(g1p.abs().max())
    assert float((t.grad - 3 * g1t).abs().max()) <= 4 * 2.0 ** -23 * 3 * float(g1t.abs().max())


def test_none_is_one_entry_per_batch_item_with_its_own_upstream():
    p, t, loss = _run("b", "none")                                 # (2, 1, 9, 39)
    (l64, _, _), (l32, _, _) = _reference("b", "none")
    assert tuple(loss.shape) == (2,)
    _bound("none loss per batch entry", loss, l64, l32)
    (loss * torch.tensor([1.0, 0.0], device="cuda")).sum().backward()
    assert float(p.grad[0].abs().max()) > 0 and float(p.grad[1].abs().max()) == 0
    (_, gp64, _), (_, gp32, _) = _reference("b", "none")
    _bound("none grad of entry 0", p.grad[0], gp64[0], gp32[0])


def test_only_the_requested_gradient_is_computed():
    (_, gp64, gt64), (_, gp32, gt32) = _reference("f")
    p, t, loss = _run("f", grad=(True, False))
    loss.backward()
    assert t.grad is None
    _bound("pred only", p.grad, gp64, gp32)
    p, t, loss = _run("f", grad=(False, True))
    loss.backward()
    assert p.grad is None
    _bound("target only", t.grad, gt64, gt32)
    assert not _run("f", grad=(False, False))[2].requires_grad


@pytest.mark.parametrize("case", ["c", "f"])
def test_bitwise_reproducible(case):
    runs = []
    for _ in range(2):
        p, t, loss = _run(case)
        loss.backward()
        runs.append((loss.detach().clone(), p.grad.clone(), t.grad.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_device_side_errors():
    x = torch.rand(1, 1, 3, 9, 9, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        losses.ssim_loss(x, x)                                     # a 3-D depth of 3
    with pytest.raises((ValueError, RuntimeError)):
        losses.ssim_loss(torch.rand(1, 1, 9, 9, device="cuda"), torch.rand(1, 1, 9, 10, device="cuda"))
    from mpgan_amd import ops
    ws = torch.empty(64, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="depth 3"):             # the library's own refusal, before any launch
        ops.ssim_loss_forward(x, x, (3, 9, 9), 1, 1, 0.0, 1.0, 0, ws, None, "mean", torch.empty((), device="cuda"))
