"""mpgan_amd.losses.sobel_magnitude and edge_loss on the MI355X against the float64 torch restatement (edge_loss_ref.py).

All kernels tile z-y-x as 4 x 8 x 32 (1 x 8 x 32 when the image is one plane).  The cases (edge_loss_ref.CASES):

    a (1,1,1,1)    f (1,1,1,1,1)       one voxel: every tap is clamped onto it
    b (1,1,2,3)    g (1,1,2,2,3)       every voxel is a border voxel on every axis
    c (1,1,3,3)    h (1,1,3,3,3)       the smallest image with an interior voxel
    d (2,1,9,39)                       two items; crosses the 8-row and the 32-wide tile by a ragged 1 and 7
    e (1,2,17,45)                      channel items; three y tiles
    i (1,1,1,9,40)                     a 5-D tensor of depth 1: the one-plane kernels
    j (1,1,9,10,40)  k (2,1,13,21,37)  volumes, ragged on every axis
    l (1,1,13,17,41)                   two tiles plus a ragged remainder on every axis
    m (1,1,21,37)                      passed at a storage offset of one element: data_ptr % 16 == 4
    n (1,1,12,24,96)                   3 x 3 x 3 tiles: the middle one touches no face of the image and runs the gather
                                       with the constant interior weights
    o (2,2,136,544)                    17 x 17 = 289 tiles per item, more than the 256 threads of the block that adds an
                                       item's partials: the loss alone, under every reduction (not in edge_loss_ref.CASES,
                                       whose every entry also runs the gradient and map tests)

The bound, for the loss, the map and each gradient (max-abs over the tensor), is the one of test_ssim_loss_gpu.py:

    err(ours, f64) <= 4 * err(torch fp32 on the CPU, f64) + 2e-6 * max|f64 reference|

Every case prints both errors under -s.  The loss has a kink where m(pred) = m(target): the gradient entries within the
3^d neighbourhood of a near-kink voxel (edge_loss_ref.near_kink_outputs, from the float64 maps; at most 2 % of a case,
test_edge_loss_host.py asserts it) are left out of the comparison of edge_loss's gradients with the reference, on our
side and on torch's.  sobel_magnitude has no kink, and neither has the comparison of edge_loss with the composition
l1(sobel_magnitude(a), sobel_magnitude(b)) on the device, which sees the same bits of m: there every entry counts."""
import functools

import pytest
import torch

import edge_loss_ref as R
from mpgan_amd import losses, ops
from mpgan_amd.gan import reconstruction_loss

pytestmark = pytest.mark.gpu

CASES = list(R.CASES)
WIDE, WIDE_SEED = (2, 2, 136, 544), 40 + len(CASES)                # shape o, the loss alone


def _dev(x, case=""):
    """The tensor on the device; case m as a contiguous view one element into a larger buffer."""
    if case == "m":
        buf = torch.empty(x.numel() + 1, device="cuda")
        view = buf[1:].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view
    return x.cuda()


@functools.lru_cache(maxsize=None)
def _reference(case, reduction="mean"):
    """(loss, grad_pred, grad_target) in fp64 and in fp32, computed once per configuration on the CPU."""
    pred, target = R.case_inputs(case)
    return (R.loss_and_gradients(pred, target, dtype=torch.float64, reduction=reduction),
            R.loss_and_gradients(pred, target, dtype=torch.float32, reduction=reduction))


@functools.lru_cache(maxsize=None)
def _kept(case):
    """The gradient entries no near-kink voxel reaches."""
    return ~R.near_kink_outputs(*R.case_inputs(case))


@functools.lru_cache(maxsize=None)
def _map_reference(case):
    """A random signed upstream map, then (m, its vjp) in fp64 and in fp32 for the case's first tensor."""
    x, _ = R.case_inputs(case)
    up = torch.rand(x.shape, generator=torch.Generator().manual_seed(90 + R.SEEDS[case])) * 2 - 1
    return up, R.magnitude_and_vjp(x, up, torch.float64), R.magnitude_and_vjp(x, up, torch.float32)


def _limit(name, f64, f32, keep=None):
    """4 * err(torch fp32, f64) + 2e-6 * max|f64|, the peer's error over the kept entries."""
    f64, f32 = f64.double(), f32.double()
    peer = (f32 - f64).abs()
    peer = float((peer[keep] if keep is not None else peer).max())
    scale = float(f64.abs().max())
    return peer, scale, 4.0 * peer + 2e-6 * scale


def _bound(name, got, f64, f32, keep=None):
    got = got.detach().double().cpu()
    peer, scale, limit = _limit(name, f64, f32, keep)
    err = (got - f64.double()).abs()
    ours = float((err[keep] if keep is not None else err).max())
    left = 0 if keep is None else int((~keep).sum())
    print(f"{name}: err ours {ours:.3e}  torch-fp32 {peer:.3e}  max|ref| {scale:.3e}  limit {limit:.3e}  left out {left}")
    assert ours <= limit, (name, ours, peer, scale, limit)


def _run(case, reduction="mean", grad=(True, True)):
    pred, target = R.case_inputs(case)
    p, t = _dev(pred, case).requires_grad_(grad[0]), _dev(target, case).requires_grad_(grad[1])
    return p, t, losses.EdgeLoss(reduction=reduction)(p, t)


@pytest.mark.parametrize("case", CASES)
def test_sobel_magnitude_and_its_backward(case):
    up, (m64, g64), (m32, g32) = _map_reference(case)
    x = _dev(R.case_inputs(case)[0], case).requires_grad_(True)
    m = losses.sobel_magnitude(x)
    assert m.shape == x.shape and m.dtype == torch.float32
    m.backward(_dev(up, case))
    _bound(f"case {case} map", m, m64, m32)
    _bound(f"case {case} map backward", x.grad, g64, g32)


@pytest.mark.parametrize("case", CASES)
def test_loss_and_both_gradients(case):
    p, t, loss = _run(case)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference(case)
    _bound(f"case {case} loss", loss, l64, l32)
    _bound(f"case {case} grad pred", p.grad, gp64, gp32, _kept(case))
    _bound(f"case {case} grad target", t.grad, gt64, gt32, _kept(case))


@pytest.mark.parametrize("case", CASES)
def test_gradient_equals_the_composition_on_every_entry(case):
    """l1(sobel_magnitude(a), sobel_magnitude(b)) through this library's own ops: the same m, hence the same signs, so no
    entry is left out; the limit is the bound's, from the fp64 reference of that composition."""
    p, t, loss = _run(case)
    loss.backward()
    pc, tc = p.detach().clone().requires_grad_(True), t.detach().clone().requires_grad_(True)
    composed = reconstruction_loss(losses.sobel_magnitude(pc), losses.sobel_magnitude(tc))
    composed.backward()
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference(case)
    for name, got, comp, f64, f32 in (("loss", loss, composed, l64, l32), ("grad pred", p.grad, pc.grad, gp64, gp32),
                                      ("grad target", t.grad, tc.grad, gt64, gt32)):
        peer, scale, limit = _limit(name, f64, f32, None if name == "loss" else _kept(case))
        diff = float((got.detach().double() - comp.detach().double()).abs().max())
        print(f"case {case} {name}: fused - composed {diff:.3e}  limit {limit:.3e}")
        assert diff <= limit, (case, name, diff, limit)


@pytest.mark.parametrize("case", ["e", "k", "n"])
def test_identical_inputs(case):
    pred, _ = R.case_inputs(case)
    p, t = pred.cuda().requires_grad_(True), pred.cuda().requires_grad_(True)
    loss = losses.edge_loss(p, t)
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert float(p.grad.abs().max()) == 0.0 and float(t.grad.abs().max()) == 0.0


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_reductions_upstream_and_second_backward(reduction):
    p, t, loss = _run("e", reduction)                              # (1, 2, 17, 45): "none" averages the two channels
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference("e", reduction)
    assert tuple(loss.shape) == ((1,) if reduction == "none" else ())
    _bound(f"{reduction} loss", loss, l64, l32)
    out = loss.sum() if reduction == "none" else loss
    out.backward(retain_graph=True)
    g1p, g1t = p.grad.clone(), t.grad.clone()
    _bound(f"{reduction} grad pred", g1p, gp64, gp32, _kept("e"))
    _bound(f"{reduction} grad target", g1t, gt64, gt32, _kept("e"))
    p.grad = t.grad = None
    out.backward(retain_graph=True)                                # nothing but the inputs is saved: the same bits
    assert torch.equal(p.grad, g1p) and torch.equal(t.grad, g1t)
    p.grad = t.grad = None
    (3 * out).backward()                                           # the upstream scalar enters as one more factor
    assert float((p.grad - 3 * g1p).abs().max()) <= 4 * 2.0 ** -23 * 3 * float(g1p.abs().max())
    assert float((t.grad - 3 * g1t).abs().max()) <= 4 * 2.0 ** -23 * 3 * float(g1t.abs().max())


@functools.lru_cache(maxsize=None)
def _wide_reference():
    """(pred, target) of shape o and the loss of every (b, c) image in fp64 and in fp32, once on the CPU."""
    pred, target = R.structured_pair(WIDE, seed=WIDE_SEED)
    return pred, target, R.loss_items(pred, target), R.loss_items(pred, target, dtype=torch.float32)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_more_than_256_tiles_per_item(reduction):
    """Shape o: an item's tile partials outnumber the 256 threads of the block that adds them.  That kernel's own error
    is one fp32 rounding of an fp64 sum (6e-8 relative), inside the bound's additive term."""
    pred, target, i64, i32 = _wide_reference()
    loss = losses.EdgeLoss(reduction=reduction)(pred.cuda(), target.cuda())
    assert tuple(loss.shape) == ((2,) if reduction == "none" else ())
    reduce = {"mean": lambda x: x.mean(), "sum": lambda x: x.sum(), "none": lambda x: x.mean(dim=1)}[reduction]
    _bound(f"shape o {reduction} loss", loss, reduce(i64), reduce(i32))


def test_none_is_one_entry_per_batch_item_with_its_own_upstream():
    p, t, loss = _run("k", "none")                                 # (2, 1, 13, 21, 37)
    (l64, gp64, _), (l32, gp32, _) = _reference("k", "none")
    assert tuple(loss.shape) == (2,)
    _bound("none loss per batch entry", loss, l64, l32)
    (loss * torch.tensor([1.0, 0.0], device="cuda")).sum().backward()
    assert float(p.grad[0].abs().max()) > 0 and float(p.grad[1].abs().max()) == 0
    _bound("none grad of entry 0", p.grad[0], gp64[0], gp32[0], _kept("k")[0])


def test_only_the_requested_gradient_is_computed(monkeypatch):
    calls = []
    real = ops.edge_loss_backward
    monkeypatch.setattr(ops, "edge_loss_backward", lambda *a: calls.append(a[8]) or real(*a))     # a[8]: wrt
    (_, gp64, gt64), (_, gp32, gt32) = _reference("k")
    p, t, loss = _run("k", grad=(True, False))
    loss.backward()
    assert t.grad is None and calls == [0]
    _bound("pred only", p.grad, gp64, gp32, _kept("k"))
    p, t, loss = _run("k", grad=(False, True))
    loss.backward()
    assert p.grad is None and calls == [0, 1]
    _bound("target only", t.grad, gt64, gt32, _kept("k"))
    assert not _run("k", grad=(False, False))[2].requires_grad


@pytest.mark.parametrize("case", ["e", "l"])
def test_bitwise_reproducible(case):
    runs = []
    for _ in range(2):
        p, t, loss = _run(case)
        loss.backward()
        runs.append((loss.detach().clone(), p.grad.clone(), t.grad.clone(), losses.sobel_magnitude(p.detach())))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_module_and_eps():
    pred, target = R.case_inputs("j")
    got = losses.EdgeLoss(eps=1e-3, reduction="sum")(pred.cuda(), target.cuda())
    _bound("eps 1e-3", got, R.loss(pred, target, 1e-3, "sum"), R.loss(pred, target, 1e-3, "sum", torch.float32))
    with pytest.raises(ValueError, match="shape mismatch"):
        losses.edge_loss(pred.cuda(), target.cuda()[..., :-1])
