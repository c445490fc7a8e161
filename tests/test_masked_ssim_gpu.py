"""The masked SSIM on the MI355X against the float64 torch restatement (masked_ssim_ref.py): losses.ssim_loss(mask= /
threshold=), SSIMLoss / ForegroundSSIMLoss, metrics.ssim(mask=), metrics.ssim_map and score_volume(mask=).

The shapes are those of test_ssim_loss_gpu.py: both kernels tile y-x as 8 x 32 and z as 4 (the forward over window
corners, the backward over samples); case "i" gives an item more forward tiles than the 256 threads of the per-item
tail that adds them (the loss alone, under every reduction).  Masks are seeded, half set, with bytes in {0, 1, 2, 255}.

The bound, for the loss, each gradient, metrics.ssim(mask=) and ssim_map (max-abs over the tensor):

    err(ours, f64) <= 4 * err(torch fp32 on the CPU, f64) + 2e-6 * max|f64 reference|

as test_ssim_loss_gpu.py states and justifies it.  Every case prints both errors under -s."""
import functools

import pytest
import torch

import masked_ssim_ref as MR
import ssim_loss_ref as R
from mpgan_amd import losses, metrics, ops
from mpgan_amd import preprocess as P

pytestmark = pytest.mark.gpu

CASES = {
    "a": (1, 1, 7, 7),             # a single 2-D window; the mask is set at its centre (3, 3)
    "b": (2, 1, 9, 39),            # ragged x tile; the two items carry different masks
    "c": (1, 2, 17, 45),           # channel items; the mask has channel extent 1
    "d": (1, 1, 7, 7, 7),          # a single 3-D window; the centre (3, 3, 3) is set
    "e": (1, 1, 9, 10, 40),        # 3-D, ragged on every axis
    "f": (2, 1, 13, 21, 37),       # 3-D
    "g": (1, 1, 21, 37),           # image and mask passed one element / one byte into a larger buffer
    "h": (1, 1, 13, 17, 41),       # two tiles and a ragged remainder on every axis
    "i": (2, 2, 136, 544),         # 17 x 17 = 289 tile partials per item through the per-item tail (loss only)
}
GRAD_CASES = [case for case in CASES if case != "i"]
RANGE = (-1.0, 1.0)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return R.structured_pair(CASES[case], seed=40 + ord(case))


@functools.lru_cache(maxsize=None)
def _mask(case):
    shape = CASES[case]
    if case == "c":
        shape = shape[:1] + (1,) + shape[2:]
    mask = MR.random_mask(shape, seed=70 + ord(case))
    if case in ("a", "d"):
        mask[(0, 0) + (3,) * (len(shape) - 2)] = 255
    if case == "b":
        assert not torch.equal(mask[0], mask[1])
    return mask


def _dev(x, case=""):
    """The tensor on the device; case g as a contiguous view one element into a larger buffer."""
    if case == "g":
        buf = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
        view = buf[1:].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % (4 * x.element_size()) == x.element_size()
        return view
    return x.cuda()


@functools.lru_cache(maxsize=None)
def _reference(case, reduction="mean"):
    """(loss, grad_pred, grad_target) in fp64 and in fp32, computed once per configuration on the CPU."""
    pred, target = _inputs(case)
    kw = dict(value_range=RANGE, reduction=reduction)
    return (MR.loss_and_gradients(pred, target, _mask(case), dtype=torch.float64, **kw),
            MR.loss_and_gradients(pred, target, _mask(case), dtype=torch.float32, **kw))


def _bound(name, got, f64, f32):
    got, f64, f32 = got.detach().double().cpu(), f64.double(), f32.double()
    ours, peer = float((got - f64).abs().max()), float((f32 - f64).abs().max())
    scale = float(f64.abs().max())
    limit = 4.0 * peer + 2e-6 * scale
    print(f"{name}: err ours {ours:.3e}  torch-fp32 {peer:.3e}  max|ref| {scale:.3e}  limit {limit:.3e}")
    assert ours <= limit, (name, ours, peer, scale, limit)


def _run(case, reduction="mean", grad=(True, True), **source):
    """(pred, target, loss) on the device; the mask source defaults to the case's explicit mask."""
    pred, target = _inputs(case)
    p, t = _dev(pred, case).requires_grad_(grad[0]), _dev(target, case).requires_grad_(grad[1])
    if not source:
        source = {"mask": _dev(_mask(case), case)}
    return p, t, losses.ssim_loss(p, t, RANGE, reduction, **source)


def _backward(case, reduction="mean", **source):
    p, t, loss = _run(case, reduction, **source)
    (loss.sum() if reduction == "none" else loss).backward()
    return loss.detach(), p.grad, t.grad


def _stats(pred, target, mask=None, thr=None):
    """(ssim_item, n_item) per item straight from the forward entry point."""
    a, b = pred.contiguous(), target.contiguous()
    items, spatial = a.shape[0] * a.shape[1], tuple(a.shape[2:])
    ws = torch.empty(ops.masked_ssim_loss_workspace(spatial, items, 0)[0] // 8, dtype=torch.float64, device="cuda")
    stats = torch.empty((items, 2), dtype=torch.float64, device="cuda")
    ops.masked_ssim_loss_forward(a, b, spatial, items, a.shape[1], RANGE[0], RANGE[1], mask, thr, 0, ws, None, stats, None,
                                 "mean", torch.empty((), device="cuda"))
    return stats[:, 0].cpu(), stats[:, 1].cpu()


@pytest.mark.parametrize("case", GRAD_CASES)
def test_loss_and_both_gradients(case):
    p, t, loss = _run(case)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference(case)
    _bound(f"case {case} loss", loss, l64, l32)
    _bound(f"case {case} grad pred", p.grad, gp64, gp32)
    _bound(f"case {case} grad target", t.grad, gt64, gt32)
    # the count is exact, and the item is the reference's
    mask = _dev(_mask(case), case).expand(CASES[case]).contiguous()
    item, count = _stats(p.detach(), t.detach(), mask)
    i64, c64 = MR.items_and_counts(*_inputs(case), _mask(case), RANGE)
    i32, _ = MR.items_and_counts(*_inputs(case), _mask(case), RANGE, torch.float32)
    assert torch.equal(count, c64.reshape(-1)) and float(count.min()) > 0
    _bound(f"case {case} ssim_item", item, i64.reshape(-1), i32.reshape(-1))


@functools.lru_cache(maxsize=None)
def _items_reference(case):
    pred, target = _inputs(case)
    return tuple(MR.items_and_counts(pred, target, _mask(case), RANGE, dtype)[0] for dtype in (torch.float64, torch.float32))


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_more_than_256_tiles_per_item(reduction):
    """Case i: an item's tile partials and counts outnumber the per-item tail's 256 threads."""
    _, _, loss = _run("i", reduction, grad=(False, False))
    assert tuple(loss.shape) == ((2,) if reduction == "none" else ())
    reduce = {"mean": lambda x: x.mean(), "sum": lambda x: x.sum(), "none": lambda x: x.mean(dim=1)}[reduction]
    i64, i32 = _items_reference("i")
    _bound(f"case i {reduction} loss", loss, reduce(1.0 - i64), reduce(1.0 - i32))
    if reduction == "mean":
        pred, target = _inputs("i")
        _, count = _stats(pred.cuda(), target.cuda(), _mask("i").cuda())
        assert torch.equal(count, MR.items_and_counts(pred, target, _mask("i"), RANGE)[1].reshape(-1))


@pytest.mark.parametrize("case", ["c", "f"])
def test_threshold_mode_is_the_explicit_foreground_mask_bit_for_bit(case):
    _, target = _inputs(case)
    td = target.cuda()
    for threshold in ("otsu", 0.1):
        mask = P.foreground_mask(td, threshold)
        frac = float(mask.float().mean())
        assert 0.05 < frac < 0.95, frac
        by_thr = _backward(case, threshold=threshold)
        by_mask = _backward(case, mask=mask)
        for x, y in zip(by_thr, by_mask):
            assert torch.equal(x, y)
        module = losses.ForegroundSSIMLoss(threshold)(_inputs(case)[0].cuda(), td)
        assert torch.equal(module, by_mask[0])
        assert torch.equal(losses.SSIMLoss(RANGE, threshold=threshold)(_inputs(case)[0].cuda(), td), by_mask[0])
    # a per-item threshold tensor; a NaN threshold empties its item
    items = CASES[case][0] * CASES[case][1]
    thr = torch.full((items,), 0.1, device="cuda")
    assert torch.equal(_backward(case, threshold=thr)[0], _backward(case, threshold=0.1)[0])
    thr[0] = float("nan")
    assert float(_stats(_inputs(case)[0].cuda(), td, thr=thr)[1][0]) == 0.0


@pytest.mark.parametrize("case", ["c", "f"])
def test_all_ones_mask_is_the_unmasked_loss(case):
    pred, target = _inputs(case)
    ones = torch.ones(CASES[case], dtype=torch.uint8, device="cuda")
    loss, gp, gt = _backward(case, mask=ones)
    p, t = pred.cuda().requires_grad_(True), target.cuda().requires_grad_(True)
    plain = losses.SSIMLoss(RANGE)(p, t)
    plain.backward()
    plain = plain.detach()
    ulp = 2.0 ** -23 * float(plain.abs())
    print(f"case {case} all-ones: masked {float(loss):.9f}  plain {float(plain):.9f}")
    assert abs(float(loss) - float(plain)) <= ulp
    torch.testing.assert_close(gp, p.grad, rtol=2.0 ** -22, atol=0.0)
    torch.testing.assert_close(gt, t.grad, rtol=2.0 ** -22, atol=0.0)
    m = 1
    for s in CASES[case][2:]:
        m *= s - 6
    assert bool((_stats(pred.cuda(), target.cuda(), ones)[1] == m).all())
    # no mask source at all weighs every window 1, too
    assert bool((_stats(pred.cuda(), target.cuda())[1] == m).all())
    # a bool mask is a uint8 one
    assert torch.equal(_backward(case, mask=ones.bool())[0], loss)


def _ring(shape):
    """Set only in the 3-wide border ring that the interior drops."""
    ring = torch.ones(shape, dtype=torch.uint8)
    ring[(Ellipsis,) + (slice(3, -3),) * (len(shape) - 2)] = 0
    return ring


@pytest.mark.parametrize("case", ["b", "f"])
def test_empty_items(case):
    shape = CASES[case]                                            # two batch entries of one channel
    pred, target = _inputs(case)
    for name, empty in (("zeros", torch.zeros(shape, dtype=torch.uint8)), ("ring", _ring(shape))):
        assert name == "zeros" or int(empty.sum()) > 0
        for reduction in ("mean", "sum", "none"):
            loss, gp, gt = _backward(case, reduction, mask=empty.cuda())
            assert bool((loss == 0).all()) and bool((gp == 0).all()) and bool((gt == 0).all()), (name, reduction)
        item, count = _stats(pred.cuda(), target.cuda(), empty.cuda())
        assert bool(torch.isnan(item).all()) and bool((count == 0).all())
        vol = (pred[0, 0] + 1.0).cuda()
        assert bool(torch.isnan(metrics.ssim(vol, (target[0, 0] + 1.0).cuda(), 2.0, mask=empty[0, 0].cuda())))
    # one empty and one non-empty item: the empty one adds 0 and an exactly-zero gradient, the other is what it is alone
    mixed = _mask(case).clone()
    mixed[0] = 0
    loss, gp, gt = _backward(case, "sum", mask=mixed.cuda())
    p1, t1 = pred[1:].cuda().requires_grad_(True), target[1:].cuda().requires_grad_(True)
    alone = losses.ssim_loss(p1, t1, RANGE, "sum", mask=mixed[1:].cuda())
    alone.backward()
    assert float(alone.detach()) > 0 and torch.equal(loss, alone.detach())
    assert bool((gp[0] == 0).all()) and bool((gt[0] == 0).all())
    assert torch.equal(gp[1:], p1.grad) and torch.equal(gt[1:], t1.grad)
    per_entry = _run(case, "none", mask=mixed.cuda())[2]
    assert float(per_entry[0]) == 0.0 and torch.equal(per_entry[1], alone.detach())
    # under "mean" the empty item still counts as an item
    mean = _run(case, "mean", mask=mixed.cuda())[2]
    assert abs(float(mean) - 0.5 * float(alone.detach())) <= 2.0 ** -23 * float(alone.detach())


@pytest.mark.parametrize("case", ["c", "f"])
def test_identical_inputs(case):
    pred, _ = _inputs(case)
    p = pred.cuda().requires_grad_(True)
    loss = losses.ssim_loss(p, pred.cuda(), RANGE, mask=_mask(case).cuda())
    loss.backward()
    assert abs(float(loss.detach())) <= 1e-6
    assert float(p.grad.abs().max()) <= 1e-6 / pred.numel()


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


@pytest.mark.parametrize("reduction", ["sum", "none"])
def test_reductions(reduction):
    p, t, loss = _run("c", reduction)                              # (1, 2, 17, 45): "none" averages the two channels
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference("c", reduction)
    assert tuple(loss.shape) == ((1,) if reduction == "none" else ())
    _bound(f"{reduction} loss", loss, l64, l32)
    (loss.sum() if reduction == "none" else loss).backward()
    _bound(f"{reduction} grad pred", p.grad, gp64, gp32)
    _bound(f"{reduction} grad target", t.grad, gt64, gt32)
    # one entry per batch item, each with its own upstream
    p, t, loss = _run("b", "none")
    (l64, gp64, _), (l32, gp32, _) = _reference("b", "none")
    _bound("none loss per batch entry", loss, l64, l32)
    (loss * torch.tensor([1.0, 0.0], device="cuda")).sum().backward()
    assert float(p.grad[0].abs().max()) > 0 and float(p.grad[1].abs().max()) == 0
    _bound("none grad of entry 0", p.grad[0], gp64[0], gp32[0])


@pytest.mark.parametrize("case", ["c", "f"])
def test_bitwise_reproducible(case):
    runs = []
    for _ in range(2):
        p, t, loss = _run(case)
        loss.backward(retain_graph=True)
        first = (loss.detach().clone(), p.grad.clone(), t.grad.clone())
        p.grad = t.grad = None
        loss.backward()                                            # a second backward reads unscaled saved state
        assert torch.equal(p.grad, first[1]) and torch.equal(t.grad, first[2])
        runs.append(first)
    for x, y in zip(*runs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("case", ["c", "g", "h"])
def test_metric_and_map(case):
    """metrics.ssim(mask=) and metrics.ssim_map of item (0, 0), shifted to [0, 2] (the metric's lo is 0)."""
    pred, target = _inputs(case)
    a, b = pred[:1, :1] + 1.0, target[:1, :1] + 1.0
    mask = _mask(case)[:1, :1]
    ad, bd, md = _dev(a[0, 0], case), _dev(b[0, 0], case), _dev(mask[0, 0], case)
    i64, c64 = MR.items_and_counts(a, b, mask, (0.0, 2.0))
    i32, _ = MR.items_and_counts(a, b, mask, (0.0, 2.0), torch.float32)
    got = metrics.ssim(ad, bd, 2.0, mask=md)
    assert got.dtype == torch.float64 and got.shape == ()
    _bound(f"case {case} metrics.ssim(mask=)", got, i64.reshape(()), i32.reshape(()))
    m64, m32 = MR.ssim_map(a, b, (0.0, 2.0))[0, 0], MR.ssim_map(a, b, (0.0, 2.0), torch.float32)[0, 0]
    smap = metrics.ssim_map(ad, bd, 2.0)
    assert smap.dtype == torch.float32 and tuple(smap.shape) == tuple(s - 6 for s in a.shape[2:])
    _bound(f"case {case} ssim_map", smap, m64, m32)
    # the map's mean is the metric; its mean over the mask's interior is the masked metric
    whole = metrics.ssim(ad, bd, 2.0)
    _bound(f"case {case} mean of the map", smap.double().mean(), m64.mean(), m32.mean())
    assert abs(float(smap.double().mean()) - float(whole)) <= 2e-6 * float(m64.abs().max())
    interior = md[(slice(3, -3),) * md.dim()] != 0
    assert int(interior.sum()) == int(c64)
    picked = smap[interior].double().mean()
    _bound(f"case {case} mean of the map over the mask", picked, i64.reshape(()), i32.reshape(()))
    assert abs(float(picked) - float(got)) <= 2e-6 * float(m64.abs().max())
    # a bool mask, and twice the same bits
    assert torch.equal(metrics.ssim(ad, bd, 2.0, mask=md != 0), got) and torch.equal(metrics.ssim_map(ad, bd, 2.0), smap)


def test_score_volume_adds_the_masked_figure_and_keeps_the_whole_one():
    pred, target = _inputs("h")
    vol, ref = pred[0, 0].cuda(), target[0, 0].cuda()
    m = P.foreground_mask(ref)
    scored, whole = metrics.score_volume(vol, ref, mask=m), metrics.score_volume(vol, ref)
    assert set(whole) == {"mae", "mse", "psnr", "ssim"}
    assert set(scored) == {"mae", "mse", "psnr", "ssim", "count", "ssim_masked"}
    assert torch.equal(scored["ssim"], whole["ssim"])
    g, t = metrics.rescale_0_255(vol), metrics.rescale_0_255(ref)
    assert torch.equal(scored["ssim_masked"], metrics.ssim(g, t, 256.0, mask=m))
    assert scored["ssim_masked"].dtype == torch.float64 and 0.0 < float(scored["ssim_masked"]) < 1.0
    assert float(scored["ssim_masked"]) != float(scored["ssim"])
    # too small for a window: neither figure
    assert "ssim_masked" not in metrics.score_volume(vol[:, :5], ref[:, :5], mask=m[:, :5])
    # with the mutual information on top
    assert set(metrics.score_volume(vol, ref, mutual_information=True, mask=m)) == set(scored) | {"mi", "nmi"}


def test_device_side_errors():
    x = torch.rand(1, 1, 3, 9, 9, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        losses.ssim_loss(x, x, mask=torch.ones_like(x, dtype=torch.uint8))       # a 3-D depth of 3
    y = torch.rand(1, 2, 9, 9, device="cuda")
    with pytest.raises(ValueError, match="channel extent 1"):
        losses.ssim_loss(y, y, mask=torch.ones(1, 2, 9, 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="inputs' device"):
        losses.ssim_loss(y, y, mask=torch.ones(1, 2, 9, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="threshold tensor"):
        losses.ssim_loss(y, y, threshold=torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError, match="same-shape"):
        metrics.ssim(y[0, 0], y[0, 0], mask=torch.ones(9, 8, dtype=torch.uint8, device="cuda"))
    ws = torch.empty(64, dtype=torch.float64, device="cuda")
    stats = torch.empty((1, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="both"):                  # the library's own refusal, before any launch
        ops.masked_ssim_loss_forward(y, y, (9, 9), 2, 2, 0.0, 1.0, torch.ones(1, 2, 9, 9, dtype=torch.uint8, device="cuda"),
                                     torch.zeros(2, device="cuda"), 0, ws, None, stats, None, "mean",
                                     torch.empty((), device="cuda"))
