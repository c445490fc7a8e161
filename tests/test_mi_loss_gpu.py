"""mpgan_amd.losses on the MI355X against the float64 torch restatement (mi_loss_ref.py).

The bound, for the loss and for each gradient (max-abs over the tensor):

    err(ours, f64) <= 4 * err(torch fp32 on the CPU, f64) + 2e-6 * max|f64 reference|

The factor 4 is the margin for a different but equally fp32 summation order (ours: wave partials of at most 512
voxels, then fp64; torch: a blocked bmm).  The additive term covers one fp32 rounding of the exponent argument:
weights above 1e-7 have |arg| <= 16, 2^-24 * 16 ~ 1e-6 is the relative error of a weight, doubled for the two images;
it matters where torch's own fp32 run happens to land on the fp64 value.  Every case prints both errors under -s."""
import functools

import pytest
import torch

import mi_loss_ref as R
from mpgan_amd import losses

pytestmark = pytest.mark.gpu

CASES = {
    "a": (2, 1, 5, 7, 9),          # N = 315: under one block, odd tail
    "b": (3, 1, 33, 31),           # N = 1023: one short of a power of two
    "c": (1, 2, 64, 64, 48),       # N = 393,216: many waves and slots, channel folding
    "d": (1, 1, 257, 255),         # N = 65,535, passed at a storage offset of one element: unaligned
}
BINS_SIGMA = [(23, 0.5), (32, 0.5), (2, 0.5), (16, 1.0), (23, 0.25)]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return R.correlated_pair(CASES[case], seed=10 + ord(case))


def _dev(x, case=""):
    """The tensor on the device; case d as a contiguous view one element into a larger buffer."""
    if case == "d":
        buf = torch.empty(x.numel() + 1, device="cuda")
        view = buf[1:].view(x.shape)
        view.copy_(x)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view
    return x.cuda()


@functools.lru_cache(maxsize=None)
def _reference(case, bins=23, sigma=0.5, reduction="mean"):
    """(loss, grad_pred, grad_target) in fp64 and in fp32, computed once per configuration on the CPU."""
    pred, target = _inputs(case)
    kw = dict(num_bins=bins, sigma_ratio=sigma, reduction=reduction)
    return (R.loss_and_gradients(pred, target, dtype=torch.float64, **kw),
            R.loss_and_gradients(pred, target, dtype=torch.float32, **kw))


def _bound(name, got, f64, f32):
    got, f64, f32 = got.detach().double().cpu(), f64.double(), f32.double()
    ours, peer = float((got - f64).abs().max()), float((f32 - f64).abs().max())
    scale = float(f64.abs().max())
    limit = 4.0 * peer + 2e-6 * scale
    print(f"{name}: err ours {ours:.3e}  torch-fp32 {peer:.3e}  max|ref| {scale:.3e}  limit {limit:.3e}")
    assert ours <= limit, (name, ours, peer, scale, limit)


def _run(case, bins=23, sigma=0.5, reduction="mean", **kw):
    pred, target = _inputs(case)
    p, t = _dev(pred, case).requires_grad_(True), _dev(target, case).requires_grad_(True)
    loss = losses.GlobalMutualInformationLoss(bins, sigma, reduction, **kw)(p, t)
    return p, t, loss


@pytest.mark.parametrize("case", list(CASES))
def test_loss_and_both_gradients(case):
    p, t, loss = _run(case)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference(case)
    _bound(f"case {case} loss", loss, l64, l32)
    _bound(f"case {case} grad pred", p.grad, gp64, gp32)
    _bound(f"case {case} grad target", t.grad, gt64, gt32)


@pytest.mark.parametrize("bins,sigma", BINS_SIGMA)
def test_bins_and_sigma_ratio(bins, sigma):
    p, t, loss = _run("b", bins, sigma)
    loss.backward()
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference("b", bins, sigma)
    _bound(f"bins {bins} sigma {sigma} loss", loss, l64, l32)
    _bound(f"bins {bins} sigma {sigma} grad pred", p.grad, gp64, gp32)
    _bound(f"bins {bins} sigma {sigma} grad target", t.grad, gt64, gt32)


@pytest.mark.parametrize("case,bins", [("a", 23), ("b", 23), ("b", 32), ("b", 2), ("c", 23), ("d", 23)])
def test_parzen_joint_histogram(case, bins):
    pred, target = _inputs(case)
    got = losses.parzen_joint_histogram(_dev(pred, case), _dev(target, case), bins)
    assert got.dtype == torch.float64 and tuple(got.shape) == (pred.shape[0], bins, bins)
    j64, _, _ = R.joint(pred, target, bins)
    j32, _, _ = R.joint(pred, target, bins, dtype=torch.float32)
    _bound(f"joint case {case} bins {bins}", got, j64, j32)
    assert float((got.sum(dim=(1, 2)) - 1.0).abs().max()) <= 1e-6


def test_clamp_edges_keep_their_gradient_and_outside_is_zero():
    p, t, loss = _run("a")
    loss.backward()
    (_, gp64, _), (_, gp32, _) = _reference("a")
    got, want = p.grad[0].reshape(-1).cpu(), gp64[0].reshape(-1)
    (i0, _), (i1, _), (ilo, _), (ihi, _) = R.PLANTED
    assert got[ilo] == 0 and got[ihi] == 0
    outside = ((_inputs("a")[0] < 0) | (_inputs("a")[0] > 1))
    assert int(outside.sum()) >= 2 and bool((p.grad.cpu()[outside] == 0).all())
    for i in (i0, i1):
        assert want[i] != 0 and got[i] != 0
    idx = torch.tensor([i0, i1])
    _bound("edge samples 0.0 and 1.0", got[idx], want[idx], gp32[0].reshape(-1)[idx])


def test_value_range_minus_one_to_one():
    """Inputs on a 2^-12 grid, so that 2x - 1 and its inverse are exact in fp32: the (-1, 1) call then maps to the very
    values of the (0, 1) call, and its gradient factor 1 / (hi - lo) is exactly one half."""
    pred, target = _inputs("b")
    pred, target = torch.round(pred * 4096) / 4096, torch.round(target * 4096) / 4096
    p, t = pred.cuda().requires_grad_(True), target.cuda().requires_grad_(True)
    loss = losses.global_mutual_information_loss(p, t)
    loss.backward()
    p2 = (2 * pred - 1).cuda().requires_grad_(True)
    t2 = (2 * target - 1).cuda().requires_grad_(True)
    loss2 = losses.global_mutual_information_loss(p2, t2, value_range=(-1.0, 1.0))
    loss2.backward()
    assert torch.equal(loss2, loss)
    assert float(p.grad.abs().max()) > 0 and torch.equal(2 * p2.grad, p.grad) and torch.equal(2 * t2.grad, t.grad)
    # separate ranges per tensor
    loss3 = losses.global_mutual_information_loss(p2.detach(), t.detach(), value_range=((-1.0, 1.0), (0.0, 1.0)))
    assert torch.equal(loss3, loss.detach())


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_reductions_upstream_and_second_backward(reduction):
    p, t, loss = _run("b", reduction=reduction)
    (l64, gp64, gt64), (l32, gp32, gt32) = _reference("b", reduction=reduction)
    assert tuple(loss.shape) == ((3,) if reduction == "none" else ())
    _bound(f"{reduction} loss", loss, l64, l32)
    out = loss.sum() if reduction == "none" else loss
    out.backward(retain_graph=True)
    g1p, g1t = p.grad.clone(), t.grad.clone()
    _bound(f"{reduction} grad pred", g1p, gp64, gp32)     # "none" summed over the items: the gradient of "sum"
    _bound(f"{reduction} grad target", g1t, gt64, gt32)
    p.grad = t.grad = None
    out.backward(retain_graph=True)                      # a second backward reads unscaled saved state
    assert torch.equal(p.grad, g1p) and torch.equal(t.grad, g1t)
    p.grad = t.grad = None
    (3 * out).backward()                                 # the upstream scalar enters as one more fp32 factor: a few ulps
    assert float((p.grad - 3 * g1p).abs().max()) <= 4 * 2.0 ** -23 * 3 * float(g1p.abs().max())
    assert float((t.grad - 3 * g1t).abs().max()) <= 4 * 2.0 ** -23 * 3 * float(g1t.abs().max())


def test_only_the_requested_gradient_is_computed():
    pred, target = _inputs("b")
    p, t = pred.cuda().requires_grad_(True), target.cuda()
    losses.global_mutual_information_loss(p, t).backward()
    (_, gp64, _), (_, gp32, _) = _reference("b")
    _bound("pred only", p.grad, gp64, gp32)
    p2, t2 = pred.cuda(), target.cuda().requires_grad_(True)
    losses.global_mutual_information_loss(p2, t2).backward()
    assert p2.grad is None
    (_, _, gt64), (_, _, gt32) = _reference("b")
    _bound("target only", t2.grad, gt64, gt32)
    assert not losses.global_mutual_information_loss(pred.cuda(), target.cuda()).requires_grad


def test_nan_stays_inside_its_item():
    pred, target = _inputs("a")
    bad = pred.clone()
    bad[0].reshape(-1)[100] = float("nan")
    got = losses.global_mutual_information_loss(bad.cuda(), target.cuda(), reduction="none").cpu()
    assert torch.isnan(got[0]) and torch.isfinite(got[1])
    (l64, _, _), (l32, _, _) = _reference("a", reduction="none")
    _bound("item beside the NaN item", got[1], l64[1], l32[1])
    got = losses.global_mutual_information_loss(target.cuda(), bad.cuda(), reduction="none").cpu()   # NaN in the target
    assert torch.isnan(got[0]) and torch.isfinite(got[1])


@pytest.mark.parametrize("case", ["b", "c"])
def test_bitwise_reproducible(case):
    runs = []
    for _ in range(2):
        p, t, loss = _run(case)
        loss.backward()
        runs.append((loss.detach().clone(), p.grad.clone(), t.grad.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_graph_capture_replays_the_eager_result():
    pred, target = _inputs("b")
    p, t, loss = _run("b")
    loss.backward()
    sp, st = pred.cuda().requires_grad_(True), target.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up off the default stream, as capture requires
        (g,) = torch.autograd.grad(losses.global_mutual_information_loss(sp, st), sp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # one stream, one linear chain of launches
        s_loss = losses.global_mutual_information_loss(sp, st)
        (s_grad,) = torch.autograd.grad(s_loss, sp)
    s_loss.detach().zero_()
    s_grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s_loss.detach(), loss.detach()) and torch.equal(s_grad, p.grad)


# ---- the trainer's opt-in term (variant A), at the smallest 2-D shape the GAN tests use ----
def _gan(**kw):
    from mpgan_amd.gan import GAN
    torch.manual_seed(0)
    return GAN(1, 64, 64, dimensions=2, n_unet_blocks=2, **kw)


@functools.lru_cache(maxsize=None)
def _batch():
    g = torch.Generator().manual_seed(5)
    return {k: (torch.rand(2, 1, 64, 64, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}


def _fit(**kw):
    m = _gan(**kw)
    opts, _ = m.configure_optimizers()
    # the D step's loss before any update: inside fit_batch it follows the generator's update, which the term is
    # meant to change, so only a D step from equal weights can show that the step itself computes what it did
    d_first = m.training_step(_batch(), 0, 1).detach().clone()
    log = {k: v.clone() for k, v in m.fit_batch(_batch(), 0, opts).items()}
    return m, log, d_first, m.generator.store.flat_grad.clone()


def test_trainer_default_is_unchanged_and_weight_adds_the_term():
    base, log0, d0, grad0 = _fit()
    zero, log1, d1, grad1 = _fit(mi_weight=0.0)
    assert set(log0) == set(log1) and "g_mi_loss" not in log0
    for k in log0:
        assert torch.equal(log0[k], log1[k]), k
    assert torch.equal(grad0, grad1)
    for a, b in ((base.generator, zero.generator), (base.discriminator, zero.discriminator)):
        assert torch.equal(a.store.flat, b.store.flat)
    assert "val_g_mi_loss" not in base.validation_step(_batch(), 0)

    mi, log2, d2, grad2 = _fit(mi_weight=0.5)
    assert "g_mi_loss" in log2 and bool(torch.isfinite(log2["g_mi_loss"]))
    want = float(log2["g_adv_loss"]) + float(log2["g_recon_loss"]) + 0.5 * float(log2["g_mi_loss"])
    assert abs(float(log2["g_loss"]) - want) <= 4 * 2.0 ** -23 * max(abs(want), 1.0)
    for k in ("g_adv_loss", "g_recon_loss"):                        # the G step's forward is the same launches
        assert torch.equal(log2[k], log0[k]), k
    assert torch.equal(d2, d0)                                      # the D step computes what it did
    assert not torch.equal(grad2, grad0) and bool(torch.isfinite(grad2).all())
    val = mi.validation_step(_batch(), 0)
    assert "val_g_mi_loss" in val and "val_g_mi_loss" in mi.logged
    want = float(val["val_g_adv_loss"]) + float(val["val_g_recon_loss"]) + 0.5 * float(val["val_g_mi_loss"])
    assert abs(float(val["val_g_loss"]) - want) <= 4 * 2.0 ** -23 * max(abs(want), 1.0)
    # the logged term is the loss of the module on the generator's output over the tanh range
    with torch.no_grad():
        from mpgan_amd.gan import eval_modes
        with eval_modes(mi.generator):
            fake = mi(_batch()["t1w"])
    direct = losses.GlobalMutualInformationLoss(23, value_range=(-1.0, 1.0))(fake, _batch()["t2w"])
    assert torch.equal(direct, val["val_g_mi_loss"])
