"""Plain-torch restatement of the SSIM loss (include/mpgan_hip.h states the definition: the structural similarity of
oracle/metrics_ref.structural_similarity per (batch, channel) image, as 1 - ssim).  The valid box sums are conv2d /
conv3d with a ones kernel.  Run in float64 it is the yardstick of the kernels; run in float32 it is their peer.
analytic_gradients() is the closed form the backward kernel implements."""
import torch
import torch.nn.functional as F

WIN = 7
K1, K2 = 0.01, 0.03


def _box(x, d):
    """Sum over every 7^d window lying inside the image; x: (items, 1, *spatial)."""
    ones = torch.ones((1, 1) + (WIN,) * d, dtype=x.dtype, device=x.device)
    return (F.conv2d if d == 2 else F.conv3d)(x, ones)


def _full_box(m, d):
    """For every sample, the sum of m over the valid windows that contain it (m zero-extended): (items, 1, *spatial)."""
    ones = torch.ones((1, 1) + (WIN,) * d, dtype=m.dtype, device=m.device)
    return (F.conv2d if d == 2 else F.conv3d)(m, ones, padding=WIN - 1)


def _items(x, lo, dtype):
    spatial = tuple(x.shape[2:])
    if len(spatial) == 3 and spatial[0] == 1:
        spatial = spatial[1:]
    return x.to(dtype).reshape((-1, 1) + spatial) - lo, len(spatial)


def _window_terms(a, b, d, data_range):
    n = float(WIN ** d)
    cn = n / (n - 1.0)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    ux, uy = _box(a, d) / n, _box(b, d) / n
    vx = cn * (_box(a * a, d) / n - ux * ux)
    vy = cn * (_box(b * b, d) / n - uy * uy)
    vxy = cn * (_box(a * b, d) / n - ux * uy)
    a1, a2 = 2 * ux * uy + c1, 2 * vxy + c2
    b1, b2 = ux * ux + uy * uy + c1, vx + vy + c2
    return n, cn, ux, uy, a1, a2, b1, b2, (a1 * a2) / (b1 * b2)


def ssim_items(pred, target, value_range=(0.0, 1.0), dtype=torch.float64):
    """ssim of every (b, c) image, shape (B, C)."""
    lo, hi = float(value_range[0]), float(value_range[1])
    a, d = _items(pred, lo, dtype)
    b, _ = _items(target, lo, dtype)
    s = _window_terms(a, b, d, hi - lo)[-1]
    return s.reshape(s.shape[0], -1).mean(dim=1).reshape(pred.shape[0], pred.shape[1])


def loss(pred, target, value_range=(0.0, 1.0), reduction="mean", dtype=torch.float64):
    per_item = 1.0 - ssim_items(pred, target, value_range, dtype)
    if reduction == "mean":
        return per_item.mean()
    if reduction == "sum":
        return per_item.sum()
    if reduction == "none":
        return per_item.mean(dim=1)
    raise ValueError(reduction)


def loss_and_gradients(pred, target, dtype=torch.float64, **kw):
    """(loss, d/dpred, d/dtarget) by autograd in `dtype` ("none" is summed over the batch for the gradients)."""
    p = pred.detach().to(dtype).requires_grad_(True)
    t = target.detach().to(dtype).requires_grad_(True)
    out = loss(p, t, dtype=dtype, **kw)
    gp, gt = torch.autograd.grad(out.sum(), (p, t))
    return out.detach(), gp, gt


def analytic_gradients(pred, target, value_range=(0.0, 1.0), dtype=torch.float64):
    """(d ssim_item / d pred, d ssim_item / d target) of every item by the closed form, in the inputs' shape."""
    lo, hi = float(value_range[0]), float(value_range[1])
    a, d = _items(pred, lo, dtype)
    b, _ = _items(target, lo, dtype)
    n, cn, ux, uy, a1, a2, b1, b2, s = _window_terms(a, b, d, hi - lo)
    q = -2.0 * cn * s / b2
    r = 2.0 * cn * a1 / (b1 * b2)
    pa = 2.0 * uy * a2 / (b1 * b2) - 2.0 * ux * s / b1 - ux * q - uy * r
    pb = 2.0 * ux * a2 / (b1 * b2) - 2.0 * uy * s / b1 - uy * q - ux * r
    m = float(s[0].numel())
    ga = (_full_box(pa, d) + a * _full_box(q, d) + b * _full_box(r, d)) / (n * m)
    gb = (_full_box(pb, d) + b * _full_box(q, d) + a * _full_box(r, d)) / (n * m)
    return ga.reshape(pred.shape), gb.reshape(target.shape)


def structured_pair(shape, seed=0):
    """(pred, target) fp32 on the CPU with values in [-1, 1]: target uniform, pred = 0.7 target + 0.3 noise; about
    30 % of the samples are exactly -1 in both (an MR background), and both carry a planted constant block of value
    0.8 that is 9 wide on every spatial axis of extent >= 9 (3 wide on a shorter one), so that with every extent >= 9 some
    windows have exactly zero variance and the gradient's flat-region cancellation is exercised."""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(shape, generator=g) * 2 - 1
    noise = torch.rand(shape, generator=g) * 2 - 1
    pred = 0.7 * target + 0.3 * noise
    background = torch.rand(shape, generator=g) < 0.3
    pred[background] = -1.0
    target[background] = -1.0
    block = (slice(None), slice(None)) + tuple(slice((s - 9) // 2, (s - 9) // 2 + 9) if s >= 9 else slice(2, 5)
                                               for s in shape[2:])
    pred[block] = 0.8
    target[block] = 0.8
    return pred.contiguous(), target.contiguous()
