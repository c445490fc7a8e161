"""Plain-torch restatement of the masked SSIM (include/mpgan_hip.h: "masked SSIM"), built on ssim_loss_ref.py's
helpers: every valid window carries the weight w = (mask != 0) of its CENTRE voxel, so the weights are the mask
cropped by its 3-sample border on every windowed axis.  Run in float64 it is the yardstick of the kernels; run in
float32 it is their peer.  analytic_gradients() is the closed form the backward kernel implements."""
import torch

import ssim_loss_ref as R

HALF = R.WIN // 2


def window_weights(mask, pred_shape, dtype=torch.float64):
    """(items, 1, *corners) weights in {0, 1}: the mask at every window's centre.  mask: pred's shape, or with channel
    extent 1; any non-zero value counts."""
    m = (torch.as_tensor(mask) != 0).expand(pred_shape)
    m, d = R._items(m, 0.0, dtype)
    crop = (slice(None), slice(None)) + (slice(HALF, -HALF),) * d
    return m[crop], d


def random_mask(shape, seed=0, density=0.5):
    """A seeded uint8 mask: `density` of the voxels non-zero, their bytes drawn from {1, 2, 255}."""
    g = torch.Generator().manual_seed(seed)
    on = torch.rand(shape, generator=g) < density
    value = torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, shape, generator=g)]
    return torch.where(on, value, torch.zeros((), dtype=torch.uint8)).contiguous()


def ssim_map(pred, target, value_range=(0.0, 1.0), dtype=torch.float64):
    """S of every valid window: (B, C, *corners)."""
    lo, hi = float(value_range[0]), float(value_range[1])
    a, d = R._items(pred, lo, dtype)
    b, _ = R._items(target, lo, dtype)
    s = R._window_terms(a, b, d, hi - lo)[-1]
    return s.reshape(tuple(pred.shape[:2]) + tuple(s.shape[2:]))


def items_and_counts(pred, target, mask, value_range=(0.0, 1.0), dtype=torch.float64):
    """(ssim_item, n_item), each (B, C): the weighted mean of S, NaN where no window is weighted, and the exact count."""
    s = ssim_map(pred, target, value_range, dtype)
    w, _ = window_weights(mask, pred.shape, dtype)
    w = w.reshape(s.shape)
    flat = lambda x: x.reshape(x.shape[0], x.shape[1], -1)
    cnt = flat(w).sum(dim=2)
    num = flat(w * s).sum(dim=2)
    nan = torch.full_like(num, float("nan"))
    return torch.where(cnt > 0, num / cnt.clamp(min=1.0), nan), cnt


def loss(pred, target, mask, value_range=(0.0, 1.0), reduction="mean", dtype=torch.float64):
    item, cnt = items_and_counts(pred, target, mask, value_range, dtype)
    per_item = torch.where(cnt > 0, 1.0 - item, torch.zeros_like(item))       # an empty item: loss 0
    if reduction == "mean":
        return per_item.mean()
    if reduction == "sum":
        return per_item.sum()
    if reduction == "none":
        return per_item.mean(dim=1)
    raise ValueError(reduction)


def loss_and_gradients(pred, target, mask, dtype=torch.float64, **kw):
    """(loss, d/dpred, d/dtarget) by autograd in `dtype` ("none" is summed over the batch for the gradients)."""
    p = pred.detach().to(dtype).requires_grad_(True)
    t = target.detach().to(dtype).requires_grad_(True)
    out = loss(p, t, mask, dtype=dtype, **kw)
    if not out.requires_grad:                                 # every item empty: the loss is the constant 0
        return out.detach(), torch.zeros_like(p), torch.zeros_like(t)
    gp, gt = torch.autograd.grad(out.sum(), (p, t))
    return out.detach(), gp, gt


def analytic_gradients(pred, target, mask, value_range=(0.0, 1.0), dtype=torch.float64):
    """(d ssim_item / d pred, d ssim_item / d target) of every item by the closed form; zeros for an empty item."""
    lo, hi = float(value_range[0]), float(value_range[1])
    a, d = R._items(pred, lo, dtype)
    b, _ = R._items(target, lo, dtype)
    w, _ = window_weights(mask, pred.shape, dtype)
    n, cn, ux, uy, a1, a2, b1, b2, s = R._window_terms(a, b, d, hi - lo)
    q = -2.0 * cn * s / b2
    r = 2.0 * cn * a1 / (b1 * b2)
    pa = 2.0 * uy * a2 / (b1 * b2) - 2.0 * ux * s / b1 - ux * q - uy * r
    pb = 2.0 * ux * a2 / (b1 * b2) - 2.0 * uy * s / b1 - uy * q - ux * r
    cnt = w.reshape(w.shape[0], -1).sum(dim=1).reshape((-1,) + (1,) * (a.dim() - 1))
    factor = torch.where(cnt > 0, 1.0 / (n * cnt.clamp(min=1.0)), torch.zeros_like(cnt))
    ga = (R._full_box(w * pa, d) + a * R._full_box(w * q, d) + b * R._full_box(w * r, d)) * factor
    gb = (R._full_box(w * pb, d) + b * R._full_box(w * q, d) + a * R._full_box(w * r, d)) * factor
    return ga.reshape(pred.shape), gb.reshape(target.shape)
