"""Plain-torch restatement of the Sobel edge loss (include/mpgan_hip.h states the definition): replicate padding, the
normalised 3^d Sobel filters as one conv2d / conv3d with d output channels, m = sqrt(sum G_k^2 + eps), the mean of
|m(pred) - m(target)| per (batch, channel) image and the three reductions.  Run in float64 it is the yardstick of the
kernels; run in float32 it is their peer.  analytic_gradients() is the closed form the backward kernels implement,
border folding included, without autograd."""
import torch
import torch.nn.functional as F

from ssim_loss_ref import structured_pair                      # noqa: F401  (the input maker of the edge-loss tests)

DV = (-1.0, 0.0, 1.0)
SV = (1.0, 2.0, 1.0)
EPS = 1e-6
KINK = 1e-5                 # |m(a) - m(b)| below KINK * max m: an fp32 rounding of m (~2e-6 relative) may flip the sign


# The shapes of the device tests (test_edge_loss_gpu.py states what each is for) and the seed of each one's inputs; the
# host test asserts the near-kink cap on exactly these inputs.
CASES = {
    "a": (1, 1, 1, 1), "b": (1, 1, 2, 3), "c": (1, 1, 3, 3), "d": (2, 1, 9, 39), "e": (1, 2, 17, 45),
    "f": (1, 1, 1, 1, 1), "g": (1, 1, 2, 2, 3), "h": (1, 1, 3, 3, 3), "i": (1, 1, 1, 9, 40), "j": (1, 1, 9, 10, 40),
    "k": (2, 1, 13, 21, 37), "l": (1, 1, 13, 17, 41), "m": (1, 1, 21, 37), "n": (1, 1, 12, 24, 96),
}
SEEDS = {case: 40 + i for i, case in enumerate(CASES)}


def case_inputs(case):
    """(pred, target) of a case: fp32 on the CPU, 30 % shared -1 background and a planted flat block."""
    return structured_pair(CASES[case], seed=SEEDS[case])


def filters(d, dtype=torch.float64, normalised=True):
    """(d, 1, 3, ..., 3): filter k differentiates along spatial axis k and smooths along the others."""
    out = []
    for k in range(d):
        w = torch.ones((3,) * d, dtype=dtype)
        for axis in range(d):
            v = torch.tensor(DV if axis == k else SV, dtype=dtype)
            w = w * v.reshape([3 if j == axis else 1 for j in range(d)])
        out.append(w)
    w = torch.stack(out).unsqueeze(1)
    return w / (2.0 * 4.0 ** (d - 1)) if normalised else w


def _items(x, dtype):
    """(items, 1, *spatial) and d; nothing is special-cased: a depth of 1 goes through the 3-D operator."""
    spatial = tuple(x.shape[2:])
    if x.dim() not in (4, 5):
        raise ValueError(f"expects (B, C, H, W) or (B, C, D, H, W), got {tuple(x.shape)}")
    return x.to(dtype).reshape((-1, 1) + spatial), len(spatial)


def gradients(x, dtype=torch.float64, normalised=True):
    """G_k of every item: (items, d, *spatial)."""
    v, d = _items(x, dtype)
    padded = F.pad(v, (1, 1) * d, mode="replicate")
    return (F.conv2d if d == 2 else F.conv3d)(padded, filters(d, dtype, normalised).to(v.device))


def magnitude(x, eps=EPS, dtype=torch.float64):
    """m(x) in the shape of x."""
    g = gradients(x, dtype)
    return torch.sqrt((g * g).sum(dim=1) + eps).reshape(x.shape)


def loss_items(pred, target, eps=EPS, dtype=torch.float64):
    """mean_p |m(pred) - m(target)| of every (b, c) image, shape (B, C)."""
    diff = (magnitude(pred, eps, dtype) - magnitude(target, eps, dtype)).abs()
    return diff.reshape(pred.shape[0], pred.shape[1], -1).mean(dim=2)


def loss(pred, target, eps=EPS, reduction="mean", dtype=torch.float64):
    per_item = loss_items(pred, target, eps, dtype)
    if reduction == "mean":
        return per_item.mean()
    if reduction == "sum":
        return per_item.sum()
    if reduction == "none":
        return per_item.mean(dim=1)
    raise ValueError(reduction)


def loss_and_gradients(pred, target, dtype=torch.float64, eps=EPS, reduction="mean"):
    """(loss, d/dpred, d/dtarget) by autograd in `dtype` ("none" is summed over the batch for the gradients)."""
    p = pred.detach().to(dtype).requires_grad_(True)
    t = target.detach().to(dtype).requires_grad_(True)
    out = loss(p, t, eps, reduction, dtype)
    gp, gt = torch.autograd.grad(out.sum(), (p, t))
    return out.detach(), gp, gt


def magnitude_and_vjp(x, upstream, dtype=torch.float64, eps=EPS):
    """(m(x), d <upstream, m(x)> / dx) by autograd in `dtype`."""
    v = x.detach().to(dtype).requires_grad_(True)
    m = magnitude(v, eps, dtype)
    (gx,) = torch.autograd.grad((m * upstream.to(dtype)).sum(), (v,))
    return m.detach(), gx


def _adjoint(coef, d):
    """dx_p = sum_q sum_k coef[k]_q dG_k(x)_q / dx_p for coef (items, d, *spatial): the transposed taps over the image
    extended by one voxel on every face (coef is zero outside the image), then every face's extension folded onto the
    border voxels it was clamped from."""
    w = torch.flip(filters(d, coef.dtype), dims=tuple(range(2, 2 + d)))
    ext = sum((F.conv2d if d == 2 else F.conv3d)(coef[:, k:k + 1], w[k:k + 1], padding=2) for k in range(d))
    for axis in range(2, 2 + d):                                   # extent n + 2 -> n
        n = ext.shape[axis] - 2
        inner = ext.narrow(axis, 1, n).clone()
        inner.narrow(axis, 0, 1).add_(ext.narrow(axis, 0, 1))
        inner.narrow(axis, n - 1, 1).add_(ext.narrow(axis, n + 1, 1))
        ext = inner
    return ext


def analytic_gradients(pred, target, eps=EPS, dtype=torch.float64):
    """(d loss_item / d pred, d loss_item / d target) of every item by the closed form, in the inputs' shape."""
    ga, gb = gradients(pred, dtype), gradients(target, dtype)
    d = ga.shape[1]
    ma = torch.sqrt((ga * ga).sum(dim=1, keepdim=True) + eps)
    mb = torch.sqrt((gb * gb).sum(dim=1, keepdim=True) + eps)
    s = torch.sign(ma - mb)
    n = float(ma[0].numel())
    da = _adjoint(s * ga / ma, d) / n
    db = _adjoint(-s * gb / mb, d) / n
    return da.reshape(pred.shape), db.reshape(target.shape)


def near_kink_outputs(pred, target, eps=EPS):
    """Bool mask, in the inputs' shape, of the gradient entries that a sign flip at a near-kink voxel can reach: the
    3^d neighbourhood of {q : 0 < |m(pred)_q - m(target)_q| < KINK * max m}, in float64.  An exact tie is left out of
    the set: it arises where both neighbourhoods are flat or equal (G is then computed exactly, in any precision), the
    sign is 0 on both sides, and those entries are compared like every other."""
    ma, mb = magnitude(pred, eps), magnitude(target, eps)
    diff = (ma - mb).abs()
    kink = (diff > 0) & (diff < KINK * max(float(ma.max()), float(mb.max())))
    v, d = _items(kink, torch.float64)
    pool = F.max_pool2d if d == 2 else F.max_pool3d
    return pool(v, 3, stride=1, padding=1).reshape(pred.shape) > 0
