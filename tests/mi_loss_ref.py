"""Plain-torch restatement of the Parzen-window mutual-information loss (include/mpgan_hip.h states the definition;
it follows MONAI 0.4.0's GlobalMutualInformationLoss with a value range in addition).  Run in float64 it is the
yardstick of the kernels; run in float32 it is their peer: the same arithmetic in the same precision, summed in
torch's order.  analytic_gradients() is the closed form the backward kernel implements."""
import torch


def _ranges(value_range):
    if isinstance(value_range[0], (tuple, list)):
        (lo_a, hi_a), (lo_b, hi_b) = value_range
    else:
        lo_a, hi_a = value_range
        lo_b, hi_b = value_range
    return float(lo_a), float(hi_a), float(lo_b), float(hi_b)


def _mapped(x, lo, hi, dtype):
    x = x.to(dtype).reshape(x.shape[0], -1, 1)                     # (B, N, 1): channels fold into samples
    return torch.clamp((x - lo) / (hi - lo), 0.0, 1.0)


def _weights(xm, num_bins, sigma_ratio):
    centres = (torch.arange(num_bins, dtype=torch.float64) / (num_bins - 1)).to(xm.dtype).reshape(1, 1, -1).to(xm.device)
    sigma = sigma_ratio / (num_bins - 1)
    preterm = 1.0 / (2.0 * sigma * sigma)
    e = torch.exp(-preterm * (xm - centres) ** 2)
    return e / e.sum(dim=-1, keepdim=True), centres, preterm       # (B, N, K)


def joint(pred, target, num_bins=23, sigma_ratio=0.5, value_range=(0.0, 1.0), dtype=torch.float64):
    """(pab (B, K, K), pa (B, K), pb (B, K)); the marginals are the sample means of the weights, as MONAI forms them."""
    lo_a, hi_a, lo_b, hi_b = _ranges(value_range)
    wa, _, _ = _weights(_mapped(pred, lo_a, hi_a, dtype), num_bins, sigma_ratio)
    wb, _, _ = _weights(_mapped(target, lo_b, hi_b, dtype), num_bins, sigma_ratio)
    n = wa.shape[1]
    pab = torch.bmm(wa.transpose(1, 2), wb) / n
    return pab, wa.mean(dim=1), wb.mean(dim=1)


def mutual_information(pred, target, num_bins=23, sigma_ratio=0.5, value_range=(0.0, 1.0), smooth_nr=1e-7,
                       smooth_dr=1e-7, dtype=torch.float64):
    """mi of every item, shape (B,)."""
    pab, pa, pb = joint(pred, target, num_bins, sigma_ratio, value_range, dtype)
    papb = torch.bmm(pa.unsqueeze(2), pb.unsqueeze(1))
    return torch.sum(pab * torch.log((pab + smooth_nr) / (papb + smooth_dr) + smooth_dr), dim=(1, 2))


def loss(pred, target, num_bins=23, sigma_ratio=0.5, reduction="mean", value_range=(0.0, 1.0), smooth_nr=1e-7,
         smooth_dr=1e-7, dtype=torch.float64):
    mi = mutual_information(pred, target, num_bins, sigma_ratio, value_range, smooth_nr, smooth_dr, dtype)
    if reduction == "mean":
        return -mi.mean()
    if reduction == "sum":
        return -mi.sum()
    if reduction == "none":
        return -mi
    raise ValueError(reduction)


def loss_and_gradients(pred, target, dtype=torch.float64, upstream=None, **kw):
    """(loss, d/dpred, d/dtarget) by autograd in `dtype`; the gradients come back in the inputs' shape."""
    p = pred.detach().to(dtype).requires_grad_(True)
    t = target.detach().to(dtype).requires_grad_(True)
    out = loss(p, t, dtype=dtype, **kw)
    up = torch.ones_like(out) if upstream is None else torch.as_tensor(upstream, dtype=dtype).expand_as(out)
    gp, gt = torch.autograd.grad(out, (p, t), up)
    return out.detach(), gp, gt


def analytic_gradients(pred, target, num_bins=23, sigma_ratio=0.5, value_range=(0.0, 1.0), smooth_nr=1e-7,
                       smooth_dr=1e-7, dtype=torch.float64):
    """(d mi_b / d pred, d mi_b / d target) of every item by the closed form, in the inputs' shape."""
    lo_a, hi_a, lo_b, hi_b = _ranges(value_range)
    nr, dr = smooth_nr, smooth_dr
    ta = (pred.to(dtype).reshape(pred.shape[0], -1, 1) - lo_a) / (hi_a - lo_a)
    tb = (target.to(dtype).reshape(target.shape[0], -1, 1) - lo_b) / (hi_b - lo_b)
    xa, xb = torch.clamp(ta, 0.0, 1.0), torch.clamp(tb, 0.0, 1.0)
    wa, centres, p = _weights(xa, num_bins, sigma_ratio)
    wb, _, _ = _weights(xb, num_bins, sigma_ratio)
    n = wa.shape[1]
    pab = torch.bmm(wa.transpose(1, 2), wb) / n
    pa, pb = pab.sum(dim=2), pab.sum(dim=1)
    papb = pa.unsqueeze(2) * pb.unsqueeze(1)
    r = (pab + nr) / (papb + dr)
    a_ = torch.log(r + dr) + pab / ((r + dr) * (papb + dr))
    dp = -pab * (pab + nr) / ((r + dr) * (papb + dr) ** 2)
    g_a = a_ + (dp * pb.unsqueeze(1)).sum(dim=2, keepdim=True)          # G_ij  = A_ij + sum_j Dp_ij pb_j
    g_b = a_ + (dp * pa.unsqueeze(2)).sum(dim=1, keepdim=True)          # G'_ij = A_ij + sum_i Dp_ij pa_i

    def one(w_x, w_y, g, x, t, span):
        h = torch.bmm(w_y, g.transpose(1, 2))                           # h_i(n) = sum_j g_ij w_y_j(n)
        hbar = (w_x * h).sum(dim=2, keepdim=True)
        inside = ((t >= 0.0) & (t <= 1.0)).to(dtype)                    # the closed interval: torch.clamp's rule
        s = (w_x * (h - hbar) * (-2.0 * p * (x - centres))).sum(dim=2, keepdim=True)
        return s * inside / (n * span)

    grad_a = one(wa, wb, g_a, xa, ta, hi_a - lo_a)
    grad_b = one(wb, wa, g_b.transpose(1, 2), xb, tb, hi_b - lo_b)
    return grad_a.reshape(pred.shape), grad_b.reshape(target.shape)


PLANTED = ((3, 0.0), (11, 1.0), (17, -0.2), (29, 1.3))                  # (flat index inside item 0, value)


def correlated_pair(shape, seed=0, planted=True):
    """(pred, target) fp32 on the CPU: target uniform in [0, 1), pred = 0.6 t + 0.5 rand - 0.05, so that 1-2 % of
    pred falls outside [0, 1]; with planted=True item 0 of pred also holds 0.0, 1.0, -0.2 and 1.3 at PLANTED."""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(shape, generator=g)
    p = 0.6 * t + 0.5 * torch.rand(shape, generator=g) - 0.05
    if planted:
        flat = p[0].reshape(-1)
        for idx, val in PLANTED:
            flat[idx] = val
    return p.contiguous(), t.contiguous()


def independent_pair(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
