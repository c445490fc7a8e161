"""References of the foreground-mask kernels (csrc/foreground.hip): numpy restatements of the four definitions in
include/mpgan_hip.h ("foreground masks") -- the binning in np.float32 exactly as written, everything else in float64 --
and a float64 torch restatement of the mask-weighted L1 for autograd.  Also the inputs the GPU tests share, with the
conditions on them that are checked on the CPU (test_foreground_host.py)."""
import functools

import numpy as np
import torch

SHAPES = ((1, 1, 1, 5, 7),        # 2-D, smaller than one group of four
          (2, 1, 3, 17, 19),      # item length 969: item 1 starts unaligned for 16-byte access
          (3, 1, 17, 19, 23),
          (2, 1, 40, 33, 35),     # 46200 values per item: several blocks per item
          (1, 1, 9, 1, 1))        # W = 1
BINS = (2, 64, 256)
WEIGHTS = ((1.0, 0.0), (1.0, 1.0), (2.0, 0.5))
REDUCTIONS = ("mean", "sum", "none")
SIGMA_GAP = 1e-9


# ---- Otsu ---------------------------------------------------------------------------------------------------------------
def histogram(x, lo, hi, bins):
    """int64 counts of one item by mpgan_joint_histogram's rule, in np.float32 as written."""
    v = np.asarray(x, dtype=np.float32).ravel()
    lo32, hi32 = np.float32(lo), np.float32(hi)
    s = np.float32(bins) / (hi32 - lo32)
    with np.errstate(invalid="ignore"):
        ok = (v >= lo32) & (v <= hi32)                   # NaN fails both
    v = v[ok]
    idx = np.floor((v - lo32) * s).astype(np.int64)      # float32 subtract, float32 multiply, floorf
    return np.bincount(np.minimum(idx, bins - 1), minlength=bins).astype(np.int64)


def centre(k, lo, hi, bins):
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return lo + (k + 0.5) * (hi - lo) / bins


def otsu_variances(counts, lo, hi):
    """var_k for k = 0 .. bins - 2 in float64, in the header's order of additions."""
    bins = len(counts)
    c = [centre(k, lo, hi, bins) for k in range(bins)]
    n = [int(v) for v in counts]
    total = sum(n)
    suf = [0.0] * (bins + 1)
    s = 0.0
    for j in range(bins - 1, 0, -1):
        s += float(n[j]) * c[j]
        suf[j] = s
    out, w0, s0 = [], 0, 0.0
    for k in range(bins - 1):
        w0 += n[k]
        s0 += float(n[k]) * c[k]
        w1 = total - w0
        var = 0.0
        if w0 and w1:
            d = s0 / float(w0) - suf[k + 1] / float(w1)
            var = (float(w0) * float(w1)) * (d * d)
        out.append(var)
    return out


def otsu_from_counts(counts, lo, hi):
    """np.float32 threshold of one histogram: NaN without counts, the centre of a single occupied bin, else the centre
    of the first bin that attains the largest var_k."""
    bins = len(counts)
    occupied = np.flatnonzero(np.asarray(counts))
    if len(occupied) == 0:
        return np.float32(np.nan)
    if len(occupied) == 1:
        return np.float32(centre(int(occupied[0]), lo, hi, bins))
    var = otsu_variances(counts, lo, hi)
    return np.float32(centre(int(np.argmax(var)), lo, hi, bins))       # argmax: the first maximum


def otsu_threshold(x, lo, hi, bins):
    return otsu_from_counts(histogram(x, lo, hi, bins), lo, hi)


def sigma_gap(counts, lo, hi):
    """Relative distance of the two largest var_k (inf when there is one bin boundary only)."""
    var = sorted(otsu_variances(counts, lo, hi), reverse=True)
    if len(var) < 2:
        return float("inf")
    return (var[0] - var[1]) / var[0] if var[0] > 0 else 0.0


def bimodal(shape, bins, seed, lo=-1.0, hi=1.0):
    """fp32 items with a different two-mode mixture each, built so that var_k has ONE clear maximum: var_k is constant
    across a run of empty bins, so the bins around the best boundary must be occupied.  An item with at least 12 values
    per bin is continuous: two wide Gaussians over a uniform floor, one value exactly at lo and one at hi.  A smaller
    item sits on the centres of n // 4 CONSECUTIVE bins, every one of them occupied, at the bottom of the range with one
    value exactly at lo (even items) or at its top with one exactly at hi (odd items).  From 40 values on, a few lie
    outside the range and a few are NaN."""
    rng = np.random.RandomState(seed)
    batch, chans = shape[:2]
    n = int(np.prod(shape[2:]))
    out = np.empty((batch * chans, n), dtype=np.float32)
    span = hi - lo
    for i in range(batch * chans):
        share = 0.3 + 0.1 * (i % 4)                                        # share of the upper mode
        if n >= 12 * bins:
            low, high = lo + span * (0.25 + 0.04 * (i % 3)), lo + span * (0.68 + 0.05 * (i % 4))
            v = np.where(rng.rand(n) < share, high, low) + 0.1 * span * rng.randn(n)
            flat = rng.rand(n) < 0.1
            v[flat] = lo + span * rng.rand(int(flat.sum()))
            v = np.clip(v, lo, hi)
            v[0], v[n - 1] = lo, hi
            keep = 1
        else:
            g = max(2, min(bins, n // 4))
            j0 = 0 if i % 2 == 0 else bins - g
            q = np.where(rng.rand(n) < share, g - 1 - rng.binomial(g - 1, 0.15, n), rng.binomial(g - 1, 0.15, n))
            q[:g] = np.arange(g)                                           # every bin of the run is occupied
            v = np.array([centre(j0 + int(k), lo, hi, bins) for k in q])
            v[0 if i % 2 == 0 else g - 1] = lo if i % 2 == 0 else hi       # bin 0 / the last bin, by its edge value
            keep = g
        if n >= 40:
            v[rng.randint(keep, n - 1, size=3)] = hi + 0.5 * span          # dropped
            v[rng.randint(keep, n - 1, size=3)] = lo - 0.5 * span          # dropped
            v[rng.randint(keep, n - 1, size=2)] = np.nan                   # dropped
        out[i] = v.astype(np.float32)
    return out.reshape(shape)


@functools.lru_cache(maxsize=None)
def otsu_case(shape, bins, lo=-1.0, hi=1.0):
    """(x, per-item counts, thresholds) of the shared bimodal input; read-only."""
    x = bimodal(shape, bins, seed=100 + len(shape) + sum(shape) + bins)
    x.setflags(write=False)
    flat = x.reshape(shape[0] * shape[1], -1)
    counts = [histogram(row, lo, hi, bins) for row in flat]
    thr = np.array([otsu_from_counts(c, lo, hi) for c in counts], dtype=np.float32)
    return x, counts, thr


# ---- mask, count, box ---------------------------------------------------------------------------------------------------
def foreground(x, thr):
    """uint8 mask of a (items, D, H, W) array against per-item np.float32 thresholds: strict, fp32, NaN is background."""
    x = np.asarray(x, dtype=np.float32)
    t = np.asarray(thr, dtype=np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    with np.errstate(invalid="ignore"):
        return (x > t).astype(np.uint8)


def bounding_box(mask, margin=(0, 0, 0)):
    """MONAI's generate_spatial_bounding_box of one (D, H, W) mask: int32 (2, 3); zeros without foreground."""
    mask = np.asarray(mask) != 0
    box = np.zeros((2, 3), dtype=np.int32)
    if not mask.any():
        return box
    for d in range(3):
        other = tuple(a for a in range(3) if a != d)
        hit = np.flatnonzero(mask.any(axis=other))
        box[0, d] = max(int(hit[0]) - int(margin[d]), 0)
        box[1, d] = min(int(hit[-1]) + 1 + int(margin[d]), mask.shape[d])
    return box


def bounding_box_brute(mask, margin=(0, 0, 0)):
    """The same box from np.argwhere."""
    idx = np.argwhere(np.asarray(mask) != 0)
    box = np.zeros((2, 3), dtype=np.int32)
    if len(idx) == 0:
        return box
    for d in range(3):
        box[0, d] = max(int(idx[:, d].min()) - int(margin[d]), 0)
        box[1, d] = min(int(idx[:, d].max()) + 1 + int(margin[d]), np.asarray(mask).shape[d])
    return box


# ---- mask-weighted L1 ---------------------------------------------------------------------------------------------------
def masked_l1_torch(pred, target, mask, w_fg, w_bg, reduction):
    """float64 torch restatement: pred, target (B, C, *S) float64 tensors (autograd flows), mask a bool tensor of
    their shape."""
    batch, chans = pred.shape[:2]
    w = torch.where(mask, torch.tensor(float(w_fg), dtype=torch.float64), torch.tensor(float(w_bg), dtype=torch.float64))
    num = (w * (pred - target).abs()).reshape(batch * chans, -1).sum(dim=1)
    den = w.reshape(batch * chans, -1).sum(dim=1)
    item = torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(num))
    if reduction == "mean":
        return item.mean()
    if reduction == "sum":
        return item.sum()
    return item.reshape(batch, chans).mean(dim=1)


def masked_l1_grad(pred, target, mask, w_fg, w_bg, reduction, gout=None):
    """The closed form of the header: d loss / d pred as a float64 array (d target is its negative).  gout: the
    upstream gradient, a scalar or (B,) for reduction "none"; default ones."""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    batch, chans = pred.shape[:2]
    items = batch * chans
    w = np.where(np.asarray(mask) != 0, float(w_fg), float(w_bg)).reshape(items, -1)
    den = w.sum(axis=1)
    scale = {"mean": 1.0 / items, "sum": 1.0, "none": 1.0 / chans}[reduction]
    up = np.ones(batch) if gout is None else np.broadcast_to(np.asarray(gout, dtype=np.float64), (batch,))
    up = np.repeat(up, chans)
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = np.where(den > 0, up * scale / den, 0.0)
    grad = coef[:, None] * w * np.sign(pred - target).reshape(items, -1)
    grad[den == 0] = 0.0
    return grad.reshape(pred.shape)


def masked_l1_numpy(pred, target, mask, w_fg, w_bg, reduction):
    with torch.no_grad():
        out = masked_l1_torch(torch.from_numpy(np.asarray(pred, dtype=np.float64)),
                              torch.from_numpy(np.asarray(target, dtype=np.float64)),
                              torch.from_numpy(np.asarray(mask) != 0), w_fg, w_bg, reduction)
    return out.numpy()


@functools.lru_cache(maxsize=None)
def l1_case(shape):
    """(pred, target, thr) fp32: target the bimodal input (NaN and out-of-range values replaced), pred target plus
    noise with a fifth of the positions left equal; thr the per-item Otsu thresholds at 256 bins."""
    x = np.nan_to_num(bimodal(shape, 256, seed=300 + sum(shape)), nan=-1.0)
    target = np.clip(x, -1.0, 1.0).astype(np.float32)
    rng = np.random.RandomState(400 + sum(shape))
    pred = np.clip(target + 0.2 * rng.randn(*shape), -1.0, 1.0).astype(np.float32)
    same = rng.rand(*shape) < 0.2
    pred[same] = target[same]
    flat = target.reshape(shape[0] * shape[1], -1)
    thr = np.array([otsu_threshold(row, -1.0, 1.0, 256) for row in flat], dtype=np.float32)
    for a in (pred, target, thr):
        a.setflags(write=False)
    return pred, target, thr


# ---- masked errors ------------------------------------------------------------------------------------------------------
def masked_errors(a, b, mask, data_range):
    """(MAE, MSE, PSNR, count) in float64 over the voxels whose mask is non-zero; NaN, NaN, NaN, 0 for none."""
    m = np.asarray(mask).ravel() != 0
    n = int(m.sum())
    if n == 0:
        return float("nan"), float("nan"), float("nan"), 0
    d = np.asarray(a, dtype=np.float64).ravel()[m] - np.asarray(b, dtype=np.float64).ravel()[m]
    mae, mse = float(np.abs(d).sum() / n), float((d * d).sum() / n)
    psnr = 10.0 * np.log10(float(data_range) ** 2 / mse) if mse > 0 else float("inf")
    return mae, mse, float(psnr), n
