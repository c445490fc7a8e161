"""numpy restatement of mpgan_amd.metrics.joint_histogram / mutual_information (include/mpgan_hip.h):
the fp32 binning rule in np.float32 arithmetic, int64 counts via np.bincount, entropies in float64."""
import numpy as np

MASK_MODES = (None, "both_nonzero", "either_nonzero")


def _ranges(value_range):
    if isinstance(value_range[0], (tuple, list)):
        (lo_a, hi_a), (lo_b, hi_b) = value_range
    else:
        lo_a, hi_a = value_range
        lo_b, hi_b = value_range
    return np.float32(lo_a), np.float32(hi_a), np.float32(lo_b), np.float32(hi_b)


def bin_index(v, lo, hi, bins):
    """(idx, inside): idx = min(floor((v - lo) * s), bins - 1), s = bins / (hi - lo), every step in fp32;
    inside is False for a value below lo, above hi or NaN (its idx is meaningless)."""
    v = np.asarray(v, dtype=np.float32).ravel()
    lo, hi = np.float32(lo), np.float32(hi)
    s = np.float32(bins) / (hi - lo)
    assert s.dtype == np.float32
    with np.errstate(invalid="ignore"):
        inside = (v >= lo) & (v <= hi)
        t = (np.where(inside, v, lo) - lo) * s
    assert t.dtype == np.float32
    idx = np.minimum(np.floor(t).astype(np.int64), bins - 1)
    return idx, inside


def joint_histogram(a, b, bins=256, value_range=(0.0, 256.0), mask=None):
    """int64 (bins, bins) counts of one image pair; rows are a's bins."""
    a = np.asarray(a, dtype=np.float32).ravel()
    b = np.asarray(b, dtype=np.float32).ravel()
    lo_a, hi_a, lo_b, hi_b = _ranges(value_range)
    ia, in_a = bin_index(a, lo_a, hi_a, bins)
    ib, in_b = bin_index(b, lo_b, hi_b, bins)
    keep = in_a & in_b
    if isinstance(mask, str):
        keep &= ((a != 0) & (b != 0)) if mask == "both_nonzero" else ((a != 0) | (b != 0))
        assert mask in ("both_nonzero", "either_nonzero")
    elif mask is not None:
        keep &= np.asarray(mask).ravel() != 0
    return np.bincount(ia[keep] * bins + ib[keep], minlength=bins * bins).astype(np.int64).reshape(bins, bins)


def _sum_clogc(counts):
    c = counts[counts > 0].astype(np.float64)
    return float(np.sum(c * np.log(c)))


def mutual_information_from_histogram(hist):
    """{"mi", "h_a", "h_b", "h_ab", "nmi", "count"} in float64 (nats): H = log N - (sum c log c) / N."""
    hist = np.asarray(hist, dtype=np.int64)
    n = int(hist.sum())
    if n == 0:
        nan = float("nan")
        return {"mi": nan, "h_a": nan, "h_b": nan, "h_ab": nan, "nmi": nan, "count": 0.0}
    if np.count_nonzero(hist) == 1:               # every voxel in one bin: H_ab == 0
        return {"mi": 0.0, "h_a": 0.0, "h_b": 0.0, "h_ab": 0.0, "nmi": 1.0, "count": float(n)}
    ln = float(np.log(np.float64(n)))
    h_a = ln - _sum_clogc(hist.sum(axis=1)) / n
    h_b = ln - _sum_clogc(hist.sum(axis=0)) / n
    h_ab = ln - _sum_clogc(hist.ravel()) / n
    return {"mi": h_a + h_b - h_ab, "h_a": h_a, "h_b": h_b, "h_ab": h_ab, "nmi": (h_a + h_b) / h_ab,
            "count": float(n)}


def mutual_information(a, b, bins=256, value_range=(0.0, 256.0), mask=None):
    return mutual_information_from_histogram(joint_histogram(a, b, bins, value_range, mask))


def mri_like_pair(shape, seed):
    """Integer-valued levels 0..255 with 60 % of the voxels of `a` set to 0, and b = clip(rint(0.7 a + N(0, 20)), 0, 255):
    most voxels fall into bin (0, 0) or next to it, as the background of an MRI volume does."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    a = rng.integers(0, 256, n).astype(np.float32)
    a[rng.random(n) < 0.6] = 0.0
    b = np.clip(np.rint(0.7 * a + rng.normal(0.0, 20.0, n)), 0, 255).astype(np.float32)
    return a.reshape(shape), b.reshape(shape)


def continuous_pair(shape, seed):
    """Correlated continuous values in [-1, 1]."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    a = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    b = np.clip(0.6 * a + 0.4 * rng.uniform(-1.0, 1.0, n), -1.0, 1.0).astype(np.float32)
    return a.reshape(shape), b.reshape(shape)
