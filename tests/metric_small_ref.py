"""TEST INFRASTRUCTURE: float64 numpy references and the shared inputs of tests/test_metrics_small_gpu.py and
tests/test_preprocess_small_gpu.py (the metric and pre-processing kernels of csrc/metric_ops.hip at small, edge-case
shapes).  No torch, no device code.  tests/test_metric_small_ref_host.py checks the references against numpy / the
oracle and asserts the conditions the inputs must meet for the GPU tests' bounds to mean something (near-tie share,
resample margins and inside share, exact-integer ranges); the derivations of the bounds are in DESIGN.md section 8.2.
"""
import functools
import math

import numpy as np

U32 = 2.0 ** -24                                   # fp32 unit roundoff
T = 1024 * 256                                     # threads of the capped minmax / rescale / error grids
SIZES = (1, 2, 255, 256, 257, T - 1, T, T + 1, 2 * T + 77, 3 * T - 1)
STRIDE_SIZES = tuple(n for n in SIZES if n > T)

# ---------------------------------------------------------------------------------------------------------------------
# rescale (mpgan_rescale_minmax)
# ---------------------------------------------------------------------------------------------------------------------
RESCALE_TOL = 255.0 * 4 * U32                      # subtract, span, divide, multiply: four fp32 roundings of <= 255
NEAR_TIE_CAP = 1e-3


def rescale_ref(x, b_min=0.0, b_max=255.0):
    """The unrounded min/max rescale in float64; a constant input gives b_min (the kernel's span == 0 branch)."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = x.min(), x.max()
    if hi == lo:
        return np.full(x.shape, float(b_min))
    return np.clip((x - lo) / (hi - lo) * (b_max - b_min) + b_min, b_min, b_max)


def near_tie_mask(ref64, tol=RESCALE_TOL):
    """Elements whose unrounded value lies within tol of a half-integer: an fp32 evaluation may round them either way."""
    return np.abs(ref64 - (np.floor(ref64) + 0.5)) <= tol


def metric_blocks(n):
    return min((n + 255) // 256, 1024)


def last_block_elements(n):
    """(first, last) element that the highest-numbered block of the capped grid reads."""
    blocks = metric_blocks(n)
    first = (blocks - 1) * 256
    idx = np.arange(first, n)
    idx = idx[(idx // 256) % blocks == blocks - 1]
    return int(idx[0]), int(idx[-1])


def rescale_placements(n):
    """name -> (index of the global minimum, index of the global maximum)."""
    if n == 1:
        return {"single": (0, 0)}
    rng = np.random.RandomState(n % 9973)
    out = {"ends": (0, n - 1)}
    if n > 2:
        i, j = rng.choice(np.arange(1, n - 1), size=2, replace=n < 4)
        if n >= 4:
            out["interior"] = (int(i), int(j))
    if n > T:
        lb0, lb1 = last_block_elements(n)
        out["ends_swapped"] = (n - 1, 0)
        out["last_block_min"] = (lb0 + 17, int(j))
        out["last_block_max"] = (int(i), lb1)
    return out


RESCALE_CASES = tuple((n, p) for n in SIZES for p in rescale_placements(n))


@functools.lru_cache(maxsize=None)
def rescale_input(n, placement):
    """Uniform fp32 data in (-1, 1) whose only minimum (-1.5) and maximum (1.75) sit where the placement says."""
    rng = np.random.RandomState((n * 7 + len(placement)) % 99991)
    x = (rng.rand(n) * 2 - 1).astype(np.float32)
    imin, imax = rescale_placements(n)[placement]
    if n > 1:
        x[imax] = 1.75
        x[imin] = -1.5
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def integer_image(n, seed=0):
    """Integer-valued fp32 data in 0..255 that contains both 0 and 255 (n >= 2)."""
    rng = np.random.RandomState(1000 + seed + n % 9973)
    x = rng.randint(0, 256, size=n).astype(np.float32)
    i, j = rng.choice(n, size=2, replace=False)
    x[i], x[j] = 0.0, 255.0
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# image errors (mpgan_image_errors)
# ---------------------------------------------------------------------------------------------------------------------
def errors_ref(a, b, data_range):
    """(MAE, MSE, PSNR) in float64; PSNR is +inf for identical inputs."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    mae, mse = float(np.abs(d).mean()), float((d * d).mean())
    psnr = 10.0 * math.log10(float(data_range) ** 2 / mse) if mse > 0 else math.inf
    return mae, mse, psnr


def error_terms_per_thread(n):
    """m: how many elements one thread of err_partial_kernel adds in fp32."""
    return -(-n // (256 * metric_blocks(n)))


def error_rel_bound(n):
    """Relative bound of MAE / MSE against float64: m additions per thread, the product rounding, six shuffle levels,
    three wave additions and the fp32 store (all terms are non-negative, so the bound is relative to the sum)."""
    return (error_terms_per_thread(n) + 11) * U32


@functools.lru_cache(maxsize=None)
def errors_float_pair(n):
    rng = np.random.RandomState(2000 + n % 9973)
    a = (rng.rand(n) * 2 - 1).astype(np.float32)
    b = np.clip(a + 0.1 * rng.randn(n), -1, 1).astype(np.float32)
    b[0] = a[0] + np.float32(0.25)                   # never identical, also at n == 1
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def errors_int_pair(n):
    """Integer-valued images in 0..255 with |a - b| <= 64: every fp32 partial sum of the kernel is exact."""
    rng = np.random.RandomState(3000 + n % 9973)
    a = rng.randint(0, 256, size=n)
    b = np.clip(a + rng.randint(-64, 65, size=n), 0, 255)
    b[0] = a[0] + (1 if a[0] < 255 else -1)
    a, b = a.astype(np.float32), b.astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def f32_ulp(v):
    """Spacing of fp32 at |v| (v a float64 scalar or array), as float64."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# SSIM (mpgan_ssim)
# ---------------------------------------------------------------------------------------------------------------------
SSIM_TOL = 2.0 ** -23
SSIM_SHAPES_2D = ((7, 7), (7, 38), (7, 39), (14, 7), (15, 7), (14, 38), (15, 39), (8, 70), (23, 71))
SSIM_SHAPES_3D = ((7, 7, 7), (10, 7, 7), (11, 7, 7), (7, 14, 38), (11, 15, 39), (8, 8, 8), (13, 9, 40))
SSIM_SHAPES = SSIM_SHAPES_2D + SSIM_SHAPES_3D
SSIM_KINDS = ("pair", "equal_const", "diff_const", "one_const", "inverted", "unit_range")


def ssim_window(a, b, data_range, K1=0.01, K2=0.03):
    """SSIM of ONE 7x7 or 7x7x7 window in closed form (means, sample variances and covariance): no filter."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    assert a.size == b.size and a.size in (49, 343)
    ux, uy = a.mean(), b.mean()
    vx = ((a - ux) ** 2).sum() / (a.size - 1)
    vy = ((b - uy) ** 2).sum() / (a.size - 1)
    vxy = ((a - ux) * (b - uy)).sum() / (a.size - 1)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    return float((2 * ux * uy + c1) * (2 * vxy + c2) / ((ux * ux + uy * uy + c1) * (vx + vy + c2)))


def ssim_single_window(shape):
    return all(s == 7 for s in shape)


@functools.lru_cache(maxsize=None)
def ssim_pair(shape, kind):
    """(a, b, data_range) for one SSIM case, fp32, read-only."""
    rng = np.random.RandomState(31 + 7 * len(shape) + sum(shape))
    a = np.round(rng.rand(*shape) * 255)
    b = np.round(np.clip(a + 25 * rng.randn(*shape), 0, 255))
    data_range = 256.0
    if kind == "equal_const":
        a = np.full(shape, 93.0)
        b = a.copy()
    elif kind == "diff_const":
        a, b = np.full(shape, 93.0), np.full(shape, 201.0)
    elif kind == "one_const":
        b = np.full(shape, 100.0)
    elif kind == "inverted":
        b = 255.0 - a
    elif kind == "unit_range":
        a = rng.rand(*shape)
        b = np.clip(a + 0.1 * rng.randn(*shape), 0, 1)
        data_range = 1.0
    else:
        assert kind == "pair"
    a, b = a.astype(np.float32), b.astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, data_range


def ssim_want(a, b, data_range):
    """ssim_window for a single-window shape, else the oracle's restatement of skimage's algorithm."""
    from oracle.metrics_ref import structural_similarity
    if ssim_single_window(a.shape):
        return ssim_window(a, b, data_range)
    return structural_similarity(a, b, data_range=data_range)


# ---------------------------------------------------------------------------------------------------------------------
# percentiles (mpgan_percentiles)
# ---------------------------------------------------------------------------------------------------------------------
PCT_QS = ((0.0, 100.0), (1.0, 99.0), (50.0,), (12.5, 87.25))
PCT_SIZES = (1, 2, 3, 255, 256, 257, 2048 * 256 - 1, 2048 * 256, 2048 * 256 + 1)


def order_stat_percentile(x32, q):
    """np.percentile(x, q) with linear interpolation, restated on the sorted float32 data: returns
    (value, s[lo], s[hi], t) with r = q/100 (n-1), lo = floor(r), hi = min(lo+1, n-1), t = r - lo, and the value
    interpolated in float64 by numpy's two-sided rule.  Where t == 0 or s[lo] == s[hi] the value IS s[lo]: no
    arithmetic, so an infinite order statistic stays infinite (numpy's own lerp forms inf - inf there)."""
    x32 = np.asarray(x32)
    assert x32.dtype == np.float32
    s = np.sort(x32.ravel())
    n = s.size
    r = q / 100.0 * (n - 1)
    lo = min(int(math.floor(r)), n - 1)
    hi = min(lo + 1, n - 1)
    t = r - lo
    a, b = float(s[lo]), float(s[hi])
    if t == 0.0 or a == b:
        v = a
    elif t >= 0.5:
        v = b - (b - a) * (1.0 - t)
    else:
        v = a + (b - a) * t
    return v, s[lo], s[hi], t


def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def percentile_datasets():
    """name -> read-only fp32 array.  The radix select keys a float by its monotone uint32 image and fixes bits
    31..21, 20..10 and 9..0 in three passes."""
    rng = np.random.RandomState(77)
    fmax, tiny, fmin = np.finfo(np.float32).max, np.float32(1e-45), np.finfo(np.float32).tiny
    d = {}
    for sign, base in (("pos", 0x3F800000), ("neg", 0xBF800000)):
        # top 22 key bits shared, the low 10 differ: pass 2 alone decides (duplicates included)
        d["low10_" + sign] = _from_bits(base + rng.randint(0, 1024, size=1500))
        # every low-10 pattern exactly once: any two bins that pass 2 merges change a rank
        d["low10_all_" + sign] = _from_bits(base + rng.permutation(1024))
        # top 11 key bits shared, bits 20..10 differ, the low 10 are zero: pass 1 decides
        d["mid11_" + sign] = _from_bits(base + (rng.randint(0, 2048, size=3000) << 10))
        # ... and with random low bits under them: passes 1 and 2
        d["mid11_low10_" + sign] = _from_bits(base + (rng.randint(0, 2048, size=3000) << 10) + rng.randint(0, 1024, size=3000))
    specials = [-fmax, -1.0, -fmin, -tiny, -0.0, 0.0, tiny, fmin, 1.0, fmax]
    d["signs_small"] = np.array(specials + [-2 * tiny, 2 * tiny, -0.0], dtype=np.float32)[rng.permutation(13)]
    big = np.concatenate([np.array(specials + [np.inf] * 3 + [-np.inf] * 3), rng.randn(400) * 1e-3,
                          np.zeros(300), -np.zeros(300), rng.randn(200) * 1e30]).astype(np.float32)
    d["signs_inf"] = big[rng.permutation(big.size)]
    d["all_equal"] = np.full(1000, 3.25, dtype=np.float32)
    d["one_low"] = np.array([5.0] + [7.0] * 999, dtype=np.float32)[rng.permutation(1000)]
    d["one_high"] = np.array([7.0] + [5.0] * 999, dtype=np.float32)[rng.permutation(1000)]
    d["ramp_up"] = (np.arange(1000) * 0.37 - 150).astype(np.float32)
    d["ramp_down"] = d["ramp_up"][::-1].copy()
    for n in PCT_SIZES:
        d[f"n{n}"] = (np.random.RandomState(n % 9973).rand(n) * 2000 - 1000).astype(np.float32)
    for v in d.values():
        v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------------
# scale intensity range (mpgan_scale_intensity_range)
# ---------------------------------------------------------------------------------------------------------------------
SCALE_SIZES = (1000, 4096 * 256 - 1, 4096 * 256, 4096 * 256 + 513)


@functools.lru_cache(maxsize=None)
def scale_input(n):
    """MRI-like: 55 % background zeros, a skewed foreground."""
    rng = np.random.RandomState(5 + n % 9973)
    x = np.where(rng.rand(n) < 0.55, 0.0, rng.gamma(2.0, 250.0, size=n)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def degenerate_scale_input(fill):
    """More than 99 % of the voxels equal `fill`, so that the 1st and 99th percentile are both `fill`."""
    rng = np.random.RandomState(9)
    x = np.full(40000, fill, dtype=np.float32)
    idx = rng.choice(x.size, size=150, replace=False)
    x[idx] = (fill + rng.gamma(2.0, 250.0, size=150)).astype(np.float32)
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# resampling (mpgan_resample_to_identity_grid)
# ---------------------------------------------------------------------------------------------------------------------
def _rot(rz, ry, rx):
    cz, sz, cy, sy, cx, sx = math.cos(rz), math.sin(rz), math.cos(ry), math.sin(ry), math.cos(rx), math.sin(rx)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    Ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return Rz @ Ry @ Rx


def centred_origin(in_dhw, spacing, direction, out_size, extent_mm=256.0, shift=(0.0, 0.0, 0.0)):
    """The origin (x, y, z) that puts the centre of the input on the centre of the reference grid, plus `shift` mm."""
    size_in = np.array(in_dhw[::-1], dtype=np.float64)
    out_size = np.array(out_size, dtype=np.float64)
    centre = -out_size / 2.0 + (extent_mm / out_size) * (out_size - 1) / 2.0
    A = np.asarray(direction, dtype=np.float64).reshape(3, 3) @ np.diag(np.asarray(spacing, dtype=np.float64))
    return tuple(float(v) for v in centre + np.asarray(shift) - A @ ((size_in - 1) / 2.0))


def _geom(in_dhw, spacing, direction, out_size, shift=(3.1, -2.3, 1.7)):
    direction = np.asarray(direction, dtype=np.float64)
    return dict(in_dhw=tuple(in_dhw), spacing=tuple(spacing), direction=direction,
                origin=centred_origin(in_dhw, spacing, direction, out_size, shift=shift), out_size=tuple(out_size))


_R3 = _rot(0.5, -0.2, 0.3)
# name -> geometry; every one but "stride" must have an inside share in [0.2, 0.8]; all a margin >= 1e-6
RESAMPLE_GEOMS = {
    "identity": _geom((10, 12, 14), (13.7, 16.3, 18.9), np.eye(3), (32, 32, 32)),
    "flip_xy": _geom((10, 12, 14), (13.7, 16.3, 18.9), np.diag([-1.0, -1.0, 1.0]), (32, 32, 32)),
    "rotation": _geom((12, 11, 13), (14.3, 16.9, 15.1), _R3, (32, 32, 32)),
    "reflection": _geom((12, 11, 13), (14.3, 16.9, 15.1), _R3 @ np.diag([1.0, -1.0, 1.0]), (32, 32, 32)),
    "size1_x": _geom((11, 12, 1), (170.3, 17.9, 19.3), _R3, (32, 32, 32)),
    "size1_y": _geom((11, 1, 12), (18.7, 171.1, 19.3), _R3, (32, 32, 32)),
    "size1_z": _geom((1, 11, 12), (18.7, 17.9, 169.7), _R3, (32, 32, 32)),
    "noncubic": _geom((9, 13, 11), (17.3, 14.9, 21.1), _R3, (40, 24, 36)),
    "noncubic_flip": _geom((9, 13, 11), (17.3, 14.9, 21.1), np.diag([-1.0, -1.0, 1.0]), (24, 36, 20)),
    "stride": _geom((8, 12, 10), (19.3, 15.7, 22.9), _R3, (160, 128, 104), shift=(1.45, -1.12, -0.5)),
}
RESAMPLE_SHARE = (0.2, 0.8)
RESAMPLE_MARGIN = 1e-6


@functools.lru_cache(maxsize=None)
def resample_volume(name):
    rng = np.random.RandomState(21 + len(name))
    v = (1.0 + 99.0 * rng.rand(*RESAMPLE_GEOMS[name]["in_dhw"])).astype(np.float32)    # >= 1: 0 means "outside"
    v.setflags(write=False)
    return v


def resample_geometry_info(in_dhw, origin, spacing, direction, out_size, extent_mm=256.0):
    """(c, inside share, margin): the continuous input indices c[ix, iy, iz, :] of every output voxel as ITK defines
    them, the share of output voxels inside the input's half-voxel border, and the smallest distance of any component
    of c to -0.5 or to size - 0.5 (how far the closest inside / outside decision is from flipping)."""
    size_in = np.array(in_dhw[::-1], dtype=np.float64)
    out_size = np.array(out_size)
    origin_out, spacing_out = -out_size / 2.0, extent_mm / out_size
    A = np.asarray(direction, dtype=np.float64).reshape(3, 3) @ np.diag(np.asarray(spacing, dtype=np.float64))
    M = np.linalg.inv(A)
    grid = np.meshgrid(*[origin_out[d] + np.arange(out_size[d]) * spacing_out[d] for d in range(3)], indexing="ij")
    c = (np.stack(grid, axis=-1) - np.asarray(origin, dtype=np.float64)) @ M.T
    inside = np.all((c >= -0.5) & (c < size_in - 0.5), axis=-1)
    margin = min(float(np.abs(c + 0.5).min()), float(np.abs(c - (size_in - 0.5)).min()))
    return c, float(inside.mean()), margin


# identity direction, 8^3 input with spacing 4 and origin -14 onto 32^3: c = 2 i - 0.5 exactly on every axis
BORDER_CASE = dict(in_dhw=(8, 8, 8), spacing=(4.0, 4.0, 4.0), direction=np.eye(3), origin=(-14.0, -14.0, -14.0),
                   out_size=(32, 32, 32))
