"""On-device evaluation metrics of the reference's offline scripts (SURVEY.md section 8(f)
row N2): 0..255 rescale + round as code/GAN/inferrence.py:188-204 applies it, then MAE / MSE /
PSNR and SSIM (data_range 256, code/GAN/psnr_ssim_metric.py:88-106; code/GAN/metrics.py:213-223).
SSIM restates skimage.metrics.structural_similarity's published algorithm (skimage itself is not in
this image: parity is pinned on a scipy.ndimage restatement in oracle/metrics_ref.py only).
joint_histogram / mutual_information add the third stored figure of SURVEY.md section 6 (the estimator behind the
reference's stored MUTINF numbers is unknown: the definition here is pinned against numpy, not against them)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple, Union

import torch

from . import ops
from ._lib import check, lib
from .preprocess import mask_bytes


def _stream():
    return torch.cuda.current_stream().cuda_stream


def rescale_0_255(x: torch.Tensor, do_round: bool = True) -> torch.Tensor:
    """ScaleIntensityRangePercentiles(lower=0, upper=100, b_min=0, b_max=255, clip=True) + round."""
    x = x.contiguous()
    part = torch.empty(int(lib().mpgan_metric_partials()), device=x.device)
    mm = torch.empty(2, device=x.device)
    y = torch.empty_like(x)
    check(lib().mpgan_rescale_minmax(x.data_ptr(), x.numel(), 0.0, 255.0, int(do_round), part.data_ptr(),
                                     mm.data_ptr(), y.data_ptr(), _stream()), "rescale_minmax")
    return y


def _masked_image_errors(a, b, data_range, mask):
    if a.dtype != torch.float32 or b.dtype != torch.float32 or not (a.is_cuda and b.is_cuda):
        raise ValueError("image_errors: a mask needs two fp32 device tensors")
    mask = mask_bytes(mask, a, "image_errors")
    if a.numel() == 0:
        raise ValueError("image_errors: empty tensors")
    out = ops.masked_image_errors(a.contiguous(), b.contiguous(), mask, data_range,
                                  torch.empty(4, dtype=torch.float64, device=a.device))
    return {"mae": out[0], "mse": out[1], "psnr": out[2], "count": out[3]}


def image_errors(a: torch.Tensor, b: torch.Tensor, data_range: float = 256.0,
                 mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """MAE, MSE and PSNR between two same-shape device tensors (scalars stay on the device).  With mask (a same-shape
    bool / uint8 device tensor, e.g. preprocess.foreground_mask's output) the three are taken over the voxels whose
    mask is non-zero, in float64, and "count" is their number; an empty mask gives NaN and count 0."""
    if a.shape != b.shape:
        raise ValueError("image_errors: shape mismatch")
    if mask is not None:
        return _masked_image_errors(a, b, data_range, mask)
    a, b = a.contiguous(), b.contiguous()
    part = torch.empty(int(lib().mpgan_metric_partials()), device=a.device)
    out = torch.empty(3, device=a.device)
    check(lib().mpgan_image_errors(a.data_ptr(), b.data_ptr(), a.numel(), float(data_range), part.data_ptr(),
                                   out.data_ptr(), _stream()), "image_errors")
    return {"mae": out[0], "mse": out[1], "psnr": out[2]}


def score_volume(generated: torch.Tensor, ground_truth: torch.Tensor,
                 mutual_information: bool = False, mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The inference script's scoring: both volumes rescaled to 0..255 and rounded, then compared
    (MAE / MSE / PSNR; plus SSIM when the tensors are (H, W) or (D, H, W)).  mutual_information=True
    adds "mi" and "nmi" of the two rescaled volumes (256 bins over [0, 256], nats).  mask (a same-shape bool / uint8
    device tensor, e.g. preprocess.foreground_mask(ground_truth)) restricts MAE / MSE / PSNR to its voxels and adds
    "count", and wherever "ssim" is returned also "ssim_masked": the SSIM over the windows whose centre voxel is in
    the mask (ssim(mask=), float64; NaN without such a window).  The rescaling, "ssim" itself, "mi" and "nmi" stay
    whole-volume figures."""
    g, t = rescale_0_255(generated), rescale_0_255(ground_truth)
    out = image_errors(g, t, 256.0, mask)
    if g.dim() in (2, 3) and min(g.shape[-2:]) >= 7 and (g.dim() == 2 or g.shape[0] >= 7):
        out["ssim"] = ssim(g, t, 256.0)
        if mask is not None:
            out["ssim_masked"] = ssim(g, t, 256.0, mask)
    if mutual_information:
        m = _mutual_information(g, t, bins=256, value_range=(0.0, 256.0))
        out["mi"], out["nmi"] = m["mi"], m["nmi"]
    return out


def _ssim_inputs(who, a, b):
    """The two images of ssim / ssim_map as contiguous fp32, and their extents."""
    if a.shape != b.shape or a.dim() not in (2, 3):
        raise ValueError(f"{who}: expects two same-shape (H, W) or (D, H, W) tensors")
    if not (a.is_cuda and b.is_cuda):
        raise ValueError(f"{who}: expects two device tensors")
    return a.contiguous().float(), b.contiguous().float(), tuple(a.shape)


def _weighted_ssim(who, a, b, data_range, mask, want_map):
    """(stats, smap) of one image through the masked SSIM forward (include/mpgan_hip.h, lo = 0): stats =
    (ssim_item, n_item) in float64, smap the fp32 map of S over the window corners when want_map."""
    a, b, spatial = _ssim_inputs(who, a, b)
    if not float(data_range) > 0:
        raise ValueError(f"{who}: data_range must be positive, got {data_range!r}")
    if mask is not None:
        mask = mask_bytes(mask, a, who)
    dev = a.device
    ws_bytes, _ = ops.ssim_loss_workspace(spatial, 1, 0, weighted=True)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    stats = torch.empty((1, 2), dtype=torch.float64, device=dev)
    corners = tuple(1 if len(spatial) == 3 and i == 0 and s == 1 else s - 6 for i, s in enumerate(spatial))
    smap = torch.empty(corners, device=dev) if want_map else None          # a depth of 1 is a slice: not windowed
    ops.ssim_loss_forward(a, b, spatial, 1, 1, 0.0, float(data_range), 0, ws, None, "mean", torch.empty((), device=dev),
                          mask=mask, stats=stats, smap=smap)
    return stats, smap


def ssim_map(a: torch.Tensor, b: torch.Tensor, data_range: float = 256.0) -> torch.Tensor:
    """The per-window SSIM S of two (H, W) slices or (D, H, W) volumes, as ssim() defines it: an fp32 device tensor of
    shape (H - 6, W - 6) or (D - 6, H - 6, W - 6), entry k the window whose corner is k and whose centre is k + 3
    (skimage's full=True map cropped by its 3-sample border).  Its mean is ssim(a, b); its mean over mask[3:-3, ...]
    is ssim(a, b, mask=mask).  One pass of the SSIM loss's forward kernel."""
    return _weighted_ssim("ssim_map", a, b, data_range, None, True)[1]


def ssim(a: torch.Tensor, b: torch.Tensor, data_range: float = 256.0, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """structural_similarity(a, b, data_range=256) of two (H, W) slices or (D, H, W) volumes
    (code/GAN/psnr_ssim_metric.py:91-92): 7-wide uniform window, K1 = 0.01, K2 = 0.03, sample
    covariance, mean over the interior.  Returns a device scalar.  With mask (a same-shape bool / uint8 device tensor,
    e.g. preprocess.foreground_mask's output) the mean runs over the windows whose centre voxel is in the mask --
    the interior of the map averaged over the mask -- and comes back as a float64 device scalar; a mask without such
    a window gives NaN.  Either way one pass of the SSIM loss's forward kernel (csrc/ssim_loss.hip)."""
    if mask is not None:
        return _weighted_ssim("ssim", a, b, data_range, mask, False)[0][0, 0]
    a, b, spatial = _ssim_inputs("ssim", a, b)
    dhw = (C.c_int32 * 3)(*((1,) * (3 - len(spatial)) + spatial))
    need = int(lib().mpgan_ssim_workspace(dhw))
    if need < 0:
        raise ValueError(f"ssim: extents {spatial} are below the 7-wide window")
    ws = torch.empty(max(need // 8, 1), dtype=torch.float64, device=a.device)
    out = torch.empty(1, device=a.device)
    check(lib().mpgan_ssim(a.data_ptr(), b.data_ptr(), dhw, float(data_range), ws.data_ptr(), ws.numel() * 8,
                           out.data_ptr(), _stream()), "ssim")
    return out[0]


_MASK_MODES = {None: 0, "both_nonzero": 1, "either_nonzero": 2}
_MI_KEYS = ("mi", "h_a", "h_b", "h_ab", "nmi", "count")
ValueRange = Union[Tuple[float, float], Tuple[Tuple[float, float], Tuple[float, float]]]


def _ranges(value_range: ValueRange) -> Tuple[float, float, float, float]:
    if len(value_range) != 2:
        raise ValueError("value_range: (lo, hi) or ((lo_a, hi_a), (lo_b, hi_b))")
    if isinstance(value_range[0], (tuple, list)):
        (lo_a, hi_a), (lo_b, hi_b) = value_range
    else:
        lo_a, hi_a = value_range
        lo_b, hi_b = value_range
    return float(lo_a), float(hi_a), float(lo_b), float(hi_b)


def joint_histogram(a: torch.Tensor, b: torch.Tensor, bins: int = 256, value_range: ValueRange = (0.0, 256.0),
                    mask: Union[None, str, torch.Tensor] = None, batched: bool = False) -> torch.Tensor:
    """Joint histogram of two same-shape fp32 device tensors: int64 (bins, bins), rows indexed by a's bin and
    columns by b's, or (B, bins, bins) with batched=True (dim 0 is the batch).  The bin of a value v over
    [lo, hi] is min(floor((v - lo) * (bins / (hi - lo))), bins - 1) in fp32, so v == hi falls into the last
    bin; voxels with a value outside its range or NaN are dropped.  value_range is (lo, hi) for both images or
    ((lo_a, hi_a), (lo_b, hi_b)).  mask: None, "both_nonzero", "either_nonzero", or a same-shape bool / uint8
    tensor (non-zero keeps the voxel).  Counts are exact; the result stays on the device."""
    if a.shape != b.shape:
        raise ValueError("joint_histogram: shape mismatch")
    if a.dtype != torch.float32 or b.dtype != torch.float32 or not (a.is_cuda and b.is_cuda):
        raise ValueError("joint_histogram: expects two fp32 device tensors")
    if batched and a.dim() < 1:
        raise ValueError("joint_histogram: batched=True needs a batch dimension")
    lo_a, hi_a, lo_b, hi_b = _ranges(value_range)
    a, b = a.contiguous(), b.contiguous()          # a contiguous view keeps its (possibly unaligned) offset
    mask_ptr = None
    if isinstance(mask, torch.Tensor):
        mask = mask_bytes(mask, a, "joint_histogram")
        mode, mask_ptr = 3, mask.data_ptr()
    elif mask in _MASK_MODES:
        mode = _MASK_MODES[mask]
    else:
        raise ValueError(f"joint_histogram: unknown mask {mask!r}")
    batch = a.shape[0] if batched else 1
    if batch < 1:
        raise ValueError("joint_histogram: empty batch")
    per_item = a.numel() // batch
    hist = torch.empty((batch, int(bins), int(bins)), dtype=torch.int64, device=a.device)
    check(lib().mpgan_joint_histogram(a.data_ptr() if per_item else None, b.data_ptr() if per_item else None, mask_ptr,
                                      mode, per_item, batch, lo_a, hi_a, lo_b, hi_b, int(bins), hist.data_ptr(),
                                      _stream()), "joint_histogram")
    return hist if batched else hist[0]


def mutual_information_from_histogram(hist: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The figures of mutual_information() from an int64 (bins, bins) or (B, bins, bins) joint histogram."""
    if hist.dtype != torch.int64 or hist.dim() not in (2, 3) or hist.shape[-1] != hist.shape[-2] or not hist.is_cuda:
        raise ValueError("mutual_information_from_histogram: expects an int64 (bins, bins) or (B, bins, bins) device tensor")
    batched = hist.dim() == 3
    hist = hist.contiguous()
    batch = hist.shape[0] if batched else 1
    out = torch.empty((batch, 6), dtype=torch.float64, device=hist.device)
    check(lib().mpgan_mutual_information(hist.data_ptr(), batch, hist.shape[-1], out.data_ptr(), _stream()),
          "mutual_information")
    return {k: (out[:, i] if batched else out[0, i]) for i, k in enumerate(_MI_KEYS)}


def mutual_information(a: torch.Tensor, b: torch.Tensor, bins: int = 256, value_range: ValueRange = (0.0, 256.0),
                       mask: Union[None, str, torch.Tensor] = None, batched: bool = False) -> Dict[str, torch.Tensor]:
    """Mutual information of two same-shape fp32 device tensors from their joint_histogram (same arguments):
    {"mi", "h_a", "h_b", "h_ab", "nmi", "count"} as float64 device scalars, or (B,) tensors with batched=True.
    Entropies H = log N - (sum c log c) / N over the exact integer counts; mi = h_a + h_b - h_ab;
    nmi = (h_a + h_b) / h_ab (Studholme); count = N, the number of admitted voxels.  Values are in nats: divide
    by ln 2 for bits.  No admitted voxel gives NaN (count 0); all voxels in one bin give mi = 0 and nmi = 1."""
    return mutual_information_from_histogram(joint_histogram(a, b, bins, value_range, mask, batched))


_mutual_information = mutual_information        # score_volume's keyword argument shadows the name there
