"""Intensity pre-processing on the device: the array half of SURVEY.md section 8(f) row N3.

`ScaleIntensityRangePercentilesd(keys, lower=1, upper=99, b_min=-1, b_max=1, clip=True)` is the last
transform before the training path (code/GAN/GAN_final.py:386-394; MONAI 0.4.0:
`a_min, a_max = np.percentile(img, lower), np.percentile(img, upper)` then `ScaleIntensityRange`).
`resample_to_identity_grid` is the array half of the transform before it, `ResampleT1T2d`
(code/GAN/transforms.py:79-213): linear interpolation onto the 256 mm identity-direction grid.  Reading the
NIfTI files themselves (ITK) stays out of scope.

`otsu_threshold`, `foreground_mask`, `foreground_bbox` and `crop_foreground` make the foreground mask that the
reference's scoring scripts import MONAI's `CropForegroundd` / `ThresholdIntensityd` for and never call
(code/GAN/minipig_inference.py:28,43): Otsu's threshold from a histogram on the device, `x > threshold`, and MONAI's
`generate_spatial_bounding_box`.  Neither MONAI nor skimage is installed here: the definitions in include/mpgan_hip.h
are what is pinned, against tests/foreground_ref.py.
"""
from __future__ import annotations

import ctypes as C
import numbers
from typing import Sequence

import torch

from . import ops
from ._lib import check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def percentiles(x: torch.Tensor, q: Sequence[float]) -> torch.Tensor:
    """np.percentile(x, q) (linear interpolation) for one or two percentiles; returns a device tensor."""
    q = [float(v) for v in q]
    if not 1 <= len(q) <= 2:
        raise ValueError("percentiles: one or two percentiles per call")
    x = x.contiguous().float()
    need = int(lib().mpgan_percentile_workspace())
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=x.device)
    out = torch.empty(len(q), device=x.device)
    qh = (C.c_double * len(q))(*q)
    check(lib().mpgan_percentiles(x.data_ptr(), x.numel(), qh, len(q), ws.data_ptr(), ws.numel() * 8, out.data_ptr(),
                                  _stream()), "percentiles")
    return out


def scale_intensity_range_percentiles(x: torch.Tensor, lower: float = 1.0, upper: float = 99.0, b_min: float = -1.0,
                                      b_max: float = 1.0, clip: bool = True) -> torch.Tensor:
    """MONAI 0.4.0 ScaleIntensityRangePercentiles(lower, upper, b_min, b_max, clip, relative=False) on
    one image/volume (any shape: the percentiles are taken over all of its elements)."""
    x = x.contiguous().float()
    mm = percentiles(x, (lower, upper))
    y = torch.empty_like(x)
    check(lib().mpgan_scale_intensity_range(x.data_ptr(), x.numel(), mm.data_ptr(), float(b_min), float(b_max),
                                            int(clip), y.data_ptr(), _stream()), "scale_intensity_range")
    return y


def resample_to_identity_grid(vol: torch.Tensor, origin, spacing, direction, output_size=(128, 128, 128),
                              extent_mm: float = 256.0) -> torch.Tensor:
    """`ResampleT1T2d` (code/GAN/transforms.py:79-213) for one volume: `vol` is the (D,H,W) array of an ITK image
    with `origin` / `spacing` in ITK's (x,y,z) order and a 3x3 `direction`; returns the (D,H,W) = reversed
    `output_size` (x,y,z) resampled array on the reference grid origin = -size/2, spacing = extent_mm/size,
    identity direction (identity transform, linear interpolation, 0 outside the input)."""
    if vol.dim() != 3:
        raise ValueError("resample_to_identity_grid: expected a (D,H,W) volume")
    vol = vol.contiguous().float()
    out_dhw = tuple(int(v) for v in reversed(tuple(output_size)))
    out = torch.empty(out_dhw, device=vol.device)
    i3 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])
    d3 = lambda v: (C.c_double * len(v))(*[float(x) for x in v])
    dirs = [float(x) for row in direction for x in row] if len(direction) == 3 else [float(x) for x in direction]
    check(lib().mpgan_resample_to_identity_grid(vol.data_ptr(), i3(vol.shape), d3(origin), d3(spacing), d3(dirs),
                                                i3(out_dhw), float(extent_mm), out.data_ptr(), _stream()),
          "resample_to_identity_grid")
    return out


# ---- foreground masks (csrc/foreground.hip) ----
OTSU_MAX_BINS = 256


def _fg_items(x: torch.Tensor, who: str):
    """x as a contiguous (B, C, *spatial) tensor, and whether it came unbatched ((H, W) or (D, H, W))."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"{who}: expects an fp32 device tensor")
    if x.dim() not in (2, 3, 4, 5) or 0 in x.shape:
        raise ValueError(f"{who}: expects a non-empty (B, C, H, W), (B, C, D, H, W), (H, W) or (D, H, W) tensor, got "
                         f"{tuple(x.shape)}")
    unbatched = x.dim() in (2, 3)
    return (x[None, None] if unbatched else x).contiguous(), unbatched     # a contiguous view keeps its offset


def _otsu_config(bins, value_range, who):
    if int(bins) != bins or not 2 <= int(bins) <= OTSU_MAX_BINS:
        raise ValueError(f"{who}: bins must be an integer in [2, {OTSU_MAX_BINS}], got {bins!r}")
    try:
        lo, hi = (float(v) for v in value_range)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: value_range must be one (lo, hi) pair, got {value_range!r}") from None
    if not hi > lo or hi - lo == float("inf"):
        raise ValueError(f"{who}: value_range needs finite hi > lo, got {value_range!r}")
    return int(bins), lo, hi


def check_threshold(threshold, who: str):
    """The complaint about a threshold that is none of "otsu", a finite number and a tensor; before any launch."""
    if isinstance(threshold, torch.Tensor) or threshold == "otsu":
        return
    if isinstance(threshold, (str, bool)) or not isinstance(threshold, numbers.Real):
        raise ValueError(f'{who}: threshold must be "otsu", a finite number or a per-item device tensor, got '
                         f"{threshold!r}")
    if threshold != threshold or threshold in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: threshold must be finite, got {threshold!r}")


def mask_bytes(mask, like: torch.Tensor, who: str, broadcast_channels: bool = False) -> torch.Tensor:
    """The mask argument of every masked statistic as contiguous uint8 in like's shape: a bool / uint8 tensor on like's
    device with like's shape, or (broadcast_channels, the losses' (B, C, *spatial) tensors) with channel extent 1."""
    shape = tuple(like.shape)
    shapes = (shape, shape[:1] + (1,) + shape[2:]) if broadcast_channels else (shape,)
    if (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != like.device
            or tuple(mask.shape) not in shapes):
        got = f"{tuple(mask.shape)} {mask.dtype} on {mask.device}" if isinstance(mask, torch.Tensor) else repr(type(mask))
        raise ValueError(f"{who}: mask must be a same-shape bool / uint8 tensor on the inputs' device, shape {shape}"
                         + (" or with channel extent 1" if broadcast_channels else "") + f", got {got}")
    mask = mask.expand(shape).contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def item_thresholds(x: torch.Tensor, threshold, bins, value_range, who: str) -> torch.Tensor:
    """The fp32 device tensor of one threshold per (b, c) item of the contiguous (B, C, *spatial) tensor x."""
    check_threshold(threshold, who)
    items = x.shape[0] * x.shape[1]
    if isinstance(threshold, torch.Tensor):
        if threshold.dtype != torch.float32 or threshold.device != x.device or threshold.numel() not in (1, items):
            raise ValueError(f"{who}: a threshold tensor must be fp32, on x's device and hold one value or one per "
                             f"(batch, channel) item ({items}), got {tuple(threshold.shape)} {threshold.dtype}")
        return threshold.detach().reshape(-1).expand(items).contiguous()
    if threshold == "otsu":
        bins, lo, hi = _otsu_config(bins, value_range, who)
        return ops.otsu_threshold(x, items, lo, hi, bins, torch.empty(items, device=x.device))
    return torch.full((items,), float(threshold), device=x.device)


def otsu_threshold(x: torch.Tensor, bins: int = 256, value_range=(-1.0, 1.0)) -> torch.Tensor:
    """Otsu's threshold of every (b, c) image of a (B, C, H, W) or (B, C, D, H, W) fp32 device tensor, as a (B, C)
    device tensor; an unbatched (H, W) or (D, H, W) tensor gives a 0-d tensor.  The histogram has `bins` (2..256)
    equal-width bins over value_range = (lo, hi), binned by joint_histogram's rule (values outside the range and NaN
    are dropped); the threshold is the centre of the first bin that maximises the between-class variance, as
    skimage.filters.threshold_otsu forms it.  No value inside the range gives NaN; one occupied bin gives its centre.
    No host sync."""
    who = "otsu_threshold"
    bins, lo, hi = _otsu_config(bins, value_range, who)
    x, unbatched = _fg_items(x, who)
    thr = ops.otsu_threshold(x, x.shape[0] * x.shape[1], lo, hi, bins,
                             torch.empty(x.shape[:2], device=x.device))
    return thr[0, 0] if unbatched else thr


def foreground_mask(x: torch.Tensor, threshold="otsu", bins: int = 256, value_range=(-1.0, 1.0)) -> torch.Tensor:
    """The uint8 mask x > threshold in x's shape (strict, in fp32; NaN is background).  threshold: "otsu" (per item,
    from otsu_threshold(x, bins, value_range)), a number, or an fp32 device tensor with one value per (b, c) item.
    The result goes into joint_histogram / mutual_information / image_errors as their explicit mask as it is."""
    who = "foreground_mask"
    xc, _ = _fg_items(x, who)
    thr = item_thresholds(xc, threshold, bins, value_range, who)
    mask = torch.empty(xc.shape, dtype=torch.uint8, device=xc.device)
    ops.foreground_mask(xc, xc.shape[2:], thr.numel(), thr, mask=mask)
    return mask.reshape(x.shape)


def _margin3(margin, nd, who):
    m = list(margin) if isinstance(margin, (tuple, list)) else [margin] * nd
    if len(m) != nd or any(not isinstance(v, numbers.Real) or int(v) != v or v < 0 for v in m):
        raise ValueError(f"{who}: margin must be a non-negative integer or one per spatial axis ({nd}), got {margin!r}")
    return (0,) * (3 - nd) + tuple(int(v) for v in m)


def foreground_bbox(x: torch.Tensor, threshold="otsu", margin=0, bins: int = 256,
                    value_range=(-1.0, 1.0)) -> torch.Tensor:
    """MONAI's generate_spatial_bounding_box of x > threshold per (b, c) image: a device int32 tensor (B, C, 2, nd),
    [..., 0, :] the start and [..., 1, :] the exclusive end over the nd spatial axes, start = max(min - margin, 0) and
    end = min(max + 1 + margin, extent); an image without foreground gives start = end = 0.  (2, nd) for an unbatched
    tensor.  No host sync."""
    who = "foreground_bbox"
    xc, unbatched = _fg_items(x, who)
    nd = xc.dim() - 2
    margin3 = _margin3(margin, nd, who)
    thr = item_thresholds(xc, threshold, bins, value_range, who)
    box = torch.empty(xc.shape[:2] + (2, 3), dtype=torch.int32, device=xc.device)
    ops.foreground_mask(xc, xc.shape[2:], thr.numel(), thr, margin3, box=box)
    box = box[..., 3 - nd:]
    return box[0, 0] if unbatched else box


def foreground_count(x: torch.Tensor, threshold="otsu", bins: int = 256, value_range=(-1.0, 1.0)) -> torch.Tensor:
    """The number of voxels with x > threshold per (b, c) image: a device int64 tensor (B, C), 0-d for an unbatched
    tensor.  No host sync."""
    who = "foreground_count"
    xc, unbatched = _fg_items(x, who)
    thr = item_thresholds(xc, threshold, bins, value_range, who)
    count = torch.empty(xc.shape[:2], dtype=torch.int64, device=xc.device)
    ops.foreground_mask(xc, xc.shape[2:], thr.numel(), thr, count=count)
    return count[0, 0] if unbatched else count


def crop_foreground(x: torch.Tensor, source: torch.Tensor = None, threshold="otsu", margin=0, bins: int = 256,
                    value_range=(-1.0, 1.0)):
    """MONAI's CropForegroundd for ONE sample: crops x ((1, C, *spatial) or unbatched) to the foreground box of
    `source` (default: x itself; same spatial extents; with several channels the union of their boxes).  Returns
    (crop, start, end), start and end being tuples of ints like CropForegroundd's foreground_start_coord /
    foreground_end_coord.  THIS FUNCTION READS THE BOX TO THE HOST (one synchronising copy of 2 * nd integers per
    channel): the crop's shape depends on the data.  Everything else in this module stays on the device.  No
    foreground gives start = end = 0 and an empty crop."""
    who = "crop_foreground"
    source = x if source is None else source
    xc, unbatched = _fg_items(x, who)
    sc, _ = _fg_items(source, who)
    if xc.shape[0] != 1 or sc.shape[0] != 1:
        raise ValueError(f"{who}: handles one sample (B == 1 or unbatched), got x {tuple(x.shape)} and source "
                         f"{tuple(source.shape)}")
    if sc.shape[2:] != xc.shape[2:]:
        raise ValueError(f"{who}: source's spatial extents {tuple(sc.shape[2:])} differ from x's {tuple(xc.shape[2:])}")
    box = foreground_bbox(sc, threshold, margin, bins, value_range)[0].cpu()          # (C, 2, nd): the host read
    filled = box[(box[:, 1] > box[:, 0]).all(dim=1)]
    if filled.shape[0] == 0:
        start = end = (0,) * box.shape[-1]
    else:
        start = tuple(int(v) for v in filled[:, 0].min(dim=0).values)
        end = tuple(int(v) for v in filled[:, 1].max(dim=0).values)
    crop = xc[(slice(None), slice(None)) + tuple(slice(s, e) for s, e in zip(start, end))]
    return (crop[0, 0] if unbatched else crop), start, end
