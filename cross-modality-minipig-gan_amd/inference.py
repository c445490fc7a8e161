"""Sliding-window inference: a 128^3-trained generator over volumes larger than its training window.

Both of the reference's inference scripts import MONAI's sliding-window inferer (code/GAN/inferrence.py:18,
code/GAN/minipig_inference.py:17) and minipig_inference.py:110-114 holds the call, commented out, with
`roi_size = (128, 128, 128)` and `sw_batch_size = 12`.  This module provides that call on the device:
`sliding_window_inference` and `SlidingWindowInferer` with MONAI 0.4.0's signatures and semantics.

The semantics restate MONAI 0.4.0 `monai/inferers/utils.py` (sliding_window_inference, _get_scan_interval) and
`monai/data/utils.py` (dense_patch_slices, compute_importance_map, gaussian_1d) from their public source.  MONAI
is not a dependency of this package, so the restatement could not be run against MONAI itself; like SURVEY.md
Appendix A it is a reading of the source, pinned by the CPU restatement in tests/test_sliding_window.py.

- roi entries <= 0 or None fall back to the image extent of that dim;
- each spatial dim is padded with `cval` to at least the roi: diff // 2 before, the rest after;
- scan interval = roi when roi equals the padded extent, else int(roi * (1 - overlap)) (1 when that is 0);
- per dim the window starts are d * interval for d = 0 .. the first d whose window reaches the end, the last
  one pulled back flush with the end; windows are their meshgrid("ij") product (first spatial dim slowest) and
  are enumerated image-major across the batch, sw_batch_size consecutive windows per predictor call;
- importance map: ones ("constant"), or ("gaussian") a unit impulse at roi // 2 through a separable Gaussian
  (sigma = roi * sigma_scale, truncated at 4 sigma, zero padding), divided by its maximum, zeros replaced by the
  smallest non-zero value;
- out[b, :, win] += imp * pred and count[b, :, win] += imp window by window, then out / count, cropped.

Only the predictor computes.  Gathering the windows (with the padding done on the fly), the count map, the
blend and the division are HIP kernels (csrc/window_ops.hip); every output element is owned by one thread that
visits the windows in the order above, with one rounded product and one rounded add per window, so the result
is bit-identical to the sequential restatement.  Only constant padding is supported: `padding_mode` "reflect" or
"replicate" raises NotImplementedError.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import torch

from ._lib import SwGeomC, check, lib

_MODES = ("constant", "gaussian")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@dataclass(frozen=True)
class WindowPlan:
    """Window geometry of one image extent (spatial dims only, in the caller's dimensionality)."""
    image_size: Tuple[int, ...]
    roi: Tuple[int, ...]
    pad_lo: Tuple[int, ...]
    padded: Tuple[int, ...]
    interval: Tuple[int, ...]
    starts: Tuple[Tuple[int, ...], ...]     # per dim, in padded coordinates

    @property
    def num_windows(self) -> int:
        return math.prod(len(s) for s in self.starts)

    def windows(self):
        """Start tuples of every window in MONAI's order (meshgrid "ij": first dim slowest)."""
        out = [()]
        for s in self.starts:
            out = [w + (v,) for w in out for v in s]
        return out


def _mode_name(mode) -> str:
    name = getattr(mode, "value", mode)          # monai.utils.BlendMode members carry their string as .value
    if not isinstance(name, str) or name not in _MODES:
        raise ValueError(f"mode must be one of {_MODES}, got {mode!r}")
    return name


def plan_windows(image_size: Sequence[int], roi_size, overlap: float) -> WindowPlan:
    """Padding, scan interval and per-dim window starts for an image of `image_size` (MONAI 0.4.0:
    fall_back_tuple, _get_scan_interval, dense_patch_slices)."""
    image_size = tuple(int(v) for v in image_size)
    nsd = len(image_size)
    if not 0.0 <= float(overlap) < 1.0:
        raise ValueError(f"overlap must be >= 0 and < 1, got {overlap!r}")
    if roi_size is None or isinstance(roi_size, (int, float)):
        roi_size = (roi_size,) * nsd
    roi_size = tuple(roi_size)
    if len(roi_size) != nsd:
        raise ValueError(f"roi_size has {len(roi_size)} dims, the input has {nsd} spatial dims")
    roi = tuple(s if r is None or int(r) <= 0 else int(r) for r, s in zip(roi_size, image_size))
    pad_lo, padded, interval, starts = [], [], [], []
    for r, s in zip(roi, image_size):
        diff = max(r - s, 0)
        pad_lo.append(diff // 2)
        size = max(s, r)
        padded.append(size)
        step = r if r == size else (int(r * (1 - overlap)) or 1)
        interval.append(step)
        num = int(math.ceil(float(size) / step))
        scan = next((d for d in range(num) if d * step + r >= size), None)
        scan = 1 if scan is None else scan + 1
        starts.append(tuple(d * step - max(d * step + r - size, 0) for d in range(scan)))
    return WindowPlan(image_size, roi, tuple(pad_lo), tuple(padded), tuple(interval), tuple(starts))


def gaussian_vectors(roi: Sequence[int], sigma_scale: float):
    """Per dim, the fp32 Gaussian (MONAI 0.4.0 gaussian_1d: sigma = roi * sigma_scale, tail int(4 sigma + 0.5),
    normalised to sum 1) that a unit impulse at roi // 2 becomes, over the roi's positions (0 beyond the tail)."""
    out = []
    for r in roi:
        sigma = r * float(sigma_scale)
        if sigma <= 0:
            raise ValueError(f"sigma_scale must be positive, got {sigma_scale!r}")
        tail = int(sigma * 4.0 + 0.5)
        x = torch.arange(-tail, tail + 1, dtype=torch.float32)
        k = torch.exp(-0.5 / (sigma * sigma) * x ** 2)
        k = k / k.sum()
        v = torch.zeros(r, dtype=torch.float32)
        c = r // 2
        lo, hi = max(0, c - tail), min(r, c + tail + 1)
        v[lo:hi] = k[lo - c + tail:hi - c + tail]
        out.append(v)
    return out


def importance_map(roi: Sequence[int], mode="constant", sigma_scale: float = 0.125) -> torch.Tensor:
    """MONAI 0.4.0 compute_importance_map on the host (fp32, CPU)."""
    roi = tuple(int(r) for r in roi)
    if _mode_name(mode) == "constant":
        return torch.ones(roi, dtype=torch.float32)
    vs = gaussian_vectors(roi, sigma_scale)
    # the separable filter applied to an impulse: every output value is one rounded product per filtered dim,
    # in the filter's dim order (the other taps multiply zeros)
    m = vs[0].reshape((-1,) + (1,) * (len(roi) - 1))
    for d in range(1, len(roi)):
        m = m * vs[d].reshape((1,) * d + (-1,) + (1,) * (len(roi) - 1 - d))
    m = m / m.max()
    nz = m[m != 0]
    m[m == 0] = nz.min()
    return m


_IMP_CACHE = {}


def _device_importance(roi, mode: str, sigma_scale: float, device) -> Optional[torch.Tensor]:
    """Device copy of the importance map, built once per (roi, sigma_scale, mode, device); None for "constant"
    (the kernels take a flag instead of a map of ones)."""
    if mode == "constant":
        return None
    key = (tuple(roi), float(sigma_scale), mode, device)
    m = _IMP_CACHE.get(key)
    if m is None:
        m = importance_map(roi, mode, sigma_scale).to(device).contiguous()
        _IMP_CACHE[key] = m
    return m


def _geometry(plan: WindowPlan, batch: int, device):
    """mpgan_sw_geom of `plan` (2-D runs as 3-D with a depth of one) and the start tables it points to (keep them
    alive while the geometry is in use)."""
    lift = 3 - len(plan.image_size)
    flat = [0] * lift + [s for ss in plan.starts for s in ss]
    starts_host = (C.c_int32 * len(flat))(*flat)
    starts_dev = torch.tensor(flat, dtype=torch.int32).to(device)
    g = SwGeomC()
    g.batch = batch
    one = (1,) * lift
    for d, (s, p, pp, r, n) in enumerate(zip(one + plan.image_size, (0,) * lift + plan.pad_lo, one + plan.padded,
                                             one + plan.roi, one + tuple(len(v) for v in plan.starts))):
        g.dhw[d], g.pad_lo[d], g.padded[d], g.roi[d], g.num[d] = s, p, pp, r, n
    g.starts_dev = starts_dev.data_ptr()
    g.starts_host = C.cast(starts_host, C.POINTER(C.c_int32))
    return g, (starts_host, starts_dev)


SW_LAUNCHES = {"gather": 0, "count": 1, "blend": 2, "finalize": 3}      # MPGAN_SW_* of include/mpgan_hip.h


def sw_kernel_name(launch: str, geom, *pointers) -> str:
    """The profiler's name of the kernel instance the `launch` ("gather", "count", "blend" or "finalize") runs for
    the geometry `geom` (a SwGeomC) and that launch's data pointers in its own argument order (integers or None;
    only their alignment is read), from the choice the launch itself makes (mpgan_sw_kernel_name).  Launches
    nothing; raises RuntimeError where the launch would refuse."""
    p = tuple(pointers) + (None,) * (3 - len(pointers))
    buf = C.create_string_buffer(64)
    check(lib().mpgan_sw_kernel_name(SW_LAUNCHES[launch], C.byref(geom), p[0], p[1], p[2], buf, len(buf)),
          "sw_kernel_name")
    return buf.value.decode()


def _same_device(dev, want: torch.device, what: str) -> None:
    if dev is None:
        return
    dev = torch.device(dev)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev != want:
        raise ValueError(f"{what} must be the input's device {want}, got {dev}")


def sliding_window_inference(inputs: torch.Tensor, roi_size, sw_batch_size: int, predictor: Callable,
                             overlap: float = 0.25, mode="constant", sigma_scale: float = 0.125,
                             padding_mode="constant", cval: float = 0.0, device=None, sw_device=None,
                             *args, **kwargs) -> torch.Tensor:
    """MONAI 0.4.0 `sliding_window_inference` on the device.

    inputs: float32 CUDA tensor (B, C_in, *S) with 2 or 3 spatial dims.  predictor(windows, *args, **kwargs) maps
    a contiguous (n, C_in, *roi) window batch (n <= sw_batch_size) to float32 CUDA (n, C_out, *roi); an eval-mode
    CasNetGenerator reads the batch in place.  Returns (B, C_out, *S).  `device` / `sw_device` may be given but
    must be the input's CUDA device.  Only padding_mode="constant" is implemented ("reflect" / "replicate" raise
    NotImplementedError).  Argument errors raise ValueError before any launch.
    """
    if not isinstance(inputs, torch.Tensor) or inputs.dim() not in (4, 5):
        raise ValueError("inputs must be a (B, C, *S) tensor with 2 or 3 spatial dims, got "
                         f"{tuple(inputs.shape) if isinstance(inputs, torch.Tensor) else type(inputs)}")
    if isinstance(sw_batch_size, bool) or int(sw_batch_size) != sw_batch_size or sw_batch_size < 1:
        raise ValueError(f"sw_batch_size must be a positive integer, got {sw_batch_size!r}")
    sw_batch_size = int(sw_batch_size)
    mode = _mode_name(mode)
    pm = getattr(padding_mode, "value", padding_mode)
    if pm != "constant":
        raise NotImplementedError(f"padding_mode {padding_mode!r}: only 'constant' padding is implemented")
    B, cin = int(inputs.shape[0]), int(inputs.shape[1])
    spatial = tuple(int(v) for v in inputs.shape[2:])
    if B < 1 or cin < 1 or min(spatial) < 1:
        raise ValueError(f"empty input of shape {tuple(inputs.shape)}")
    plan = plan_windows(spatial, roi_size, overlap)
    if mode == "gaussian" and not float(sigma_scale) > 0:
        raise ValueError(f"sigma_scale must be positive, got {sigma_scale!r}")
    if inputs.dtype != torch.float32 or not inputs.is_cuda:
        raise ValueError(f"inputs must be a float32 CUDA tensor, got {inputs.dtype} on {inputs.device}")
    _same_device(device, inputs.device, "device")
    _same_device(sw_device, inputs.device, "sw_device")

    dev = inputs.device
    x = inputs.contiguous()
    imp = _device_importance(plan.roi, mode, sigma_scale, dev)
    g, keep = _geometry(plan, B, dev)          # keep: the start tables g points to, alive until return
    gp = C.byref(g)
    L, st = lib(), _stream()

    total = B * plan.num_windows
    count = torch.empty(plan.padded, device=dev)
    check(L.mpgan_sw_count(gp, None if imp is None else imp.data_ptr(), count.data_ptr(), st), "sw_count")
    win = torch.empty((min(sw_batch_size, total), cin) + plan.roi, device=dev)
    acc, cout = None, None
    for first in range(0, total, sw_batch_size):
        n = min(sw_batch_size, total - first)
        w = win[:n]
        check(L.mpgan_sw_gather(gp, x.data_ptr(), cin, first, n, float(cval), w.data_ptr(), st), "sw_gather")
        pred = predictor(w, *args, **kwargs)
        if (not isinstance(pred, torch.Tensor) or pred.dtype != torch.float32 or pred.device != dev
                or pred.dim() != 2 + len(spatial) or pred.shape[0] != n or tuple(pred.shape[2:]) != plan.roi
                or pred.shape[1] < 1 or (cout is not None and pred.shape[1] != cout)):
            got = (tuple(pred.shape), pred.dtype, pred.device) if isinstance(pred, torch.Tensor) else type(pred)
            raise ValueError(f"predictor must return float32 {(n, cout or 'C_out') + plan.roi} on {dev}, got {got}")
        if acc is None:
            cout = int(pred.shape[1])
            acc = torch.zeros((B, cout) + plan.padded, device=dev)
        pred = pred.contiguous()
        check(L.mpgan_sw_blend(gp, pred.data_ptr(), cout, first, n, None if imp is None else imp.data_ptr(),
                               acc.data_ptr(), st), "sw_blend")
    out = torch.empty((B, cout) + spatial, device=dev)
    check(L.mpgan_sw_finalize(gp, acc.data_ptr(), cout, count.data_ptr(), out.data_ptr(), st), "sw_finalize")
    return out


class SlidingWindowInferer:
    """MONAI 0.4.0 `SlidingWindowInferer`: `inferer(inputs, network)` runs sliding_window_inference."""

    def __init__(self, roi_size, sw_batch_size: int = 1, overlap: float = 0.25, mode="constant",
                 sigma_scale: float = 0.125, padding_mode="constant", cval: float = 0.0, sw_device=None,
                 device=None):
        self.roi_size = roi_size
        self.sw_batch_size = sw_batch_size
        self.overlap = overlap
        self.mode = _mode_name(mode)
        self.sigma_scale = sigma_scale
        self.padding_mode = padding_mode
        self.cval = cval
        self.sw_device = sw_device
        self.device = device

    def __call__(self, inputs: torch.Tensor, network: Callable, *args, **kwargs) -> torch.Tensor:
        return sliding_window_inference(inputs, self.roi_size, self.sw_batch_size, network, self.overlap, self.mode,
                                        self.sigma_scale, self.padding_mode, self.cval, self.device, self.sw_device,
                                        *args, **kwargs)
