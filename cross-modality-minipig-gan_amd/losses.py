"""Differentiable losses beyond the reference trainer's own two (gan.py holds BCE and L1).

GlobalMutualInformationLoss restates MONAI 0.4.0's loss of that name, which the reference's scoring script imports
(code/GAN/metrics.py:19): mutual information from Parzen-window (Gaussian) soft bins, the differentiable form of
metrics.mutual_information.  MONAI is not installed here: the definition in include/mpgan_hip.h is what is pinned,
against a float64 torch restatement (tests/mi_loss_ref.py).  Forward and backward are fused HIP kernels
(csrc/mi_loss.hip): no (B, N, bins) weight tensor exists, and the result is bitwise reproducible.

SSIMLoss is 1 - the structural similarity that metrics.ssim scores a volume with (code/GAN/psnr_ssim_metric.py:88-106),
as a loss: the forward kernel of csrc/ssim_loss.hip also leaves the per-window coefficient maps of the closed-form
gradient, the backward kernel box-sums them.  Its definition is pinned in include/mpgan_hip.h against the float64
torch restatement tests/ssim_loss_ref.py.  With a mask or a threshold (ForegroundSSIMLoss) the same two kernels weight
every window by the foreground at its centre voxel and normalise per image on the device (pinned against
tests/masked_ssim_ref.py).

EdgeLoss is the edge-aware generator term of Ea-GAN (Yu et al. 2019): the L1 distance of the 3-D Sobel edge-magnitude
maps of the two volumes, over a replicate border.  csrc/edge_loss.hip holds the fused stencils (the forward writes no
map, the backward recomputes from the two inputs) and sobel_magnitude, the map itself as a differentiable op.  Ea-GAN's
code is not available here: the definition in include/mpgan_hip.h is what is pinned, against tests/edge_loss_ref.py.

MaskedL1Loss / ForegroundL1Loss weight the L1 by a foreground mask: an explicit mask, or
target > threshold formed on the fly with the threshold found on the device (preprocess.otsu_threshold).
csrc/foreground.hip holds the kernels; pinned against tests/foreground_ref.py."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .metrics import ValueRange, _ranges
from .preprocess import _otsu_config, check_threshold, item_thresholds, mask_bytes

_REDUCTIONS = ("mean", "sum", "none")
MAX_BINS = 32


def _check_reduction(reduction, who):
    if reduction not in _REDUCTIONS:
        raise ValueError(f"{who}: unknown reduction {reduction!r} (expected one of {_REDUCTIONS})")


def _pair_inputs(pred, target, who, shape_error):
    """The checks every pair loss makes, in their order: one shape, the loss's own rule for that shape
    (shape_error(shape) gives the complaint or None), two fp32 device tensors."""
    if pred.shape != target.shape:
        raise ValueError(f"{who}: shape mismatch, pred {tuple(pred.shape)} and target {tuple(target.shape)}")
    complaint = shape_error(tuple(pred.shape))
    if complaint:
        raise ValueError(f"{who}: {complaint}")
    if pred.dtype != torch.float32 or target.dtype != torch.float32 or not (pred.is_cuda and target.is_cuda):
        raise ValueError(f"{who}: expects two fp32 device tensors")


def _pair_forward(pred, target, reduction, per_channel=True):
    """What every pair loss's forward starts from: the contiguous inputs, (batch, channels, spatial), the empty loss of
    the reduction and d loss / d(sum over the items) for an upstream gradient of 1.  Every (b, c) image is an item;
    without per_channel the channels fold into the batch entry's item."""
    a, b = pred.contiguous(), target.contiguous()         # a contiguous view keeps its (possibly unaligned) offset
    batch, channels = a.shape[0], a.shape[1] if per_channel else 1
    loss = torch.empty((batch,) if reduction == "none" else (), device=a.device)
    scale = {"mean": 1.0 / (batch * channels), "sum": 1.0, "none": 1.0 / channels}[reduction]
    return a, b, (batch, channels, tuple(a.shape[2:])), loss, scale


def _pair_backward(ctx, gout, launch):
    """(grad pred, grad target) of a pair loss: launch(gout, wrt, out) for each input that needs_input_grad names."""
    gout = gout.contiguous()
    like = ctx.saved_tensors[0]
    return tuple(launch(gout, wrt, torch.empty_like(like)) if ctx.needs_input_grad[wrt] else None for wrt in (0, 1))


def _config(num_bins, sigma_ratio, reduction, value_range, who):
    if int(num_bins) != num_bins or not 2 <= int(num_bins) <= MAX_BINS:
        raise ValueError(f"{who}: num_bins must be an integer in [2, {MAX_BINS}], got {num_bins!r}")
    if not sigma_ratio > 0:
        raise ValueError(f"{who}: sigma_ratio must be positive, got {sigma_ratio!r}")
    _check_reduction(reduction, who)
    ranges = _ranges(value_range)
    if not (ranges[1] > ranges[0] and ranges[3] > ranges[2]):
        raise ValueError(f"{who}: value_range needs hi > lo, got {value_range!r}")
    return int(num_bins), float(sigma_ratio), ranges


def _mi_shape_error(shape):
    if len(shape) < 2 or 0 in shape:
        return f"expects non-empty (B, C, *spatial) tensors, got {shape}"


class _ParzenMIFn(torch.autograd.Function):
    """The reduced loss -mi; saves the two inputs and the K x K gradient coefficients of every item, so that a second
    backward (retain_graph) reads unscaled state."""

    @staticmethod
    def forward(ctx, pred, target, bins, sigma_ratio, nr, dr, ranges, reduction):
        a, b, (batch, _, _), loss, scale = _pair_forward(pred, target, reduction, per_channel=False)
        dev = a.device
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        ws = torch.empty(ops.parzen_mi_workspace(batch, a.numel() // batch, bins) // 8, dtype=torch.float64, device=dev)
        mi = torch.empty(batch, dtype=torch.float64, device=dev)
        coef = torch.empty((batch, 2, 32, 32), device=dev) if need_grad else None
        ops.parzen_mi_forward(a, b, batch, ranges, bins, sigma_ratio, nr, dr, ws, mi, None, coef, reduction, loss)
        ctx.cfg = (batch, ranges, bins, sigma_ratio, -scale)
        ctx.save_for_backward(a, b, coef)
        return loss

    @staticmethod
    def backward(ctx, gout):
        a, b, coef = ctx.saved_tensors
        batch, ranges, bins, sigma_ratio, scale = ctx.cfg
        return _pair_backward(ctx, gout, lambda g, wrt, out: ops.parzen_mi_backward(
            a, b, batch, ranges, bins, sigma_ratio, coef, g, scale, wrt, out)) + (None,) * 6


def global_mutual_information_loss(pred: torch.Tensor, target: torch.Tensor, num_bins: int = 23,
                                   sigma_ratio: float = 0.5, reduction: str = "mean", smooth_nr: float = 1e-7,
                                   smooth_dr: float = 1e-7, value_range: ValueRange = (0.0, 1.0)) -> torch.Tensor:
    """-MI of two (B, C, *spatial) fp32 device tensors from Gaussian soft bins; channels fold into samples.
    Values are mapped by clamp((x - lo) / (hi - lo), 0, 1) with value_range = (lo, hi) for both tensors or
    ((lo_pred, hi_pred), (lo_target, hi_target)); the default (0, 1) is MONAI's behaviour, (-1, 1) suits a tanh
    output.  reduction: "mean" (a scalar), "sum", or "none" ((B,)).  A NaN sample makes its item's loss NaN."""
    who = "global_mutual_information_loss"
    bins, sigma_ratio, ranges = _config(num_bins, sigma_ratio, reduction, value_range, who)
    _pair_inputs(pred, target, who, _mi_shape_error)
    return _ParzenMIFn.apply(pred, target, bins, sigma_ratio, float(smooth_nr), float(smooth_dr), ranges, reduction)


class GlobalMutualInformationLoss(nn.Module):
    """monai.losses.GlobalMutualInformationLoss(num_bins, sigma_ratio, reduction, smooth_nr, smooth_dr) with a
    value_range in addition (see global_mutual_information_loss)."""

    def __init__(self, num_bins: int = 23, sigma_ratio: float = 0.5, reduction: str = "mean", smooth_nr: float = 1e-7,
                 smooth_dr: float = 1e-7, value_range: ValueRange = (0.0, 1.0)):
        super().__init__()
        _config(num_bins, sigma_ratio, reduction, value_range, "GlobalMutualInformationLoss")
        self.num_bins, self.sigma_ratio, self.reduction = int(num_bins), float(sigma_ratio), reduction
        self.smooth_nr, self.smooth_dr, self.value_range = float(smooth_nr), float(smooth_dr), value_range

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return global_mutual_information_loss(pred, target, self.num_bins, self.sigma_ratio, self.reduction,
                                              self.smooth_nr, self.smooth_dr, self.value_range)


def parzen_joint_histogram(a: torch.Tensor, b: torch.Tensor, num_bins: int = 23, sigma_ratio: float = 0.5,
                           value_range: ValueRange = (0.0, 1.0)) -> torch.Tensor:
    """The float64 (B, num_bins, num_bins) Parzen-window joint distribution of two (B, C, *spatial) fp32 device
    tensors: rows indexed by a's bin, columns by b's; every item's entries sum to 1."""
    who = "parzen_joint_histogram"
    bins, sigma_ratio, ranges = _config(num_bins, sigma_ratio, "none", value_range, who)
    _pair_inputs(a, b, who, _mi_shape_error)
    a, b = a.contiguous(), b.contiguous()
    batch = a.shape[0]
    ws = torch.empty(ops.parzen_mi_workspace(batch, a.numel() // batch, bins) // 8, dtype=torch.float64,
                     device=a.device)
    mi = torch.empty(batch, dtype=torch.float64, device=a.device)
    joint = torch.empty((batch, bins, bins), dtype=torch.float64, device=a.device)
    ops.parzen_mi_forward(a, b, batch, ranges, bins, sigma_ratio, 1e-7, 1e-7, ws, mi, joint)
    return joint


SSIM_WINDOW = 7


def _ssim_config(value_range, reduction, who):
    _check_reduction(reduction, who)
    try:
        lo, hi = (float(v) for v in value_range)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: value_range must be one (lo, hi) pair, got {value_range!r}") from None
    if not hi > lo or hi - lo == float("inf"):
        raise ValueError(f"{who}: value_range needs finite hi > lo, got {value_range!r}")
    return lo, hi


def _ssim_shape_error(shape):
    if len(shape) not in (4, 5) or shape[0] < 1 or shape[1] < 1:
        return f"expects (B, C, H, W) or (B, C, D, H, W) tensors, got {shape}"
    spatial = shape[2:]
    windowed = spatial[1:] if len(spatial) == 3 and spatial[0] == 1 else spatial      # a depth of 1 is a slice
    if min(windowed) < SSIM_WINDOW:
        return f"spatial extents {spatial} are below the {SSIM_WINDOW}-wide window"


class _SSIMLossFn(torch.autograd.Function):
    """The reduced loss 1 - ssim; saves the two inputs and the float64 coefficient maps of the gradients that
    needs_input_grad asks for.  With a weight per window -- one of mask (uint8, the inputs' shape) and thr (fp32, one per
    item) -- it also saves stats = (ssim_item, n_item) per item, from which the backward reads every item's divisor on
    the device; without one there is no stats tensor and the plain entry points run.  backward only reads what was
    saved, so nothing syncs and a second backward (retain_graph) gives the same bits."""

    @staticmethod
    def forward(ctx, pred, target, mask, thr, lo, hi, reduction):
        a, b, (batch, channels, spatial), loss, scale = _pair_forward(pred, target, reduction)
        items, dev = batch * channels, a.device
        weighted = mask is not None or thr is not None
        grads = int(ctx.needs_input_grad[0]) | (int(ctx.needs_input_grad[1]) << 1)
        ws_bytes, coef_bytes = ops.ssim_loss_workspace(spatial, items, grads, weighted)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
        coef = torch.empty(coef_bytes // 8, dtype=torch.float64, device=dev) if grads else None
        stats = torch.empty((items, 2), dtype=torch.float64, device=dev) if weighted else None
        ops.ssim_loss_forward(a, b, spatial, items, channels, lo, hi, grads, ws, coef, reduction, loss, mask=mask,
                              thr=thr, stats=stats)
        ctx.cfg = (spatial, items, channels, lo, grads, -scale)
        ctx.save_for_backward(a, b, coef, stats)
        return loss

    @staticmethod
    def backward(ctx, gout):
        a, b, coef, stats = ctx.saved_tensors
        spatial, items, channels, lo, grads, scale = ctx.cfg
        return _pair_backward(ctx, gout, lambda g, wrt, out: ops.ssim_loss_backward(
            a, b, spatial, items, channels, lo, grads, coef, g, scale, wrt, out, stats)) + (None,) * 5


def ssim_loss(pred: torch.Tensor, target: torch.Tensor, value_range=(0.0, 1.0), reduction: str = "mean", *,
              mask: torch.Tensor = None, threshold=None, bins: int = 256) -> torch.Tensor:
    """1 - SSIM of two (B, C, H, W) or (B, C, D, H, W) fp32 device tensors: every (b, c) image is one item, scored as
    metrics.ssim scores it (7-wide uniform window on every spatial axis, K1 = 0.01, K2 = 0.03, sample covariance,
    mean over the windows inside the image) with data range hi - lo of value_range = (lo, hi); lo is subtracted from
    both tensors, nothing is clamped.  reduction: "mean" (a scalar over the B * C items), "sum", or "none" ((B,), each
    entry the mean over its channels).  Differentiable in both arguments; bitwise reproducible.

    With at most one of mask and threshold the mean runs over the foreground windows alone: a window
    counts when its centre voxel is foreground, which is the map of S cropped by its 3-sample border and averaged
    over the mask.
      mask       a bool / uint8 device tensor of pred's shape, or with channel extent 1 (broadcast over the channels);
      threshold  "otsu", a number, or an fp32 device tensor with one value per (b, c) image: the foreground is
                 target > threshold, read on the fly -- no mask tensor exists and nothing syncs.  "otsu" takes
                 preprocess.otsu_threshold(target, bins, value_range).
    An image without a foreground window adds a loss of 0 and an exactly-zero gradient; nothing flows into the mask or
    the threshold.  Defined in include/mpgan_hip.h ("masked SSIM"), pinned against tests/masked_ssim_ref.py."""
    who = "ssim_loss"
    lo, hi = _ssim_config(value_range, reduction, who)
    if mask is not None and threshold is not None:
        raise ValueError(f"{who}: give at most one of mask and threshold")
    if mask is not None and pred.shape == target.shape:   # a mismatch of the pair itself is _pair_inputs' complaint
        mask = mask_bytes(mask, pred, who, broadcast_channels=True)
    elif threshold is not None:
        check_threshold(threshold, who)
    _pair_inputs(pred, target, who, _ssim_shape_error)
    thr = None if threshold is None else item_thresholds(target.contiguous(), threshold, bins, value_range, who)
    return _SSIMLossFn.apply(pred, target, mask, thr, lo, hi, reduction)


class SSIMLoss(nn.Module):
    """ssim_loss as a module: SSIMLoss(value_range=(-1.0, 1.0)) suits a tanh output.  forward(pred, target, mask=None):
    without a mask the module's threshold is used, and without either the whole image is scored."""

    def __init__(self, value_range=(0.0, 1.0), reduction: str = "mean", threshold=None, bins: int = 256):
        super().__init__()
        _ssim_config(value_range, reduction, "SSIMLoss")
        if threshold is not None:
            check_threshold(threshold, "SSIMLoss")
            _otsu_config(bins, value_range, "SSIMLoss")
        self.value_range, self.reduction, self.threshold, self.bins = tuple(value_range), reduction, threshold, bins

    def forward(self, pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
        return ssim_loss(pred, target, self.value_range, self.reduction, mask=mask,
                         threshold=None if mask is not None else self.threshold, bins=self.bins)


class ForegroundSSIMLoss(nn.Module):
    """(pred, target) -> 1 - the SSIM over the windows whose centre lies in the foreground of target,
    target > threshold ("otsu": Otsu's threshold of every target image over value_range, on the device; or a number):
    the generator term GAN's fg_ssim_weight switches on.  The air around the anatomy, whose flat windows score S = 1,
    carries no weight."""

    def __init__(self, threshold="otsu", value_range=(-1.0, 1.0), bins: int = 256):
        super().__init__()
        check_threshold(threshold, "ForegroundSSIMLoss")
        if isinstance(threshold, torch.Tensor):
            raise ValueError("ForegroundSSIMLoss: threshold must be \"otsu\" or a finite number")
        _otsu_config(bins, value_range, "ForegroundSSIMLoss")
        self.threshold, self.value_range, self.bins = threshold, tuple(value_range), int(bins)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return ssim_loss(pred, target, self.value_range, threshold=self.threshold, bins=self.bins)


def _edge_config(eps, reduction, who):
    _check_reduction(reduction, who)
    try:
        eps = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: eps must be a positive number, got {eps!r}") from None
    if not (eps > 0 and eps != float("inf") and torch.tensor(eps, dtype=torch.float32).item() > 0):
        raise ValueError(f"{who}: eps must be positive and finite in fp32, got {eps!r}")
    return eps


def _edge_shape_error(shape):
    if len(shape) not in (4, 5) or 0 in shape:
        return f"expects non-empty (B, C, H, W) or (B, C, D, H, W) tensors, got {shape}"


def _edge_input(x, who):
    complaint = _edge_shape_error(tuple(x.shape))
    if complaint:
        raise ValueError(f"{who}: {complaint}")
    if x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"{who}: expects fp32 device tensors")


class _SobelMagnitudeFn(torch.autograd.Function):
    """m(x); saves x alone, backward recomputes G and m from it."""

    @staticmethod
    def forward(ctx, x, eps):
        x = x.contiguous()                                # a contiguous view keeps its (possibly unaligned) offset
        ctx.cfg = (tuple(x.shape[2:]), x.shape[0] * x.shape[1], eps)
        ctx.save_for_backward(x)
        return ops.sobel_magnitude_forward(x, *ctx.cfg, torch.empty_like(x))

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        return ops.sobel_magnitude_backward(x, *ctx.cfg, gout.contiguous(), torch.empty_like(x)), None


def sobel_magnitude(x: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """The Sobel edge-magnitude map sqrt(sum_k G_k^2 + eps) of a (B, C, H, W) or (B, C, D, H, W) fp32 device tensor, in
    the shape of x: G_k is the 3^d Sobel operator along axis k, normalised so that a ramp of slope 1 answers 1, over a
    replicate border (a constant image has no edges, up to its faces).  Differentiable; the gradient is 0 in flat
    regions.  The definition is pinned in include/mpgan_hip.h against tests/edge_loss_ref.py."""
    who = "sobel_magnitude"
    eps = _edge_config(eps, "none", who)
    _edge_input(x, who)
    return _SobelMagnitudeFn.apply(x, eps)


class _EdgeLossFn(torch.autograd.Function):
    """The reduced loss; saves the two inputs and nothing else: backward forms the signs from them again, so a second
    backward (retain_graph) gives the same bits."""

    @staticmethod
    def forward(ctx, pred, target, eps, reduction):
        a, b, (batch, channels, spatial), loss, scale = _pair_forward(pred, target, reduction)
        items = batch * channels
        ws = torch.empty(ops.edge_loss_workspace(spatial, items) // 8, dtype=torch.float64, device=a.device)
        ops.edge_loss_forward(a, b, spatial, items, channels, eps, ws, reduction, loss)
        ctx.cfg = (spatial, items, channels, eps, scale)
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        spatial, items, channels, eps, scale = ctx.cfg
        return _pair_backward(ctx, gout, lambda g, wrt, out: ops.edge_loss_backward(
            a, b, spatial, items, channels, eps, g, scale, wrt, out)) + (None,) * 2


def edge_loss(pred: torch.Tensor, target: torch.Tensor, eps: float = 1e-6, reduction: str = "mean") -> torch.Tensor:
    """The edge-aware term of Ea-GAN (Yu et al. 2019): mean |m(pred) - m(target)| of the Sobel edge-magnitude maps
    (sobel_magnitude) of two (B, C, H, W) or (B, C, D, H, W) fp32 device tensors; every (b, c) image is one item.
    reduction: "mean" (a scalar over the B * C items), "sum", or "none" ((B,), each entry the mean over its channels).
    One fused kernel each way (csrc/edge_loss.hip): no gradient or magnitude map is materialised.  Differentiable in
    both arguments; bitwise reproducible."""
    who = "edge_loss"
    eps = _edge_config(eps, reduction, who)
    _pair_inputs(pred, target, who, _edge_shape_error)
    return _EdgeLossFn.apply(pred, target, eps, reduction)


class EdgeLoss(nn.Module):
    """edge_loss as a module."""

    def __init__(self, eps: float = 1e-6, reduction: str = "mean"):
        super().__init__()
        self.eps, self.reduction = _edge_config(eps, reduction, "EdgeLoss"), reduction

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return edge_loss(pred, target, self.eps, self.reduction)


def _masked_l1_config(fg_weight, bg_weight, reduction, who):
    _check_reduction(reduction, who)
    try:
        w_fg, w_bg = float(fg_weight), float(bg_weight)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: fg_weight and bg_weight must be numbers, got {fg_weight!r} and {bg_weight!r}") from None
    if not (0.0 <= w_fg < float("inf") and 0.0 <= w_bg < float("inf")):
        raise ValueError(f"{who}: fg_weight and bg_weight must be finite and >= 0, got {fg_weight!r} and {bg_weight!r}")
    return w_fg, w_bg


def _masked_l1_shape_error(shape):
    if len(shape) not in (4, 5) or 0 in shape:
        return f"expects non-empty (B, C, H, W) or (B, C, D, H, W) tensors, got {shape}"


class _MaskedL1Fn(torch.autograd.Function):
    """The reduced loss; saves the two inputs, the mask source and every item's denominator.  One backward launch
    writes both gradients; it only reads what was saved, so a second backward (retain_graph) gives the same bits."""

    @staticmethod
    def forward(ctx, pred, target, mask, thr, w_fg, w_bg, reduction):
        a, b, (batch, channels, _), loss, scale = _pair_forward(pred, target, reduction)
        items = batch * channels
        den = torch.empty(items, dtype=torch.float64, device=a.device)
        ops.masked_l1_forward(a, b, items, channels, mask, thr, w_fg, w_bg, den, reduction, loss)
        ctx.cfg = (items, channels, w_fg, w_bg, scale)
        ctx.save_for_backward(a, b, den, mask, thr)
        return loss

    @staticmethod
    def backward(ctx, gout):
        a, b, den, mask, thr = ctx.saved_tensors
        items, channels, w_fg, w_bg, scale = ctx.cfg
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            ops.masked_l1_backward(a, b, items, channels, mask, thr, w_fg, w_bg, den, gout.contiguous(), scale, da, db)
        return (da, db) + (None,) * 5


def masked_l1_loss(pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor = None, *, threshold=None,
                   fg_weight: float = 1.0, bg_weight: float = 0.0, reduction: str = "mean", bins: int = 256,
                   value_range=(-1.0, 1.0)) -> torch.Tensor:
    """The mask-weighted L1 of two (B, C, H, W) or (B, C, D, H, W) fp32 device tensors: per (b, c) image
    sum_i w_i |pred_i - target_i| / sum_i w_i with w_i = fg_weight inside the mask and bg_weight outside (0 for an image
    whose weights sum to 0).  Exactly one of:
      mask       a bool / uint8 device tensor of pred's shape, or with channel extent 1 (broadcast over the channels);
      threshold  "otsu", a number, or an fp32 device tensor with one value per (b, c) image: the mask is
                 target > threshold, formed on the fly -- no mask tensor exists and nothing syncs.  "otsu" takes
                 preprocess.otsu_threshold(target, bins, value_range).
    reduction: "mean" (a scalar over the B * C images), "sum", or "none" ((B,), each entry the mean over its channels).
    Differentiable in pred and target (d target = -d pred); nothing flows into the mask or the threshold.  Sums are
    fp64 in a fixed order: bitwise reproducible.  Defined in include/mpgan_hip.h, pinned against
    tests/foreground_ref.py."""
    who = "masked_l1_loss"
    w_fg, w_bg = _masked_l1_config(fg_weight, bg_weight, reduction, who)
    if (mask is None) == (threshold is None):
        raise ValueError(f"{who}: give exactly one of mask and threshold")
    if mask is None:
        check_threshold(threshold, who)
    elif pred.shape == target.shape:                      # a mismatch of the pair itself is _pair_inputs' complaint
        mask = mask_bytes(mask, pred, who, broadcast_channels=True)
    _pair_inputs(pred, target, who, _masked_l1_shape_error)
    thr = None if mask is not None else item_thresholds(target.contiguous(), threshold, bins, value_range, who)
    return _MaskedL1Fn.apply(pred, target, mask, thr, w_fg, w_bg, reduction)


class MaskedL1Loss(nn.Module):
    """masked_l1_loss as a module: forward(pred, target, mask=None); without a mask the module's threshold is used."""

    def __init__(self, threshold=None, fg_weight: float = 1.0, bg_weight: float = 0.0, reduction: str = "mean",
                 bins: int = 256, value_range=(-1.0, 1.0)):
        super().__init__()
        self.fg_weight, self.bg_weight = _masked_l1_config(fg_weight, bg_weight, reduction, "MaskedL1Loss")
        if threshold is not None:
            check_threshold(threshold, "MaskedL1Loss")
        self.threshold, self.reduction, self.bins, self.value_range = threshold, reduction, bins, tuple(value_range)

    def forward(self, pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
        return masked_l1_loss(pred, target, mask, threshold=None if mask is not None else self.threshold,
                              fg_weight=self.fg_weight, bg_weight=self.bg_weight, reduction=self.reduction,
                              bins=self.bins, value_range=self.value_range)


class ForegroundL1Loss(nn.Module):
    """(pred, target) -> the mean |pred - target| over the foreground of target, target > threshold ("otsu": Otsu's
    threshold of every target image over value_range, on the device; or a number): the generator term GAN's fg_weight
    switches on.  The background carries no weight."""

    def __init__(self, threshold="otsu", value_range=(-1.0, 1.0), bins: int = 256):
        super().__init__()
        check_threshold(threshold, "ForegroundL1Loss")
        if isinstance(threshold, torch.Tensor):
            raise ValueError("ForegroundL1Loss: threshold must be \"otsu\" or a finite number")
        _otsu_config(bins, value_range, "ForegroundL1Loss")
        self.threshold, self.value_range, self.bins = threshold, tuple(value_range), int(bins)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return masked_l1_loss(pred, target, threshold=self.threshold, bins=self.bins, value_range=self.value_range)
