"""CPU restatement of MONAI 0.4.0 sliding_window_inference (monai/inferers/utils.py) and the helpers it calls
(monai/data/utils.py: dense_patch_slices, compute_importance_map; monai/networks/layers: gaussian_1d,
GaussianFilter), written from their public source in plain torch on the CPU, fp32.  MONAI itself is not
importable here; this file is the yardstick of tests/test_sliding_window*.py, independent of the package."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def fall_back_tuple(user, default):
    return tuple(d if (u is None or u <= 0) else u for u, d in zip(user, default))


def get_scan_interval(image_size, roi_size, num_spatial_dims, overlap):
    scan_interval = []
    for i in range(num_spatial_dims):
        if roi_size[i] == image_size[i]:
            scan_interval.append(int(roi_size[i]))
        else:
            interval = int(roi_size[i] * (1 - overlap))
            scan_interval.append(interval if interval > 0 else 1)
    return tuple(scan_interval)


def dense_patch_slices(image_size, patch_size, scan_interval):
    num_spatial_dims = len(image_size)
    scan_num = []
    for i in range(num_spatial_dims):
        if scan_interval[i] == 0:
            scan_num.append(1)
        else:
            num = int(math.ceil(float(image_size[i]) / scan_interval[i]))
            scan_dim = next((d for d in range(num) if d * scan_interval[i] + patch_size[i] >= image_size[i]), None)
            scan_num.append(scan_dim + 1 if scan_dim is not None else 1)
    starts = []
    for dim in range(num_spatial_dims):
        dim_starts = []
        for idx in range(scan_num[dim]):
            start_idx = idx * scan_interval[dim]
            start_idx -= max(start_idx + patch_size[dim] - image_size[dim], 0)
            dim_starts.append(start_idx)
        starts.append(dim_starts)
    out = np.asarray([x.flatten() for x in np.meshgrid(*starts, indexing="ij")]).T
    return [tuple(slice(int(s), int(s) + patch_size[d]) for d, s in enumerate(x)) for x in out]


def gaussian_1d(sigma, truncated=4.0):
    tail = int(sigma * truncated + 0.5)
    sigma2 = sigma * sigma
    x = torch.arange(-tail, tail + 1, dtype=torch.float)
    out = torch.exp(-0.5 / sigma2 * x ** 2)
    out /= out.sum()
    return out


def gaussian_filter(x, sigmas):
    """GaussianFilter(spatial_dims, sigma).forward: separable conv, dim 0 first, zero padding."""
    sp = x.dim() - 2
    conv = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}[sp]
    for d in range(sp):
        k = gaussian_1d(sigmas[d])
        shape = [1, 1] + [1] * sp
        shape[d + 2] = -1
        padding = [0] * sp
        padding[d] = (k.shape[0] - 1) // 2
        x = conv(x, k.reshape(shape), padding=padding)
    return x


def compute_importance_map(patch_size, mode="constant", sigma_scale=0.125):
    if mode == "constant":
        return torch.ones(patch_size, dtype=torch.float32)
    center = [i // 2 for i in patch_size]
    sigmas = [i * sigma_scale for i in patch_size]
    m = torch.zeros(patch_size)
    m[tuple(center)] = 1
    m = gaussian_filter(m.unsqueeze(0).unsqueeze(0), sigmas).squeeze(0).squeeze(0)
    m = m / torch.max(m)
    m = m.float()
    m[m == 0] = torch.min(m[m != 0])
    return m


def sliding_window(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant", sigma_scale=0.125,
                   cval=0.0):
    """sliding_window_inference with padding_mode="constant" on CPU tensors; `predictor` is called with each window
    batch (CPU) in order.  Returns (output, [window batches])."""
    nsd = inputs.dim() - 2
    image_size_ = list(inputs.shape[2:])
    batch_size = inputs.shape[0]
    roi_size = fall_back_tuple(roi_size, image_size_)
    image_size = tuple(max(image_size_[i], roi_size[i]) for i in range(nsd))
    pad_size = []
    for k in range(len(inputs.shape) - 1, 1, -1):
        diff = max(roi_size[k - 2] - inputs.shape[k], 0)
        half = diff // 2
        pad_size.extend([half, diff - half])
    inputs = F.pad(inputs, pad=pad_size, mode="constant", value=cval)
    scan_interval = get_scan_interval(image_size, roi_size, nsd, overlap)
    slices = dense_patch_slices(image_size, roi_size, scan_interval)
    num_win = len(slices)
    total_slices = num_win * batch_size
    importance_map = compute_importance_map(roi_size, mode, sigma_scale)
    output_image = count_map = None
    batches = []
    for slice_g in range(0, total_slices, sw_batch_size):
        slice_range = range(slice_g, min(slice_g + sw_batch_size, total_slices))
        unravel = [[slice(idx // num_win, idx // num_win + 1), slice(None)] + list(slices[idx % num_win])
                   for idx in slice_range]
        window_data = torch.cat([inputs[tuple(s)] for s in unravel])
        batches.append(window_data)
        seg_prob = predictor(window_data)
        if output_image is None:
            shape = [batch_size, seg_prob.shape[1]] + list(image_size)
            output_image = torch.zeros(shape, dtype=torch.float32)
            count_map = torch.zeros(shape, dtype=torch.float32)
        for idx, orig in zip(slice_range, unravel):
            output_image[tuple(orig)] += importance_map * seg_prob[idx - slice_g]
            count_map[tuple(orig)] += importance_map
    output_image = output_image / count_map
    crop = [slice(None), slice(None)]
    for d in range(nsd):
        lo = pad_size[2 * (nsd - 1 - d)]
        crop.append(slice(lo, lo + image_size_[d]))
    return output_image[tuple(crop)], batches
