#!/usr/bin/env python3
"""joint_histogram + mutual_information beside the torch composition on the device (needs an MI355X).

    python tools/bench_mutual_information.py [--iters 20] [--repeats 7]

Rows: one 128^3 pair and 16 x 256^2 batched, 64 and 256 bins over [0, 256], two inputs each: independent uniform
integer levels 0..255 (every counter of the histogram is hit), and an MRI-like pair with 60 % of the voxels exactly
0 in both images (most voxels crowd the counter (0, 0)).  The torch composition applies the same fp32 binning
with torch ops, counts with torch.bincount and forms the entropies in torch float64; its histogram must equal
the kernel's.  Each figure: HIP events around `iters` calls after a warm-up, per call; median of `repeats`
windows, spread = max - min of the windows; the windows of the two paths alternate in one process.  GB/s is the
two fp32 input reads (8 bytes per voxel) over the kernel path's time.  The last column is joint_histogram alone."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpgan_amd import metrics  # noqa: E402

LO, HI = 0.0, 256.0


def torch_histogram(a, b, bins, batched):
    batch = a.shape[0] if batched else 1
    a, b = a.reshape(batch, -1), b.reshape(batch, -1)
    s = float(np.float32(bins) / (np.float32(HI) - np.float32(LO)))
    ia = ((a - LO) * s).floor().clamp_(max=bins - 1).long()
    ib = ((b - LO) * s).floor().clamp_(max=bins - 1).long()
    keep = (a >= LO) & (a <= HI) & (b >= LO) & (b <= HI)
    item = torch.arange(batch, device=a.device).view(batch, 1) * (bins * bins)
    key = torch.where(keep, ia * bins + ib + item, batch * bins * bins)          # dropped voxels: one extra counter
    return torch.bincount(key.flatten(), minlength=batch * bins * bins + 1)[:-1].view(batch, bins, bins)


def torch_mutual_information(a, b, bins, batched):
    h = torch_histogram(a, b, bins, batched)
    n = h.sum((1, 2)).double()
    ent = [n.log() - torch.xlogy(c, c).sum(-1) / n
           for c in (h.sum(2).double(), h.sum(1).double(), h.double().flatten(1))]
    return h, ent[0] + ent[1] - ent[2], (ent[0] + ent[1]) / ent[2]


def inputs(shape, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randint(0, 256, shape, device="cuda", generator=g).float()
    if kind == "uniform":
        return a, torch.randint(0, 256, shape, device="cuda", generator=g).float()
    b = (0.7 * a + 20.0 * torch.randn(shape, device="cuda", generator=g)).round().clamp_(0, 255)
    zero = torch.rand(shape, device="cuda", generator=g) < 0.6
    return a.masked_fill(zero, 0.0), b.masked_fill(zero, 0.0)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    print(f"ms per call: median of {args.repeats} windows x {args.iters} calls (+- = max - min of the windows)")
    print(f"{'row':34s} {'kernels':>16s} {'GB/s':>7s} {'torch':>16s} {'ratio':>6s} {'hist only':>16s}")
    lost = []
    for label, shape, batched in (("128^3", (128, 128, 128), False), ("16x256^2", (16, 256, 256), True)):
        for kind in ("uniform", "mri-like"):
            a, b = inputs(shape, kind, seed=1)
            for bins in (64, 256):
                paths = {
                    "kernels": lambda: metrics.mutual_information(a, b, bins, (LO, HI), batched=batched),
                    "torch": lambda: torch_mutual_information(a, b, bins, batched),
                    "hist": lambda: metrics.joint_histogram(a, b, bins, (LO, HI), batched=batched),
                }
                ours = metrics.joint_histogram(a, b, bins, (LO, HI), batched=True if batched else False)
                theirs, mi_t, _ = torch_mutual_information(a, b, bins, batched)
                mi_k = metrics.mutual_information(a, b, bins, (LO, HI), batched=batched)["mi"]
                if not torch.equal(ours.view(theirs.shape), theirs) or float((mi_k - mi_t).abs().max()) > 1e-9:
                    raise SystemExit(f"{label} {kind} {bins}: the two paths disagree")
                for fn in paths.values():
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                t = {k: [] for k in paths}
                for _ in range(args.repeats):
                    for k, fn in paths.items():
                        t[k].append(window(fn, args.iters))
                med = {k: statistics.median(v) for k, v in t.items()}
                spr = {k: max(v) - min(v) for k, v in t.items()}
                gbs = 8.0 * a.numel() / (med["kernels"] * 1e-3) / 1e9
                name = f"{label} {kind} bins {bins}"
                print(f"{name:34s} {med['kernels']:9.4f} +-{spr['kernels']:6.4f} {gbs:7.0f} "
                      f"{med['torch']:9.4f} +-{spr['torch']:6.4f} {med['torch'] / med['kernels']:6.1f} "
                      f"{med['hist']:9.4f} +-{spr['hist']:6.4f}")
                if med["kernels"] > med["torch"] + spr["torch"]:
                    lost.append(name)
    print("rows on which the kernel path is slower than the torch composition by more than its spread:", lost or "none")
    sys.exit(1 if lost else 0)


if __name__ == "__main__":
    main()
