#!/usr/bin/env python3
"""The foreground-mask calls beside their torch compositions on the device (needs an MI355X).

    python tools/bench_foreground.py [--iters 20] [--repeats 7] [--no-step]

Shapes: (4, 1, 128, 128, 128) and (16, 1, 256, 256); a head-like pair, tissue values inside an ellipsoid on a background
at -1.  One row per call, the library's path ("ours", through the public functions, with their allocations) beside the
composition a user would write with torch on the same device:

    otsu      preprocess.otsu_threshold (256 bins)    | torch.histc per item + Otsu by cumulative sums
    mask+box  foreground_mask's three outputs at once | x > thr, then min / max of nonzero() per item (syncs)
    l1        masked_l1_loss(threshold=thr) forward   | (w * (p - t).abs()).sum() / w.sum() per item, w from where(),
              + backward for pred                     | with autograd
              ("launches alone": the same four launches through mpgan_amd.ops on preallocated outputs, without the
              autograd node, the argument checks and their allocations)
    errors    image_errors(a, b, mask=...)            | (a - b)[mask]: abs().mean() and square mean

Each figure: HIP events around `iters` calls after a warm-up, per call; median of `repeats` windows, spread = max - min
of the windows; the windows of the two paths alternate in one process.  GB/s is the least traffic of the call (every
input read once, every output written once) over ours' time.  The last rows time a fit_batch of variant A at the C5
shape (4 x 128^3, bf16 storage) with fg_weight 0 and 1.  No figure is a condition: the exit status is 0 whichever path
is faster."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpgan_amd import losses, metrics, ops  # noqa: E402
from mpgan_amd import preprocess as P  # noqa: E402

LO, HI, BINS = -1.0, 1.0, 256


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(paths, iters, repeats):
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in paths}
    for _ in range(repeats):
        for k, fn in paths.items():
            t[k].append(window(fn, iters))
    return {k: statistics.median(v) for k, v in t.items()}, {k: max(v) - min(v) for k, v in t.items()}


def head_pair(shape, seed):
    """(pred, target): tissue in [0.1, 0.9] inside an ellipsoid, -1 outside; pred is target plus noise."""
    g = torch.Generator().manual_seed(seed)
    axes = [torch.linspace(-1, 1, s) for s in shape[2:]]
    grid = torch.meshgrid(*axes, indexing="ij")
    inside = sum((c / r) ** 2 for c, r in zip(grid, (0.7, 0.55, 0.45)[-len(axes):])) < 1.0
    target = torch.where(inside, torch.rand(shape, generator=g) * 0.8 + 0.1, torch.full(shape, -1.0))
    pred = (target + 0.1 * torch.randn(shape, generator=g)).clamp(-1, 1)
    return pred.cuda(), target.cuda()


def torch_otsu(x):
    out = []
    centres = LO + (torch.arange(BINS, device=x.device, dtype=torch.float64) + 0.5) * (HI - LO) / BINS
    for item in x.flatten(0, 1):
        n = torch.histc(item, BINS, LO, HI).double()
        w0 = n.cumsum(0)
        w1 = n.sum() - w0
        s0 = (n * centres).cumsum(0)
        s1 = (n * centres).sum() - s0
        var = w0 * w1 * (s0 / w0.clamp(min=1) - s1 / w1.clamp(min=1)) ** 2
        out.append(centres[var[:-1].argmax()].float())
    return torch.stack(out).reshape(x.shape[:2])


def torch_mask_box(x, thr):
    mask = x > thr.reshape(x.shape[:2] + (1,) * (x.dim() - 2))
    boxes = []
    for m in mask.flatten(0, 1):
        idx = m.nonzero()
        boxes.append(torch.stack([idx.min(0).values, idx.max(0).values + 1]))
    return mask.to(torch.uint8), torch.stack(boxes), mask.flatten(2).sum(2)


def torch_masked_l1(p, t, thr):
    w = torch.where(t > thr.reshape(t.shape[:2] + (1,) * (t.dim() - 2)), 1.0, 0.0)
    return ((w * (p - t).abs()).flatten(1).sum(1) / w.flatten(1).sum(1)).mean()


def torch_masked_errors(a, b, mask):
    d = (a - b)[mask]
    mse = (d * d).mean()
    return d.abs().mean(), mse, 10 * torch.log10(4.0 / mse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the fit_batch rows")
    args = ap.parse_args()
    print(f"ms per call: median of {args.repeats} windows x {args.iters} calls (+- = max - min)")
    print(f"{'row':22s} {'ours':>16s} {'GB/s':>6s} {'torch':>16s} {'torch/ours':>10s}")
    lost = []
    for label, shape in (("4x128^3", (4, 1, 128, 128, 128)), ("16x256^2", (16, 1, 256, 256))):
        pred, target = head_pair(shape, seed=1)
        n = target.numel()
        thr = P.otsu_threshold(target)
        ref = torch_otsu(target)
        # var_k is flat across the empty bins between background and tissue and the two paths round it differently:
        # the thresholds may sit anywhere in that gap, the masks they give must be the same
        view = shape[:2] + (1,) * (len(shape) - 2)
        if not torch.equal(target > thr.reshape(view), target > ref.reshape(view)):
            raise SystemExit(f"{label}: the Otsu paths disagree: {thr.flatten().tolist()} and {ref.flatten().tolist()}")
        flat_thr = thr.reshape(-1).contiguous()
        items, spatial = shape[0] * shape[1], shape[2:]
        mask = torch.empty(shape, dtype=torch.uint8, device="cuda")
        box = torch.empty((items, 2, 3), dtype=torch.int32, device="cuda")
        count = torch.empty(items, dtype=torch.int64, device="cuda")
        p = pred.clone().requires_grad_(True)

        def ours_mask():
            ops.foreground_mask(target, spatial, items, flat_thr, mask=mask, box=box, count=count)

        def ours_l1():
            return torch.autograd.grad(losses.masked_l1_loss(p, target, threshold=flat_thr), (p,))

        den = torch.empty(items, dtype=torch.float64, device="cuda")
        loss, one, grad = torch.empty((), device="cuda"), torch.ones((), device="cuda"), torch.empty_like(pred)

        def kernels_l1():                                 # the launches alone, on preallocated outputs
            ops.masked_l1_forward(pred, target, items, 1, None, flat_thr, 1.0, 0.0, den, "mean", loss)
            ops.masked_l1_backward(pred, target, items, 1, None, flat_thr, 1.0, 0.0, den, one, 1.0 / items, grad, None)

        def torch_l1():
            return torch.autograd.grad(torch_masked_l1(p, target, thr), (p,))

        ours_mask()
        tm, tb, tc = torch_mask_box(target, thr)
        nd = len(spatial)
        if not (torch.equal(tm, mask) and torch.equal(tb.int(), box[:, :, 3 - nd:]) and torch.equal(tc.flatten(), count)):
            raise SystemExit(f"{label}: the mask paths disagree")
        go, gt = ours_l1()[0], torch_l1()[0]
        if float((go - gt).abs().max()) > 1e-5 * float(gt.abs().max()):
            raise SystemExit(f"{label}: the masked-L1 gradients disagree")
        del go, gt, tm, tb, tc
        bmask = mask.bool()
        rows = (("otsu", 4 * n, lambda: P.otsu_threshold(target), lambda: torch_otsu(target)),
                ("mask+box+count", 5 * n, ours_mask, lambda: torch_mask_box(target, thr)),
                ("l1 fwd+bwd pred", 20 * n, ours_l1, torch_l1),
                ("l1 launches alone", 20 * n, kernels_l1, torch_l1),
                ("errors", 9 * n, lambda: metrics.image_errors(pred, target, 2.0, mask=mask),
                 lambda: torch_masked_errors(pred, target, bmask)))
        for name, nbytes, ours, composed in rows:
            med, spr = measure({"ours": ours, "torch": composed}, args.iters, args.repeats)
            row = f"{label} {name}"
            print(f"{row:22s} {med['ours']:9.4f} +-{spr['ours']:6.4f} {nbytes / 1e9 / med['ours'] * 1e3:6.0f} "
                  f"{med['torch']:9.4f} +-{spr['torch']:6.4f} {med['torch'] / med['ours']:10.1f}")
            if med["ours"] > med["torch"]:
                lost.append(row)
        del pred, target, mask, p
        torch.cuda.empty_cache()
    if not args.no_step:
        from mpgan_amd.gan import GAN
        spatial = (128, 128, 128)
        t1, t2 = head_pair((4, 1) + spatial, seed=6)
        batch = {"t1w": t1, "t2w": t2}
        steps = {}
        for w in (0.0, 1.0):
            torch.manual_seed(0)
            m = GAN(1, *spatial, storage_dtype="bf16", fg_weight=w)
            opts, _ = m.configure_optimizers()
            steps[f"C5 4x128^3 bf16 fg_weight {w}"] = (lambda m=m, opts=opts: m.fit_batch(batch, 0, opts))
        med, spr = measure(steps, max(args.iters // 2, 1), args.repeats)
        for k in steps:
            print(f"fit_batch {k:30s} {med[k]:9.4f} +-{spr[k]:6.4f}")
    print("rows on which ours is slower than the torch composition:", lost or "none")


if __name__ == "__main__":
    main()
