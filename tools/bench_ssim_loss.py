#!/usr/bin/env python3
"""SSIMLoss (forward + backward) beside the torch composition on the device (needs an MI355X).

    python tools/bench_ssim_loss.py [--iters 10] [--repeats 7] [--no-step]

Rows: (4, 1, 128, 128, 128) and (16, 1, 256, 256), value range (-1, 1), gradient for the first tensor (the generator's
case) and for both.  The torch composition is tests/ssim_loss_ref.py run on the device in fp32 with autograd: five
box filters (conv2d / conv3d with a ones kernel) and their graph.  Each figure: HIP events around `iters` calls after
a warm-up, per call; median of `repeats` windows, spread = max - min of the windows; the windows of the two paths
alternate in one process.  Peak memory is torch.cuda.max_memory_allocated over one call, above what the inputs hold.
The last rows time a fit_batch of variant A at the C3 shape (16 x 256^2, fp32) and at the C5 shape (4 x 128^3, bf16
storage) with ssim_weight 0 and 0.5."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssim_loss_ref  # noqa: E402
from mpgan_amd import losses  # noqa: E402

RANGE = (-1.0, 1.0)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the fit_batch rows")
    args = ap.parse_args()
    print(f"ms per forward + backward: median of {args.repeats} windows x {args.iters} calls (+- = max - min)")
    print(f"{'row':30s} {'kernels':>16s} {'peak MB':>8s} {'torch':>16s} {'peak MB':>8s} {'ratio':>6s}")
    lost = []
    for label, shape in (("4x128^3", (4, 1, 128, 128, 128)), ("16x256^2", (16, 1, 256, 256))):
        pred, target = (x.cuda() for x in ssim_loss_ref.structured_pair(shape, seed=1))
        for both in (False, True):
            p = pred.clone().requires_grad_(True)
            t = target.clone().requires_grad_(both)
            wrt = (p, t) if both else (p,)

            def ours():
                return torch.autograd.grad(losses.ssim_loss(p, t, RANGE), wrt)

            def composed():
                return torch.autograd.grad(ssim_loss_ref.loss(p, t, RANGE, dtype=torch.float32), wrt)

            go, gt = ours(), composed()
            scale = float(gt[0].abs().max())
            if float((go[0] - gt[0]).abs().max()) > 1e-3 * scale:
                raise SystemExit(f"{label}: the two paths disagree")
            del go, gt
            paths = {"kernels": ours, "torch": composed}
            med, spr = measure(paths, args.iters, args.repeats)
            mem = {k: peak_mb(fn) for k, fn in paths.items()}
            name = f"{label} grad {'both' if both else 'pred'}"
            print(f"{name:30s} {med['kernels']:9.4f} +-{spr['kernels']:6.4f} {mem['kernels']:8.1f} "
                  f"{med['torch']:9.4f} +-{spr['torch']:6.4f} {mem['torch']:8.1f} {med['torch'] / med['kernels']:6.1f}")
            if med["kernels"] > med["torch"]:
                lost.append(name)
        del pred, target
        torch.cuda.empty_cache()
    if not args.no_step:
        from mpgan_amd.gan import GAN
        for label, bs, spatial, kw in (("C3 16x256^2 f32", 16, (256, 256), {}),
                                       ("C5 4x128^3 bf16", 4, (128, 128, 128), {"storage_dtype": "bf16"})):
            g = torch.Generator().manual_seed(6)
            batch = {k: (torch.rand(bs, 1, *spatial, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}
            steps = {}
            for w in (0.0, 0.5):
                torch.manual_seed(0)
                m = GAN(1, *spatial, dimensions=len(spatial), ssim_weight=w, **kw)
                opts, _ = m.configure_optimizers()
                steps[f"{label} ssim_weight {w}"] = (lambda m=m, opts=opts, batch=batch: m.fit_batch(batch, 0, opts))
            med, spr = measure(steps, args.iters, args.repeats)
            for k in steps:
                print(f"fit_batch {k:30s} {med[k]:9.4f} +-{spr[k]:6.4f}")
            del steps, batch
            torch.cuda.empty_cache()
    print("rows on which the kernel path is slower than the torch composition:", lost or "none")
    sys.exit(1 if lost else 0)


if __name__ == "__main__":
    main()
