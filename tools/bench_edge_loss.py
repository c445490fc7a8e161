#!/usr/bin/env python3
"""EdgeLoss (forward + backward) beside the torch composition on the device (needs an MI355X).

    python tools/bench_edge_loss.py [--iters 20] [--repeats 7] [--no-step]

Rows: (4, 1, 128, 128, 128) and (16, 1, 256, 256), eps 1e-6, gradient for the first tensor (the generator's case) and
for both.  Three paths per row:

    kernels   the library's launches alone, through mpgan_amd.ops on preallocated buffers: edge_loss_forward (three
              launches) and one edge_loss_backward per gradient
    autograd  losses.edge_loss + torch.autograd.grad: the same launches plus the autograd node and its allocations
    torch     the composition on the device in fp32 with autograd: replicate pad, conv2d / conv3d with the three
              normalised Sobel filters, square-sum-sqrt, l1_loss (tests/edge_loss_ref.magnitude)

Each figure: HIP events around `iters` calls after a warm-up, per call; median of `repeats` windows, spread = max - min
of the windows; the windows of the paths alternate in one process.  GB/s is the least traffic of the kernels path (the
forward reads both tensors once, a backward reads both and writes one gradient) over its time.  Peak memory is
torch.cuda.max_memory_allocated over one call, above what the inputs hold.  The last rows time a fit_batch of variant A
at the C3 shape (16 x 256^2, fp32) and at the C5 shape (4 x 128^3, bf16 storage) with edge_weight 0 and 0.5.  No figure
is a condition: the exit status is 0 whichever path is faster."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edge_loss_ref  # noqa: E402
from mpgan_amd import losses, ops  # noqa: E402

EPS = 1e-6


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the fit_batch rows")
    args = ap.parse_args()
    print(f"ms per forward + backward: median of {args.repeats} windows x {args.iters} calls (+- = max - min)")
    print(f"{'row':24s} {'kernels':>16s} {'GB/s':>6s} {'autograd':>16s} {'peak MB':>8s} {'torch':>16s} {'peak MB':>8s} "
          f"{'torch/autograd':>14s}")
    lost = []
    for label, shape in (("4x128^3", (4, 1, 128, 128, 128)), ("16x256^2", (16, 1, 256, 256))):
        pred, target = (x.cuda() for x in edge_loss_ref.structured_pair(shape, seed=1))
        spatial, items = tuple(shape[2:]), shape[0] * shape[1]
        ws = torch.empty(ops.edge_loss_workspace(spatial, items) // 8, dtype=torch.float64, device="cuda")
        loss, one = torch.empty((), device="cuda"), torch.ones((), device="cuda")
        grads = [torch.empty_like(pred), torch.empty_like(pred)]
        for both in (False, True):
            p = pred.clone().requires_grad_(True)
            t = target.clone().requires_grad_(both)
            wrt = (p, t) if both else (p,)

            def kernels():
                ops.edge_loss_forward(pred, target, spatial, items, 1, EPS, ws, "mean", loss)
                for k in range(len(wrt)):
                    ops.edge_loss_backward(pred, target, spatial, items, 1, EPS, one, 1.0 / items, k, grads[k])

            def ours():
                return torch.autograd.grad(losses.edge_loss(p, t, EPS), wrt)

            def composed():
                return torch.autograd.grad(F.l1_loss(edge_loss_ref.magnitude(p, EPS, torch.float32),
                                                     edge_loss_ref.magnitude(t, EPS, torch.float32)), wrt)

            go, gt = ours(), composed()
            kernels()
            scale = float(gt[0].abs().max())
            # the two paths round m differently, so a few signs differ next to the kink: compare the bulk
            off = ((go[0] - gt[0]).abs() > 1e-3 * scale).float().mean()
            if float(off) > 1e-3 or not torch.equal(go[0], grads[0]):
                raise SystemExit(f"{label}: the paths disagree ({float(off):.2e} of the entries)")
            del go, gt
            paths = {"kernels": kernels, "autograd": ours, "torch": composed}
            med, spr = measure(paths, args.iters, args.repeats)
            mem = {k: peak_mb(fn) for k, fn in paths.items()}
            gbytes = pred.numel() * 4 * (2 + 3 * len(wrt)) / 1e9
            name = f"{label} grad {'both' if both else 'pred'}"
            print(f"{name:24s} {med['kernels']:9.4f} +-{spr['kernels']:6.4f} {gbytes / med['kernels'] * 1e3:6.0f} "
                  f"{med['autograd']:9.4f} +-{spr['autograd']:6.4f} {mem['autograd']:8.1f} "
                  f"{med['torch']:9.4f} +-{spr['torch']:6.4f} {mem['torch']:8.1f} {med['torch'] / med['autograd']:14.1f}")
            if med["autograd"] > med["torch"]:
                lost.append(name)
        del pred, target, ws, grads
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
                m = GAN(1, *spatial, dimensions=len(spatial), edge_weight=w, **kw)
                opts, _ = m.configure_optimizers()
                steps[f"{label} edge_weight {w}"] = (lambda m=m, opts=opts, batch=batch: m.fit_batch(batch, 0, opts))
            med, spr = measure(steps, max(args.iters // 2, 1), args.repeats)
            for k in steps:
                print(f"fit_batch {k:30s} {med[k]:9.4f} +-{spr[k]:6.4f}")
            del steps, batch
            torch.cuda.empty_cache()
    print("rows on which the autograd path is slower than the torch composition:", lost or "none")


if __name__ == "__main__":
    main()
