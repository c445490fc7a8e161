#!/usr/bin/env python3
"""Differentiable augmentation (forward + backward) beside the same composition built from torch index ops on the
device (needs an MI355X).

    python tools/bench_diffaug.py [--iters 20] [--repeats 7] [--no-step]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_diffaug.py --loop 30      # kernel durations

Rows: (4, 1, 128, 128, 128) and (16, 1, 256, 256), policy "color,translation,cutout" and the spatial ops alone, one fixed
draw of the parameters.  The torch composition is the definition of include/mpgan_hip.h in fp32 with autograd: a mean,
the affine colour step, one advanced-indexing gather, a mask and a where.  Before timing the two paths are compared at
the timed size (bit for bit without a colour op).  Each figure: HIP events around `iters` calls after a warm-up, per call;
median of `repeats` windows, spread = max - min of the windows; the windows of the two paths alternate in one process.
floor = the bytes the launches must move (each launch reads its input once, the apply launches write their output once)
over 6.3 TB/s.  The last rows time a fit_batch of variant A at the C3 shape (16 x 256^2, fp32) and at the C5 shape
(4 x 128^3, bf16 storage) without and with diff_augment="color,translation,cutout"."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpgan_amd import augment as A  # noqa: E402

POLICY = "color,translation,cutout"
HBM_BYTES_PER_S = 6.3e12


def composed(x, p, ops_mask, fill):
    B = x.shape[0]
    S = (1,) * (5 - x.dim()) + tuple(x.shape[2:])
    xs = x.reshape(B, *S)
    u = xs
    if ops_mask & (A.BRIGHTNESS | A.CONTRAST):
        b, c = p.color[:, 0].view(B, 1, 1, 1), p.color[:, 1].view(B, 1, 1, 1)
        m = xs.mean(dim=(1, 2, 3), keepdim=True)
        u = c * (xs - m) + m + b
    geom = p.geom.long()
    idx, inside, inbox = [], [], []
    for k in range(3):
        q = torch.arange(S[k], device=x.device)[None, :]
        t = geom[:, k, None] if ops_mask & A.TRANSLATION else torch.zeros(B, 1, dtype=torch.long, device=x.device)
        src = q + t
        inside.append((src >= 0) & (src < S[k]))
        idx.append(src.clamp(0, S[k] - 1))
        if ops_mask & A.CUTOUT:
            inbox.append((q >= geom[:, 3 + k, None]) & (q < geom[:, 3 + k, None] + geom[:, 6 + k, None]))
        else:
            inbox.append(torch.zeros(B, S[k], dtype=torch.bool, device=x.device))
    v = lambda a, k: a.view(B, *[S[k] if j == k else 1 for j in range(3)])
    keep = (v(inside[0], 0) & v(inside[1], 1) & v(inside[2], 2)) & ~(v(inbox[0], 0) & v(inbox[1], 1) & v(inbox[2], 2))
    bi = torch.arange(B, device=x.device).view(B, 1, 1, 1)
    moved = u[bi, v(idx[0], 0), v(idx[1], 1), v(idx[2], 2)]
    return torch.where(keep, moved, torch.full_like(moved, fill)).reshape(x.shape)


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


def floor_ms(numel, ops_mask):
    """Forward + backward: the apply launches read and write numel floats each, the sum launches (contrast) read them."""
    launches_bytes = 2 * (8 * numel) + (2 * (4 * numel) if ops_mask & A.CONTRAST else 0)
    return launches_bytes / HBM_BYTES_PER_S * 1e3


SHAPES = (("4x128^3", (4, 1, 128, 128, 128)), ("16x256^2", (16, 1, 256, 256)))


def make_case(shape):
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(*shape, generator=g) * 2 - 0.7).cuda()
    gy = (torch.rand(*shape, generator=g) - 0.4).cuda()
    p = A.sample_params(shape[0], shape[2:], POLICY, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    return x, gy, p


def loop(n):
    """The launches alone, preallocated buffers: under `rocprofv3 --kernel-trace --stats` the trace holds, per shape, n
    forward and n backward passes of two launches each (sum, apply); the shapes differ in their grid sizes."""
    from mpgan_amd import ops
    for label, shape in SHAPES:
        x, gy, p = make_case(shape)
        ws = torch.empty(ops.diffaug_workspace(shape[0], shape[2:]) // 8, dtype=torch.float64, device="cuda")
        y, gx = torch.empty_like(x), torch.empty_like(x)
        for _ in range(n):
            ops.diffaug_forward(x, p.ops, p.color, p.geom, -1.0, ws, y)
            ops.diffaug_backward(gy, p.ops, p.color, p.geom, ws, gx)
        torch.cuda.synchronize()
        print(f"{label}: {n} forward + backward passes, policy {POLICY!r}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the fit_batch rows")
    ap.add_argument("--loop", type=int, default=0, metavar="N",
                    help="only run N forward + backward calls per shape through ops.diffaug_* (for a kernel trace)")
    args = ap.parse_args()
    if args.loop:
        return loop(args.loop)
    print(f"ms per forward + backward: median of {args.repeats} windows x {args.iters} calls (+- = max - min)")
    print(f"{'row':34s} {'kernels':>16s} {'floor':>8s} {'torch':>16s} {'ratio':>6s}")
    for label, shape in SHAPES:
        x, gy, p = make_case(shape)
        x.requires_grad_(True)
        for name, use_color in (("color,translation,cutout", True), ("translation,cutout", False)):
            mask = p.ops if use_color else p.ops & ~(A.BRIGHTNESS | A.CONTRAST)

            def ours():
                return torch.autograd.grad(A.diff_augment(x, p, color=use_color, fill=-1.0), x, gy)[0]

            def torch_ops():
                return torch.autograd.grad(composed(x, p, mask, -1.0), x, gy)[0]

            y_k, y_t = A.diff_augment(x, p, color=use_color, fill=-1.0).detach(), composed(x, p, mask, -1.0).detach()
            g_k, g_t = ours(), torch_ops()
            if use_color:
                ok = float((y_k - y_t).abs().max()) <= 1e-5 and float((g_k - g_t).abs().max()) <= 1e-5
            else:
                ok = torch.equal(y_k, y_t) and torch.equal(g_k, g_t)
            if not ok:
                raise SystemExit(f"{label} {name}: the two paths disagree")
            del y_k, y_t, g_k, g_t
            med, spr = measure({"kernels": ours, "torch": torch_ops}, args.iters, args.repeats)
            row = f"{label} {name}"
            print(f"{row:34s} {med['kernels']:9.4f} +-{spr['kernels']:6.4f} {floor_ms(x.numel(), mask):8.4f} "
                  f"{med['torch']:9.4f} +-{spr['torch']:6.4f} {med['torch'] / med['kernels']:6.1f}")
        del x, gy
        torch.cuda.empty_cache()
    if not args.no_step:
        from mpgan_amd.gan import GAN
        for label, bs, spatial, kw in (("C3 16x256^2 f32", 16, (256, 256), {}),
                                       ("C5 4x128^3 bf16", 4, (128, 128, 128), {"storage_dtype": "bf16"})):
            g = torch.Generator().manual_seed(6)
            batch = {k: (torch.rand(bs, 1, *spatial, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}
            steps = {}
            for policy in ("", POLICY):
                torch.manual_seed(0)
                m = GAN(1, *spatial, dimensions=len(spatial), diff_augment=policy, **kw)
                opts, _ = m.configure_optimizers()
                steps[f"{label} diff_augment={policy!r}"] = (lambda m=m, opts=opts, batch=batch: m.fit_batch(batch, 0, opts))
            med, spr = measure(steps, max(args.iters // 2, 1), args.repeats)
            for k in steps:
                print(f"fit_batch {k:56s} {med[k]:9.4f} +-{spr[k]:6.4f}")
            del steps, batch
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
