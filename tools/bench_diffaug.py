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
(4 x 128^3, bf16 storage) without diff_augment, with "color,translation,cutout" and with "color,affine,translation,cutout".

The affine rows time the warp's backward launch alone, ops.affine_warp_backward on preallocated buffers,
at the same two shapes under two sets of maps: one draw of augment.DEFAULT_AFFINE, and the worst supported map (zoom 2
with a rotation about every axis: a reach of about 3.4 voxels).  Beside it: the backward of torch's
affine_grid + grid_sample(padding_mode="zeros", align_corners=True) for the same maps on the same device, an atomic
scatter (the forward is run once, outside the timed window).  floor = 8 bytes per voxel (g_y read once, g_x written once)
over 6.3 TB/s.  Before timing the two gradients are compared at the timed size."""
import argparse
import math
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
POLICY_AFFINE = "color,affine,translation,cutout"


def zoom_theta(n, spatial, angles=(0.3, -0.5, 0.7), scale=2.0):
    """(n, 12) float64 on the device: A = R / scale about the centre, R = R_d R_h R_w (2-D: the in-plane angle alone)."""
    ad, ah, aw = angles if len(spatial) == 3 else (angles[0], 0.0, 0.0)
    c, s = math.cos, math.sin
    Rd = torch.tensor([[1, 0, 0], [0, c(ad), -s(ad)], [0, s(ad), c(ad)]], dtype=torch.float64)
    Rh = torch.tensor([[c(ah), 0, s(ah)], [0, 1, 0], [-s(ah), 0, c(ah)]], dtype=torch.float64)
    Rw = torch.tensor([[c(aw), -s(aw), 0], [s(aw), c(aw), 0], [0, 0, 1]], dtype=torch.float64)
    A_ = Rd @ Rh @ Rw / scale
    ctr = (torch.tensor((1,) * (3 - len(spatial)) + tuple(spatial), dtype=torch.float64) - 1.0) / 2.0
    if len(spatial) == 2:
        A_[0], A_[:, 0] = torch.tensor([1.0, 0, 0], dtype=torch.float64), torch.tensor([1.0, 0, 0], dtype=torch.float64)
    theta = torch.cat([A_, (ctr - A_ @ ctr)[:, None]], 1).reshape(1, 12)
    return theta.repeat(n, 1).cuda()


def torch_grid(theta, shape):
    """The grid of F.grid_sample(align_corners=True) that samples where theta (voxel indices, (d, h, w) order) does:
    u_in = N^-1 (A N (u_out + 1) + t) - 1 with N = diag((S - 1) / 2), rows and columns reversed to (x, y, z)."""
    import torch.nn.functional as F
    nd = len(shape) - 2
    S = torch.tensor(shape[2:], dtype=torch.float64, device=theta.device)
    th = theta.view(-1, 3, 4)[:, 3 - nd:, :]
    A_, t = th[:, :, 3 - nd:3], th[:, :, 3]
    N = torch.diag((S - 1.0) / 2.0)
    Ni = torch.diag(2.0 / (S - 1.0))
    An = Ni @ A_ @ N
    tn = (Ni @ (A_ @ (N @ torch.ones(nd, dtype=torch.float64, device=theta.device)) + t).unsqueeze(-1)).squeeze(-1) - 1.0
    mat = torch.cat([An.flip(1, 2), tn.flip(1).unsqueeze(-1)], 2).to(torch.float32)
    return F.affine_grid(mat, list(shape), align_corners=True)


def affine_rows(iters, repeats):
    import torch.nn.functional as F
    from mpgan_amd import ops
    print(f"ms per backward launch: median of {repeats} windows x {iters} calls (+- = max - min)")
    print(f"{'row':34s} {'gather kernel':>16s} {'floor':>8s} {'torch scatter':>16s} {'ratio':>6s}")
    for label, shape in SHAPES:
        n, spatial = shape[0], shape[2:]
        g = torch.Generator().manual_seed(2)
        x = (torch.rand(*shape, generator=g) * 2 - 1).cuda().requires_grad_(True)
        gy = (torch.rand(*shape, generator=g) - 0.4).cuda()
        drawn = A.sample_affine_params(n, spatial, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda",
                                       **A.DEFAULT_AFFINE).theta
        for name, theta in (("DEFAULT_AFFINE draw", drawn), ("zoom 2 + rotation", zoom_theta(n, spatial))):
            gx = torch.empty_like(gy)
            y_t = F.grid_sample(x, torch_grid(theta, shape), mode="bilinear", padding_mode="zeros", align_corners=True)

            def ours():
                return ops.affine_warp_backward(gy, theta, ops.WARP_CONSTANT, gx)

            def torch_ops():
                return torch.autograd.grad(y_t, x, gy, retain_graph=True)[0]

            gap = float((ours() - torch_ops()).abs().max())
            if not gap <= 1e-3:                                    # (the grid is fp32: coordinates differ by ~1e-5 voxels)
                raise SystemExit(f"{label} {name}: the two gradients disagree by {gap}")
            med, spr = measure({"kernels": ours, "torch": torch_ops}, iters, repeats)
            row = f"{label} {name}"
            print(f"{row:34s} {med['kernels']:9.4f} +-{spr['kernels']:6.4f} {8 * gy.numel() / HBM_BYTES_PER_S * 1e3:8.4f} "
                  f"{med['torch']:9.4f} +-{spr['torch']:6.4f} {med['torch'] / med['kernels']:6.2f}   (max gap {gap:.1e})")
            del y_t
        del x, gy
        torch.cuda.empty_cache()


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
        theta = A.sample_affine_params(shape[0], shape[2:], generator=torch.Generator(device="cuda").manual_seed(3),
                                       device="cuda", **A.DEFAULT_AFFINE).theta
        for _ in range(n):
            ops.affine_warp_backward(gy, theta, ops.WARP_CONSTANT, gx)
            ops.affine_warp_backward(gy, zoom_theta(shape[0], shape[2:]), ops.WARP_CONSTANT, gx)
        torch.cuda.synchronize()
        print(f"{label}: {n} forward + backward passes, policy {POLICY!r}; {n} warp backward launches per set of maps")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the fit_batch rows")
    ap.add_argument("--no-affine", action="store_true", help="skip the warp backward rows")
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
    if not args.no_affine:
        affine_rows(args.iters, args.repeats)
    if not args.no_step:
        from mpgan_amd.gan import GAN
        for label, bs, spatial, kw in (("C3 16x256^2 f32", 16, (256, 256), {}),
                                       ("C5 4x128^3 bf16", 4, (128, 128, 128), {"storage_dtype": "bf16"})):
            g = torch.Generator().manual_seed(6)
            batch = {k: (torch.rand(bs, 1, *spatial, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}
            steps = {}
            for policy in ("", POLICY, POLICY_AFFINE):
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
