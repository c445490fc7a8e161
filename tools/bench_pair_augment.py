#!/usr/bin/env python3
"""Paired affine augmentation: the two-plane kernel with noise beside the same result composed from torch ops on the
device (needs an MI355X).

    python tools/bench_pair_augment.py [--iters 20] [--repeats 7] [--no-step]
    MPGAN_LIB_PATH=.../libmpgan_hip_dev.so python tools/bench_pair_augment.py --tiles      # every tile of the dev build
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_pair_augment.py --loop 30    # kernel durations
    python tools/bench_pair_augment.py --deform                                           # the elastic / intensity kernel

Rows: (4, 1, 128, 128, 128) and (16, 1, 256, 256), mode "border", one fixed draw with rotate 0.4 rad on every axis, scale
0.15, shift 0.05 and noise on t1w.  "kernel" is ops.affine_warp into preallocated outputs (the launch alone),
"function" augment.affine_warp (plus its two allocations).  The torch composition is what one would write without the
kernel, in fp32: F.affine_grid from the normalised theta (converted once, outside the timed window), two F.grid_sample
(bilinear, padding_mode="border", align_corners=True) and the noise add.  Before timing the two paths are compared at
the timed size (fp32 grid arithmetic: within 1e-3).  Each figure: HIP events around `iters` calls after a warm-up, per
call; median of `repeats` windows, spread = max - min of the windows; the windows of the paths alternate in one process.
traffic = the bytes the launch must move (2 reads + 2 writes + 1 noise read per voxel pair = 20 B) and the share of
6.3 TB/s that the kernel figure amounts to.  The last rows time a fit_batch of variant A at the C3 shape (16 x 256^2,
fp32) and at the C5 shape (4 x 128^3, bf16 storage) without and with pair_augment.

--deform: at the same shapes and under the same affine draw, the launch alone of ops.affine_warp, of
ops.deform_warp with an elastic lattice only (elastic 0.3, grid 6) and with elastic + bias field + gamma (0.3 each, bias
grid 4; gain and gamma on t1w), alternating in one process, each with its ratio to the affine launch; then a fit_batch at
the C5 shape without pair_augment, with the affine options and with the affine + deform options.  With the development
build (MPGAN_LIB_PATH) four more rows per shape time what else was built: the 4 x 8 x 32 tile (MPGAN_DBG_DEFORM_TILE=0)
beside the product's 1 x 8 x 32, and the 64-term sum per voxel (MPGAN_DBG_DEFORM_FORM=1) beside the product's row
lattices in LDS (the two forms are first compared at the timed size: within 1e-6)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpgan_amd import augment as A  # noqa: E402
from mpgan_amd import ops  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
OPTIONS = dict(rotate=0.4, scale=0.15, shift=0.05, noise_std=0.1)
SHAPES = (("4x128^3", (4, 1, 128, 128, 128)), ("16x256^2", (16, 1, 256, 256)))
TILES = ((0, "4x8x32"), (1, "1x8x32"), (2, "1x1x256"), (3, "1x16x16"), (4, "4x8x8"), (5, "8x4x32"), (6, "1x4x64"),
         (7, "4x4x64"), (8, "1x2x128"))


def normalised_theta(theta, spatial):
    """(A | t) in (d, h, w) voxel indices -> F.affine_grid's theta (align_corners=True): (B, 3, 4) in (x, y, z) order,
    (B, 2, 3) for an image."""
    B, nd = theta.shape[0], len(spatial)
    th = theta.view(B, 3, 4)[:, 3 - nd:, :]
    A_, t = th[:, :, 3 - nd:3], th[:, :, 3]
    half = (torch.tensor(spatial, dtype=torch.float64, device=theta.device) - 1.0) / 2.0          # p = half * (pn + 1)
    An = A_ * half[None, None, :] / half[None, :, None]
    tn = ((A_ * half[None, None, :]).sum(2) + t - half[None, :]) / half[None, :]
    out = torch.cat([An, tn[:, :, None]], 2)
    return out.flip(1)[:, :, list(range(nd - 1, -1, -1)) + [nd]].float().contiguous()


def composed(t1w, t2w, theta_n, noise, sigma):
    grid = F.affine_grid(theta_n, list(t1w.shape), align_corners=True)
    y1 = F.grid_sample(t1w, grid, mode="bilinear", padding_mode="border", align_corners=True)
    y2 = F.grid_sample(t2w, grid, mode="bilinear", padding_mode="border", align_corners=True)
    return y1 + sigma[:, 0].view(-1, *[1] * (t1w.dim() - 1)) * noise, y2


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


def make_case(shape):
    g = torch.Generator().manual_seed(2)
    t1w = (torch.rand(*shape, generator=g) * 2 - 1).cuda()
    t2w = (torch.rand(*shape, generator=g) * 2 - 1).cuda()
    gen = torch.Generator(device="cuda").manual_seed(3)
    p = A.sample_affine_params(shape[0], shape[2:], generator=gen, device="cuda", **OPTIONS)
    noise = torch.randn(shape, generator=gen, device="cuda")
    return t1w, t2w, p, noise


def kernel_call(t1w, t2w, p, noise):
    y1, y2 = torch.empty_like(t1w), torch.empty_like(t2w)
    return lambda: ops.affine_warp(t1w, t2w, p.theta, ops.WARP_BORDER, -1.0, -1.0, noise, None, p.sigma, y1, y2)


def loop(n):
    """The launch alone, preallocated buffers: under `rocprofv3 --kernel-trace --stats` the trace holds n launches per
    shape; the shapes differ in their grid sizes."""
    for label, shape in SHAPES:
        call = kernel_call(*make_case(shape))
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        print(f"{label}: {n} two-plane launches with noise")


def tiles(iters, repeats):
    """Every tile of the development build (MPGAN_DBG_WARP_TILE), alternating in one process."""
    print(f"ms per launch by tile: median of {repeats} windows x {iters} calls (+- = max - min)")
    for label, shape in SHAPES:
        call = kernel_call(*make_case(shape))

        def with_tile(k):
            def run():
                os.environ["MPGAN_DBG_WARP_TILE"] = str(k)
                call()
            return run

        med, spr = measure({name: with_tile(k) for k, name in TILES}, iters, repeats)
        os.environ.pop("MPGAN_DBG_WARP_TILE", None)
        for _, name in TILES:
            print(f"{label:10s} tile {name:8s} {med[name]:9.4f} +-{spr[name]:6.4f}")


DEFORM = dict(elastic=0.3, bias_field=0.3, gamma=0.3)


def deform_call(t1w, t2w, p, noise, q, intensity, switch=None):
    y1, y2 = torch.empty_like(t1w), torch.empty_like(t2w)
    pad = lambda t, ctrl: t if t is None or t1w.dim() == 5 else (
        torch.cat([torch.zeros_like(t[:, :1]), t], 1).unsqueeze(2) if ctrl else t.unsqueeze(1)).contiguous()
    ctrl, gain = pad(q.ctrl, True), pad(q.gain, False) if intensity else None
    gamma = q.gamma if intensity else None

    def run():
        if switch is not None:
            os.environ[switch[0]] = switch[1]
        ops.deform_warp(t1w, t2w, p.theta, ctrl, gain, 1, gamma, -1.0, 1.0, ops.WARP_BORDER, -1.0, -1.0, noise, None,
                        p.sigma, y1, y2)
        if switch is not None:
            os.environ.pop(switch[0])
        return y1, y2
    return run


def deform(iters, repeats, no_step):
    dev = "dev" in os.path.basename(os.environ.get("MPGAN_LIB_PATH", ""))
    print(f"ms per launch: median of {repeats} windows x {iters} calls (+- = max - min); ratio = to the affine launch")
    for label, shape in SHAPES:
        t1w, t2w, p, noise = make_case(shape)
        q = A.sample_deform_params(shape[0], shape[2:], generator=torch.Generator(device="cuda").manual_seed(4),
                                   device="cuda", **DEFORM)
        paths = {"affine": kernel_call(t1w, t2w, p, noise), "elastic": deform_call(t1w, t2w, p, noise, q, False),
                 "elastic + bias + gamma": deform_call(t1w, t2w, p, noise, q, True)}
        if dev:
            tile, form = ("MPGAN_DBG_DEFORM_TILE", "0"), ("MPGAN_DBG_DEFORM_FORM", "1")
            paths["elastic, tile 4x8x32"] = deform_call(t1w, t2w, p, noise, q, False, tile)
            paths["elastic + bias + gamma, tile 4x8x32"] = deform_call(t1w, t2w, p, noise, q, True, tile)
            paths["elastic, 64 terms per voxel"] = deform_call(t1w, t2w, p, noise, q, False, form)
            paths["elastic + bias + gamma, 64 terms per voxel"] = deform_call(t1w, t2w, p, noise, q, True, form)
            for a, b in zip(paths["elastic + bias + gamma"](), paths["elastic + bias + gamma, 64 terms per voxel"]()):
                if not float((a - b).abs().max()) <= 1e-6:
                    raise SystemExit(f"{label}: the two forms disagree by {float((a - b).abs().max()):.3e}")
        med, spr = measure(paths, iters, repeats)
        for k in paths:
            print(f"{label:10s} {k:44s} {med[k]:9.4f} +-{spr[k]:6.4f}   ratio {med[k] / med['affine']:5.2f}")
        del t1w, t2w, noise, paths
        torch.cuda.empty_cache()
    if not no_step:
        from mpgan_amd.gan import GAN
        spatial = (128, 128, 128)
        g = torch.Generator().manual_seed(6)
        batch = {k: (torch.rand(4, 1, *spatial, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}
        steps = {}
        for name, opt in (("None", None), ("affine", OPTIONS), ("affine + deform", dict(OPTIONS, **DEFORM))):
            torch.manual_seed(0)
            m = GAN(1, *spatial, dimensions=3, pair_augment=opt, storage_dtype="bf16")
            opts, _ = m.configure_optimizers()
            steps[f"C5 4x128^3 bf16 pair_augment={name}"] = (lambda m=m, opts=opts: m.fit_batch(batch, 0, opts))
        med, spr = measure(steps, max(iters // 2, 1), repeats)
        for k in steps:
            print(f"fit_batch {k:46s} {med[k]:9.4f} +-{spr[k]:6.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="skip the fit_batch rows")
    ap.add_argument("--loop", type=int, default=0, metavar="N", help="only run N launches per shape (for a kernel trace)")
    ap.add_argument("--tiles", action="store_true", help="time every tile of the development build instead")
    ap.add_argument("--deform", action="store_true", help="time the elastic / intensity kernel beside the affine one instead")
    args = ap.parse_args()
    if args.deform:
        return deform(args.iters, args.repeats, args.no_step)
    if args.loop:
        return loop(args.loop)
    if args.tiles:
        return tiles(args.iters, args.repeats)
    print(f"ms per call: median of {args.repeats} windows x {args.iters} calls (+- = max - min)")
    print(f"{'row':10s} {'kernel':>16s} {'function':>16s} {'torch':>16s} {'ratio':>6s} {'traffic':>9s} {'of HBM':>7s}")
    for label, shape in SHAPES:
        t1w, t2w, p, noise = make_case(shape)
        theta_n = normalised_theta(p.theta, shape[2:])
        ours = kernel_call(t1w, t2w, p, noise)
        fn = lambda: A.affine_warp(t1w, p.theta, t2w, mode="border", noise=noise, sigma=p.sigma)
        torch_ops = lambda: composed(t1w, t2w, theta_n, noise, p.sigma)
        for a, b in zip(fn(), torch_ops()):
            if float((a - b).abs().max()) > 1e-3:
                raise SystemExit(f"{label}: the two paths disagree by {float((a - b).abs().max()):.3e}")
        med, spr = measure({"kernel": ours, "function": fn, "torch": torch_ops}, args.iters, args.repeats)
        traffic = 20 * t1w.numel()
        share = traffic / (med["kernel"] * 1e-3) / HBM_BYTES_PER_S
        print(f"{label:10s} {med['kernel']:9.4f} +-{spr['kernel']:6.4f} {med['function']:9.4f} +-{spr['function']:6.4f} "
              f"{med['torch']:9.4f} +-{spr['torch']:6.4f} {med['torch'] / med['kernel']:6.1f} {traffic / 1e6:7.1f}MB {share:7.3f}")
        del t1w, t2w, noise
        torch.cuda.empty_cache()
    if not args.no_step:
        from mpgan_amd.gan import GAN
        for label, bs, spatial, kw in (("C3 16x256^2 f32", 16, (256, 256), {}),
                                       ("C5 4x128^3 bf16", 4, (128, 128, 128), {"storage_dtype": "bf16"})):
            g = torch.Generator().manual_seed(6)
            batch = {k: (torch.rand(bs, 1, *spatial, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}
            steps = {}
            for name, opt in (("None", None), ("on", OPTIONS)):
                torch.manual_seed(0)
                m = GAN(1, *spatial, dimensions=len(spatial), pair_augment=opt, **kw)
                opts, _ = m.configure_optimizers()
                steps[f"{label} pair_augment={name}"] = (lambda m=m, opts=opts, batch=batch: m.fit_batch(batch, 0, opts))
            med, spr = measure(steps, max(args.iters // 2, 1), args.repeats)
            for k in steps:
                print(f"fit_batch {k:40s} {med[k]:9.4f} +-{spr[k]:6.4f}")
            del steps, batch
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
