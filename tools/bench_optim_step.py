#!/usr/bin/env python3
"""The optimiser step with and without its extras (needs an MI355X).

    python tools/bench_optim_step.py [--iters 20] [--repeats 21]

Times `opt_g.step()` and `opt_d.step()` of variant A at the C3 shape (16 x 256^2, fp32) and the C5 shape (4 x 128^3, bf16
storage) in four configurations of FusedAdam:
    plain        the one mpgan_adam_step launch (the default)
    measure      measure_grad_norm=True: mpgan_grad_norm (two launches) + mpgan_adam_step_ex
    clip         max_grad_norm=1.0: the same launches, the step reads the coefficient from the device
    clip+ema     ... and (generator only) the weight EMA inside the step + the mpgan_ema_buffers launch
The gradients are those of one real fit_batch.  Each figure: HIP events around `iters` calls after a warm-up, per call;
median of `repeats` windows (+- = max - min); the windows of the configurations alternate in one process.  floor = the
bytes the launches must move over 6.3 TB/s: 28 B per element for Adam (p, g, m, v read, p, m, v written), 4 more for the
norm's pass over g, 8 more for the EMA (read and written)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12
CONFIGS = (("plain", {}, 28), ("measure", dict(measure_grad_norm=True), 32), ("clip", dict(max_grad_norm=1.0), 32),
           ("clip+ema", dict(max_grad_norm=1.0), 40))


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
        for _ in range(5):
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
    ap.add_argument("--repeats", type=int, default=21)
    args = ap.parse_args()
    if args.repeats < 20:
        raise SystemExit("--repeats: the median is taken over at least 20 windows")
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_step: needs an MI355X (there is no CPU path)")
    from mpgan_amd.gan import GAN, FusedAdam
    print(f"ms per step(): median of {args.repeats} windows x {args.iters} calls (+- = max - min); floor at 6.3 TB/s")
    print(f"{'row':44s} {'elements':>10s} {'ms':>9s} {'+-':>8s} {'floor':>8s}")
    for label, bs, spatial, kw in (("C3 16x256^2 f32", 16, (256, 256), {}),
                                   ("C5 4x128^3 bf16", 4, (128, 128, 128), {"storage_dtype": "bf16"})):
        torch.manual_seed(0)
        gan = GAN(1, *spatial, dimensions=len(spatial), ema_decay=0.999, **kw)
        g = torch.Generator().manual_seed(6)
        batch = {k: (torch.rand(bs, 1, *spatial, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}
        h = gan.hparams
        plain = [FusedAdam(gan.generator, lr=h.g_lr, betas=(h.b1, h.b2)),
                 FusedAdam(gan.discriminator, lr=h.d_lr, betas=(h.b1, h.b2))]
        gan.fit_batch(batch, 0, plain)                       # real gradients in both flat buffers
        for net_name, net, lr in (("opt_g", gan.generator, h.g_lr), ("opt_d", gan.discriminator, h.d_lr)):
            paths, floors = {}, {}
            for name, opts, bytes_per in CONFIGS:
                if name == "clip+ema":
                    if net is not gan.generator:
                        continue
                    opts = dict(opts, ema=gan.generator_ema, ema_decay=0.999)
                opt = FusedAdam(net, lr=lr, betas=(h.b1, h.b2), **opts)
                paths[name] = opt.step
                floors[name] = bytes_per * net.store.flat.numel() / HBM_BYTES_PER_S * 1e3
            med, spr = measure(paths, args.iters, args.repeats)
            for name in paths:
                row = f"{label} {net_name}.step() {name}"
                print(f"{row:44s} {net.store.flat.numel():10d} {med[name]:9.4f} {spr[name]:8.4f} {floors[name]:8.4f}")
        del gan, batch, plain, paths
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
