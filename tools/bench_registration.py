#!/usr/bin/env python3
"""The affine warp's gradient in theta and a whole registration, timed on the device (needs an MI355X).

    python tools/bench_registration.py [--warmup 20] [--iters 100]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_registration.py --loop 50        # kernel durations

Rows, at (4, 1, 128, 128, 128) and (16, 1, 256, 256), one draw of augment.DEFAULT_AFFINE for theta:
  theta-gradient   ops.affine_warp_backward_theta, one plane (two launches; the workspace is allocated inside the call)
  forward          ops.affine_warp, one plane, mode constant, on preallocated buffers, the same theta
  torch            the backward to theta of torch's own composition on the same device: a voxel grid from theta,
                   grid_sample(padding_mode="zeros", align_corners=True), autograd.grad in theta (fp32 images, fp64 theta
                   cast to fp32 for the grid; the forward is built once, the timed call is the backward alone).  Before
                   timing, the kernel is compared with the same composition in fp64 at the timed size.
Then one whole register_affine of a 4 x 128^3 pair (the phantom of the tests, enlarged), levels (4, 2, 1), iterations
(40, 20, 10): wall time of the call between two device synchronisations, and beside it the device time of the same
number of warp + theta-gradient + MI launches alone, which is what the loop costs without its small torch launches.
Each per-call figure: HIP events around `iters` calls after `warmup` calls."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpgan_amd import augment as A  # noqa: E402
from mpgan_amd import losses, ops  # noqa: E402
from mpgan_amd import registration as reg  # noqa: E402

SHAPES = (("4x128^3", (4, 1, 128, 128, 128)), ("16x256^2", (16, 1, 256, 256)))


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def torch_theta_backward(x, theta, gy, dtype=torch.float32):
    """A closure running the backward to theta of grid_sample's composition in `dtype` (retain_graph: the forward is built
    once)."""
    B, S = x.shape[0], (1,) * (5 - x.dim()) + tuple(x.shape[2:])
    x, gy = x.to(dtype), gy.to(dtype)
    th = theta.clone().requires_grad_(True)
    p = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=dtype, device=x.device) for s in S], indexing="ij")
                    + (torch.ones(S, dtype=dtype, device=x.device),), dim=-1)
    c = torch.einsum("nkj,dhwj->ndhwk", th.reshape(B, 3, 4).to(dtype), p)
    if S[0] == 1:
        norm = torch.tensor([S[2] - 1, S[1] - 1], dtype=dtype, device=x.device)
        y = torch.nn.functional.grid_sample(x, 2.0 * c[:, 0, :, :, [2, 1]] / norm - 1.0, mode="bilinear",
                                            padding_mode="zeros", align_corners=True)
    else:
        norm = torch.tensor([S[2] - 1, S[1] - 1, S[0] - 1], dtype=dtype, device=x.device)
        y = torch.nn.functional.grid_sample(x, 2.0 * c[..., [2, 1, 0]] / norm - 1.0, mode="bilinear", padding_mode="zeros",
                                            align_corners=True)
    return lambda: torch.autograd.grad(y, th, gy, retain_graph=True)[0]


def phantom_pair(n, size, seed=0):
    """n pairs of the tests' phantom at `size` (tests/registration_ref.py), the moving image under a small rigid map."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import affine_ref as R
    import registration_ref as G
    moving, fixed = [], []
    rng = np.random.default_rng(seed)
    for s in range(n):
        t1, t2 = G.phantom(seed + s, size)
        theta = torch.from_numpy(R.theta_from_params(rng.uniform(-0.1, 0.1, 3), 1.0, rng.uniform(-4, 4, 3), in_size=size)[None]).cuda()
        m = A.affine_warp(torch.from_numpy(t1.astype(np.float32))[None, None].cuda(), reg.invert_theta(theta), mode="constant",
                          fill=-1.0)
        moving.append(m)
        fixed.append(torch.from_numpy(t2.astype(np.float32))[None, None].cuda())
    return torch.cat(moving).contiguous(), torch.cat(fixed).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--loop", type=int, default=0, help="only run the two launches this many times per shape (for a profiler)")
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}; {args.warmup} warm-up + {args.iters} timed calls per figure, HIP events")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for label, shape in SHAPES:
        n, spatial = shape[0], shape[2:]
        x = torch.rand(shape, device="cuda", generator=gen) * 2 - 1
        gy = torch.rand(shape, device="cuda", generator=gen) * 2 - 1
        y = torch.empty_like(x)
        theta = A.sample_affine_params(n, spatial, generator=gen, device="cuda", **A.DEFAULT_AFFINE).theta
        gtheta = torch.empty((n, 12), dtype=torch.float64, device="cuda")
        ours = lambda: ops.affine_warp_backward_theta(x, None, gy, None, theta, ops.WARP_CONSTANT, 0.0, 0.0, gtheta)
        fwd = lambda: ops.affine_warp(x, None, theta, ops.WARP_CONSTANT, 0.0, 0.0, None, None, None, y, None)
        if args.loop:                                  # for rocprofv3 --kernel-trace --stats: the launches alone
            for _ in range(args.loop):
                ours()
                fwd()
            torch.cuda.synchronize()
            continue
        ref_fn = torch_theta_backward(x, theta, gy)
        rows = slice(4, 12) if len(spatial) == 2 else slice(0, 12)      # grid_sample has no d coordinate in 2-D
        got, want = ours().clone()[:, rows], torch_theta_backward(x, theta, gy, torch.float64)()[:, rows]
        scale = float(want.abs().max())
        print(f"{label}: max |ours - torch fp64| / max |torch fp64| = {float((got - want).abs().max()) / scale:.2e}; "
              f"torch fp32 against torch fp64: {float((ref_fn()[:, rows] - want).abs().max()) / scale:.2e}")
        t_ours, t_fwd, t_ref = (timed(f, args.warmup, args.iters) for f in (ours, fwd, ref_fn))
        print(f"{label}: theta-gradient {t_ours * 1e3:8.1f} us   forward {t_fwd * 1e3:8.1f} us   ratio {t_ours / t_fwd:5.2f}   "
              f"torch grid_sample backward to theta {t_ref * 1e3:8.1f} us ({t_ref / t_ours:5.1f} x)")
    if args.loop:
        return
    # one whole registration
    levels, iters, lr = (4, 2, 1), (40, 20, 10), (0.02, 0.01, 0.005)
    moving, fixed = phantom_pair(4, (128, 128, 128))
    reg.register_affine(moving, fixed, levels=levels, iters=(2, 2, 2), lr=lr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = reg.register_affine(moving, fixed, levels=levels, iters=iters, lr=lr)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    hist = res.history.cpu().numpy()
    print(f"register_affine 4x128^3 rigid, levels {levels}, iters {iters}: wall {wall * 1e3:.1f} ms "
          f"({wall * 1e3 / sum(iters):.2f} ms per iteration); -MI {hist[0].mean():.4f} -> {hist[-1].mean():.4f}")
    kernel_ms = 0.0
    for L, steps in zip(levels, iters):
        m_lv, f_lv = reg._pooled(moving, L), reg._pooled(fixed, L)
        th = reg.level_theta(res.theta, L, moving.shape[2:])

        def step():
            t = th.clone().requires_grad_(True)
            item = losses.global_mutual_information_loss(A.diff_affine_warp(m_lv, t, fill=-1.0), f_lv, num_bins=23,
                                                         reduction="none", value_range=(-1.0, 1.0))
            torch.autograd.grad(item.sum(), t)

        per = timed(step, 5, 20)
        kernel_ms += per * steps
        print(f"  level {L}: warp + MI forward and backward to theta {per * 1e3:8.1f} us per iteration x {steps}")
    print(f"  warp + MI + theta-gradient alone: {kernel_ms:.1f} ms of the {wall * 1e3:.1f} ms wall "
          f"(the rest: the parameter arithmetic's small torch launches and Adam)")


if __name__ == "__main__":
    main()
