#!/usr/bin/env python3
"""The conditional discriminator's first conv (two input planes) beside the unconditional one and beside
what the one-plane entry points can compose for the same result (development aid; needs an MI355X).

    python tools/bench_cond_conv1.py                # the conv1 geometries of C3 (256^2, bs 16) and C5 (128^3, bs 4)
    python tools/bench_cond_conv1.py --config C5    # one of them
    python tools/bench_cond_conv1.py --steps        # also GAN.fit_batch, conditional beside unconditional (child processes)

Rows per geometry, all in one process on the same buffers:
  forward   (a) mpgan_conv2p_forward (fp32 out) and mpgan_conv2p_forward_f32_to_bf16
            (b) the unconditional conv1: mpgan_conv_forward (cin = 1) and mpgan_conv_forward_f32_to_bf16
            (c1) two mpgan_conv_forward cin = 1 launches, the second adding the first's result as `resid`
            (c2) one mpgan_conv_forward cin = 2 launch on an interleaved (N, D, H, W, 2) tensor: the generic form
  wgrad     (a) mpgan_conv2p_backward_weight with dy fp32 and bf16
            (b) mpgan_conv_backward_weight (cin = 1) and mpgan_conv_backward_weight_bf16dy
            (c1) two mpgan_conv_backward_weight cin = 1 launches, one per plane   (c2) one cin = 2 launch, interleaved x
(c1), (c2) give (a)'s fp32 result, so (a) fp32 is what they are compared with.  Each figure: HIP events around `iters`
calls after a warm-up, per call; median of `repeats` windows, spread = max - min of the windows (the method of
tools/bench_disc_eval.py).  Floors: 54 FMA per output on the vector units at 157 TFLOP/s, and the 64-channel tensor
moved once at 8 TB/s.  The last line per geometry says whether (a) beats the faster composition by more than the
spreads; the exit status is 1 if it does not."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
CONFIGS = {"C3": (16, (256, 256), "f32"), "C5": (4, (128, 128, 128), "bf16")}   # batch, spatial, the step's storage
HBM_BYTES_PER_S, VALU_FLOPS = 8e12, 157e12


def timed(fn, iters, repeats, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) / iters)
    return {"ms": statistics.median(windows), "spread": max(windows) - min(windows)}


def kernel_rows(config, iters, repeats):
    import dataclasses
    import torch
    from mpgan_amd import ops
    n, spatial, _ = CONFIGS[config]
    dims = len(spatial)
    t3 = lambda v, fill: (fill,) * (3 - dims) + (v,) * dims
    g2 = ops.ConvGeom(n, (1,) * (3 - dims) + tuple(spatial), 2, 64, t3(3, 1), (1, 1, 1), (0, 0, 0))
    g1 = dataclasses.replace(g2, cin=1)
    torch.manual_seed(0)
    R = lambda *s: torch.rand(*s, device="cuda") - 0.5
    img, cond = R(n, *g2.in_dhw, 1), R(n, *g2.in_dhw, 1)
    inter = torch.cat([img, cond], -1).contiguous()
    w = R(64, 2, *([3] * dims)) * 0.3
    bias = R(64)
    wp2 = ops.pack_weight(w)
    wp_img, wp_cond = ops.pack_weight(w[:, :1].contiguous()), ops.pack_weight(w[:, 1:].contiguous())
    y32, y32b = torch.empty(n, *g2.out_dhw, 64, device="cuda"), torch.empty(n, *g2.out_dhw, 64, device="cuda")
    y16 = torch.empty(n, *g2.out_dhw, 64, device="cuda", dtype=torch.bfloat16)
    rows_bf = ops.conv2p_stats_rows(g2, True)
    part = torch.empty(max(rows_bf, (y16.numel() // 64 + 255) // 256) * 128, device="cuda")
    fwd = {
        "(a) conv2p_forward f32": lambda: ops.conv2p_forward(g2, img, cond, wp2, bias, y32),
        "(a) conv2p_forward bf16 + stats": lambda: ops.conv2p_forward(g2, img, cond, wp2, bias, y16, stats_partials=part),
        "(b) conv_forward cin=1 f32": lambda: ops.conv_forward(g1, img, wp_img, bias, y32),
        "(b) conv_forward_f32_to_bf16 + stats": lambda: ops.conv_forward_f32_to_bf16(g1, img, wp_img, bias, y16, stats_partials=part),
        "(c1) 2 x conv_forward cin=1, resid": lambda: (ops.conv_forward(g1, img, wp_img, bias, y32b),
                                                         ops.conv_forward(g1, cond, wp_cond, None, y32, resid=y32b)),
        "(c2) conv_forward cin=2 interleaved": lambda: ops.conv_forward(g2, inter, wp2, bias, y32),
    }
    out = {"forward": {k: timed(f, iters, repeats) for k, f in fwd.items()}}
    del y32b
    dy32 = y32.copy_(R(*y32.shape))
    dy16 = y16.copy_(dy32)
    dw2, dw1a, dw1b, db = torch.zeros_like(w), torch.zeros_like(w[:, :1]).contiguous(), torch.zeros_like(w[:, :1]).contiguous(), torch.zeros(64, device="cuda")
    ws = torch.empty(max(ops.conv2p_wgrad_workspace(g2), ops.conv_wgrad_workspace(g2), ops.conv_wgrad_workspace(g1),
                         ops.conv_wgrad_workspace_bf16dy(g1)) // 4 + 4, device="cuda")
    wg = {
        "(a) conv2p_backward_weight f32 dy": lambda: ops.conv2p_backward_weight(g2, img, cond, dy32, dw2, ws, beta=1.0, dbias=db),
        "(a) conv2p_backward_weight bf16 dy": lambda: ops.conv2p_backward_weight(g2, img, cond, dy16, dw2, ws, beta=1.0, dbias=db),
        "(b) conv_backward_weight cin=1": lambda: ops.conv_backward_weight(g1, img, dy32, dw1a, ws, beta=1.0, dbias=db),
        "(b) conv_backward_weight_bf16dy": lambda: ops.conv_backward_weight_bf16dy(g1, img, dy16, dw1a, ws, beta=1.0, dbias=db),
        "(c1) 2 x conv_backward_weight cin=1": lambda: (ops.conv_backward_weight(g1, img, dy32, dw1a, ws, beta=1.0, dbias=db),
                                                          ops.conv_backward_weight(g1, cond, dy32, dw1b, ws, beta=1.0)),
        "(c2) conv_backward_weight cin=2 interleaved": lambda: ops.conv_backward_weight(g2, inter, dy32, dw2, ws, beta=1.0, dbias=db),
    }
    out["wgrad"] = {k: timed(f, iters, repeats) for k, f in wg.items()}
    outputs = y32.numel()
    out["floors"] = {"fma_ms": outputs * 54 * 2 / VALU_FLOPS * 1e3, "store_f32_ms": outputs * 4 / HBM_BYTES_PER_S * 1e3,
                     "store_bf16_ms": outputs * 2 / HBM_BYTES_PER_S * 1e3}
    out["labels"] = {"forward f32": ops.conv2p_kernel_name(g2, False), "forward bf16": ops.conv2p_kernel_name(g2, True),
                     "wgrad f32": ops.conv2p_wgrad_kernel_name(g2, False), "wgrad bf16": ops.conv2p_wgrad_kernel_name(g2, True)}
    return out


def step_child(config, conditional, iters, repeats):
    import torch
    from mpgan_amd.gan import GAN
    n, spatial, dtype = CONFIGS[config]
    torch.manual_seed(0)
    gan = GAN(1, *spatial, dimensions=len(spatial), g_lr=1e-6, d_lr=1e-6, storage_dtype=dtype, conditional=conditional)
    with torch.no_grad():                            # as bench.py: keep the huge Linear head out of sigmoid saturation
        gan.discriminator.model_linear[1].weight.mul_(0.02 * (0.4 if len(spatial) == 3 else 1.0))
    gan.train()
    opts, _ = gan.configure_optimizers()
    g = torch.Generator().manual_seed(1234)
    batch = {k: (torch.rand(n, 1, *spatial, generator=g) * 2 - 1).cuda() for k in ("t1w", "t2w")}
    step = [0]

    def one():
        gan.fit_batch(batch, step[0], opts)
        step[0] += 1
    res = timed(one, iters, repeats, warmup=2)
    res["d_loss"] = float(gan.logged["d_loss"])
    print("RESULT " + json.dumps(res), flush=True)


def run_child(config, conditional, iters, repeats):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "cond" if conditional else "plain", "--config", config,
           "--step-iters", str(iters), "--repeats", str(repeats)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    for line in res.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError(f"step child: no result (exit {res.returncode})\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=("C3", "C5", "both"))
    ap.add_argument("--iters", type=int, default=10, help="calls per window")
    ap.add_argument("--step-iters", type=int, default=3, help="training steps per window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--child", default=None, choices=("plain", "cond"))
    a = ap.parse_args()
    if a.child:
        step_child(a.config, a.child == "cond", a.step_iters, a.repeats)
        return 0
    configs = ["C3", "C5"] if a.config == "both" else [a.config]
    steps = {}
    if a.steps:                                      # before this process opens the GPU: one process at a time
        for c in configs:
            steps[c] = {False: [], True: []}
            for _ in range(a.rounds):
                for cond in (False, True):
                    steps[c][cond].append(run_child(c, cond, a.step_iters, a.repeats))
    ok = True
    for c in configs:
        n, spatial, _ = CONFIGS[c]
        res = kernel_rows(c, a.iters, a.repeats)
        fl = res["floors"]
        print(f"{c} conv1 (bs {n}, {'x'.join(map(str, spatial))}): ms per call, median of {a.repeats} windows x {a.iters} calls; "
              f"+- = spread of the windows")
        print(f"  floors: 54 FMA per output at 157 TFLOP/s {fl['fma_ms']:.3f} ms; the 64-channel tensor once at 8 TB/s "
              f"{fl['store_f32_ms']:.3f} ms fp32, {fl['store_bf16_ms']:.3f} ms bf16")
        print("  labels: " + ", ".join(f"{k} = {v}" for k, v in res["labels"].items()))
        for group, first in (("forward", "(a) conv2p_forward f32"), ("wgrad", "(a) conv2p_backward_weight f32 dy")):
            rows = res[group]
            for name, r in rows.items():
                print(f"  {group:8s} {name:46s} {r['ms']:9.4f} +-{r['spread']:7.4f}")
            a_row = rows[first]
            best_name, best = min(((k, r) for k, r in rows.items() if k.startswith("(c")), key=lambda kr: kr[1]["ms"])
            wins = a_row["ms"] + a_row["spread"] < best["ms"] - best["spread"]
            ok &= wins
            b32 = [r for k, r in rows.items() if k.startswith("(b)")][0]
            b16 = [r for k, r in rows.items() if k.startswith("(b)")][1]
            a16 = [r for k, r in rows.items() if k.startswith("(a)")][1]
            print(f"  {group}: (a) {a_row['ms']:.4f} vs the faster composition {best_name} {best['ms']:.4f}: "
                  f"{'FASTER beyond the spreads' if wins else 'NOT faster beyond the spreads'}; (a)/(b) = "
                  f"{a_row['ms'] / b32['ms']:.2f} fp32, {a16['ms'] / b16['ms']:.2f} bf16")
        if c in steps:
            print(f"  GAN.fit_batch, ms per step (median of {a.rounds} processes x {a.repeats} windows x {a.step_iters} steps; "
                  f"+- = largest spread seen)")
            for cond, runs in steps[c].items():
                ms = [r["ms"] for r in runs]
                sp = max(max(r["spread"] for r in runs), max(ms) - min(ms))
                print(f"  conditional={str(cond):5s} {statistics.median(ms):9.2f} +-{sp:6.2f}   (d_loss of the last step "
                      f"{runs[-1]['d_loss']:.4f})")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
