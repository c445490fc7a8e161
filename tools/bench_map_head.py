#!/usr/bin/env python3
"""The Markovian (PatchGAN) head beside the Linear head (development aid; needs an MI355X).

    python tools/bench_map_head.py                 # C3: 2-D 256^2, bs 16, fp32 storage
    python tools/bench_map_head.py --dtype bf16    # C5: 128^3, bs 4, bf16 storage
    python tools/bench_map_head.py --no-steps      # the head launches alone

Head rows: the head's own launches on the last layer's tensor at that shape (16 x 61^2 x 256 at C3, 4 x 29^3 x 256 at
C5; fp32 in every plan), as the training plans issue them: forward through the BatchNorm + LeakyReLU prologue in fp32
storage and without one in bf16 storage, backward with all three outputs (the D step) and with g_a alone (the G step).
Step rows: GAN.fit_batch with d_head="linear" and d_head="markovian", each in a fresh child process, alternating.
Each figure: HIP events around `iters` calls after a warm-up, per call; median of `repeats` windows, spread = max - min
of the windows (the method of tools/bench_disc_eval.py).  The floor printed beside a head row is the bytes that launch
has to move once (z for the forward; g_a written for the G-step backward; z read and g_a written for the D step's) at
8 TB/s.  No gate: the two heads do different work."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
CONFIGS = {  # dtype -> name, batch, spatial, last feature map, step iterations
    "f32": ("C3 256^2 bs16 f32", 16, (256, 256), (1, 61, 61)),
    "bf16": ("C5 128^3 bs4 bf16", 4, (128, 128, 128), (29, 29, 29)),
}
HBM_BYTES_PER_S = 8e12


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


def head_rows(dtype, iters, repeats):
    import torch
    from mpgan_amd import ops
    _, n, _, last = CONFIGS[dtype]
    c, dims = 256, 2 if last[0] == 1 else 3
    k = (1, 4, 4) if dims == 2 else (4, 4, 4)
    torch.manual_seed(0)
    z = torch.rand(n, *last, c, device="cuda") - 0.5
    g_a = torch.empty_like(z)
    pro = None
    if dtype == "f32":                               # fp32 storage: raw z read through BatchNorm + LeakyReLU
        pro = ops.Prologue(torch.rand(c, device="cuda") + 0.5, torch.rand(c, device="cuda") - 0.5, 0, ops.ACT_LEAKY, 0.2)
    P_lin = last[0] * last[1] * last[2]
    out = tuple(i - kk + 1 for i, kk in zip(last, k))
    P_map = out[0] * out[1] * out[2]
    z_bytes = z.numel() * 4
    rows = {}
    # Linear head
    w = ops.pack_weight((torch.rand(1, c, *last, device="cuda") - 0.5) * 1e-3)
    bias, part = torch.zeros(1, device="cuda"), torch.empty(ops.linear1_partials(n), device="cuda")
    logit, prob, dl = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.rand(n, device="cuda") - 0.5
    dw, db = torch.zeros(c * P_lin, device="cuda"), torch.zeros(1, device="cuda")
    rows["linear1_forward"] = (timed(lambda: ops.linear1_forward(z, pro, w, bias, part, logit, prob), iters, repeats),
                               z_bytes + w.numel() * 4)
    rows["linear1_backward (g_a, dw, dbias)"] = (
        timed(lambda: ops.linear1_backward(z, pro, w, dl, g_a, dw, db, beta=1.0), iters, repeats), 2 * z_bytes)
    rows["linear1_backward (g_a)"] = (
        timed(lambda: ops.linear1_backward(z, pro, w, dl, g_a, None, None), iters, repeats), z_bytes)
    # Markovian head
    wk = k[3 - dims:]
    wm = ops.pack_weight((torch.rand(1, c, *wk, device="cuda") - 0.5) / 16)
    logit, prob = torch.empty(n * P_map, device="cuda"), torch.empty(n * P_map, device="cuda")
    dl = torch.rand(n * P_map, device="cuda") - 0.5
    dw = torch.zeros(1, c, *wk, device="cuda")
    ws = torch.empty(ops.maphead_workspace(n, last, c, k) // 4, device="cuda")
    rows["maphead_forward"] = (timed(lambda: ops.maphead_forward(z, pro, k, wm, bias, logit, prob), iters, repeats),
                               z_bytes)
    rows["maphead_backward (g_a, dw, dbias)"] = (
        timed(lambda: ops.maphead_backward(z, pro, k, wm, dl, g_a, dw, db, beta=1.0, workspace=ws), iters, repeats),
        2 * z_bytes)
    rows["maphead_backward (g_a)"] = (
        timed(lambda: ops.maphead_backward(z, pro, k, wm, dl, g_a, None, None), iters, repeats), z_bytes)
    return {name: dict(t, floor_ms=b / HBM_BYTES_PER_S * 1e3, mbytes=b / 1e6) for name, (t, b) in rows.items()}


def step_child(dtype, head, iters, repeats):
    import torch
    from mpgan_amd.gan import GAN
    _, n, spatial, _ = CONFIGS[dtype]
    torch.manual_seed(0)
    gan = GAN(1, *spatial, dimensions=len(spatial), g_lr=1e-6, d_lr=1e-6, storage_dtype=dtype, d_head=head)
    if head == "linear":                             # as bench.py: keep the huge Linear head out of sigmoid saturation
        with torch.no_grad():
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


def run_child(dtype, head, iters, repeats):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", head, "--dtype", dtype, "--step-iters", str(iters),
           "--repeats", str(repeats)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    for line in res.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError(f"{head}: no result (exit {res.returncode})\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32", choices=("f32", "bf16"))
    ap.add_argument("--iters", type=int, default=20, help="head calls per window")
    ap.add_argument("--step-iters", type=int, default=3, help="training steps per window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--child", default=None, choices=("linear", "markovian"))
    a = ap.parse_args()
    if a.child:
        step_child(a.dtype, a.child, a.step_iters, a.repeats)
        return
    name = CONFIGS[a.dtype][0]
    steps = {"linear": [], "markovian": []}
    if not a.no_steps:                               # before this process opens the GPU: one process at a time
        for _ in range(a.rounds):
            for head in steps:
                steps[head].append(run_child(a.dtype, head, a.step_iters, a.repeats))
    print(f"{name}: head launches, ms per call (median of {a.repeats} windows x {a.iters} calls; +- = spread of the windows)")
    print(f"{'launch':36s} {'ms':>9s} {'+-':>7s} {'MB once':>9s} {'floor ms @ 8 TB/s':>18s}")
    for row, r in head_rows(a.dtype, a.iters, a.repeats).items():
        print(f"{row:36s} {r['ms']:9.4f} {r['spread']:7.4f} {r['mbytes']:9.1f} {r['floor_ms']:18.4f}")
    if a.no_steps:
        return
    print(f"{name}: GAN.fit_batch, ms per step (median of {a.rounds} processes x {a.repeats} windows x "
          f"{a.step_iters} steps; +- = largest spread seen)")
    for head, runs in steps.items():
        ms = [r["ms"] for r in runs]
        sp = max(max(r["spread"] for r in runs), max(ms) - min(ms))
        print(f"d_head={head:10s} {statistics.median(ms):9.2f} +-{sp:6.2f}   (d_loss of the last step {runs[-1]['d_loss']:.4f})")


if __name__ == "__main__":
    main()
