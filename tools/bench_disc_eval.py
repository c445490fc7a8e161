#!/usr/bin/env python3
"""Eval-mode discriminator forwards beside train-mode forwards (development aid; needs an MI355X).

    python tools/bench_disc_eval.py                       # this tree: eval and train rows
    python tools/bench_disc_eval.py --parent DIR          # + the train-mode forward of another built checkout (the
                                                          #   parent commit), alternated with this tree's in one visit

Rows: variant A at C3 (2-D 256^2, bs 16, fp32) and C5 (128^3, bs 4, bf16 storage), variant B on 896 patches of 16^3
(fp32 and bf16 storage; with and without taps in eval mode).  Each figure: HIP events around `iters` forwards under
no_grad after a warm-up, per forward; median of `repeats` windows, spread = max - min of the windows.  Every
(tree, mode) runs in a fresh child process, trees alternating, so that two trees never share a process or a warmed
allocator.  The condition checked at the end: no eval forward is slower than the other tree's train-mode forward of the
same shape by more than that row's own spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [  # name, variant, input shape, dims, storage, use_perceptual
    ("A C3 256^2 bs16 f32", "A", (16, 1, 256, 256), 2, "f32", None),
    ("A C5 128^3 bs4 bf16", "A", (4, 1, 128, 128, 128), 3, "bf16", None),
    ("B 896x16^3 f32 taps", "B", (896, 1, 16, 16, 16), 3, "f32", True),
    ("B 896x16^3 f32 fused", "B", (896, 1, 16, 16, 16), 3, "f32", False),
    ("B 896x16^3 bf16 taps", "B", (896, 1, 16, 16, 16), 3, "bf16", True),
    ("B 896x16^3 bf16 fused", "B", (896, 1, 16, 16, 16), 3, "bf16", False),
]


def child(tree, mode, iters, repeats):
    sys.path.insert(0, tree)
    import torch
    from mpgan_amd.networks import Discriminator, PatchDiscriminator
    out = {}
    for name, variant, shape, dims, storage, perceptual in ROWS:
        torch.manual_seed(0)
        if variant == "A":
            d = Discriminator((1,) + shape[2:], dimensions=dims, device="cuda", storage_dtype=storage)
        else:
            d = PatchDiscriminator((1,) + shape[2:], use_perceptual=perceptual, dimensions=dims, device="cuda",
                                   storage_dtype=storage)
        x = torch.rand(*shape, device="cuda") * 2 - 1
        d.train()
        with torch.no_grad():
            d(x)                                   # running statistics worth the name
            d.train(mode == "train")
            for _ in range(3):
                d(x)
            torch.cuda.synchronize()
            windows = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    d(x)
                e1.record()
                e1.synchronize()
                windows.append(e0.elapsed_time(e1) / iters)
        out[name] = {"ms": statistics.median(windows), "spread": max(windows) - min(windows)}
        del d, x
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(tree, mode, iters, repeats):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--mode", mode, "--iters", str(iters),
           "--repeats", str(repeats)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    for line in res.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError(f"{tree} {mode}: no result (exit {res.returncode})\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout whose train-mode forward is the yardstick")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--mode", default="eval", choices=("eval", "train"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.tree, a.mode, a.iters, a.repeats)
        return
    base_tree = a.parent or HERE
    runs = {"base train": [], "eval": [], "train": []}
    for _ in range(a.rounds):                      # alternate: base train, this eval, this train
        runs["base train"].append(run_child(base_tree, "train", a.iters, a.repeats))
        runs["eval"].append(run_child(HERE, "eval", a.iters, a.repeats))
        runs["train"].append(run_child(HERE, "train", a.iters, a.repeats))

    def fold(kind, name):
        ms = [r[name]["ms"] for r in runs[kind]]
        sp = max(max(r[name]["spread"] for r in runs[kind]), max(ms) - min(ms))     # within a process and across processes
        return statistics.median(ms), sp

    label = "parent" if a.parent else "this tree"
    print(f"forward per call, ms (median of {a.rounds} processes x {a.repeats} windows x {a.iters} calls; +- = largest spread seen)")
    print(f"{'row':24s} {'train (' + label + ')':>22s} {'train (this tree)':>20s} {'eval (this tree)':>20s}  eval - train")
    slower = []
    for name, *_ in ROWS:
        (bt, bs), (tt, ts), (et, es) = fold("base train", name), fold("train", name), fold("eval", name)
        print(f"{name:24s} {bt:14.3f} +-{bs:5.3f} {tt:12.3f} +-{ts:5.3f} {et:12.3f} +-{es:5.3f}  {et - bt:+8.3f}")
        if et > bt + bs:
            slower.append(name)
    print("eval forwards slower than the yardstick's train-mode forward by more than its spread:", slower or "none")
    sys.exit(1 if slower else 0)


if __name__ == "__main__":
    main()
