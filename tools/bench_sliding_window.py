#!/usr/bin/env python3
"""Sliding-window inference of one (1, 1, 256, 256, 256) volume through an eval-mode 3-D CasNetGenerator
(roi 128^3, sw_batch_size 4, overlap 0.25: 27 windows in 7 predictor calls), both blend modes.  Prints the total
time, the predictor's share, and each window kernel's time with its algorithmic bytes / time next to the
6.3 TB/s achievable HBM figure (MI355X_MICROARCH.md).  Development aid."""
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mpgan_amd import inference as inf
from mpgan_amd._lib import lib
from mpgan_amd.networks import CasNetGenerator

SHAPE, ROI, SW, OVERLAP = (256, 256, 256), (128, 128, 128), 4, 0.25
ACHIEVABLE = 6.3e12


class Timed:
    """Predictor wrapper: device time spent inside the predictor, from events around each call."""

    def __init__(self, fn):
        self.fn, self.ev = fn, []

    def __call__(self, x):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = self.fn(x)
        b.record()
        self.ev.append((a, b))
        return y

    def ms(self):
        return sum(a.elapsed_time(b) for a, b in self.ev)


def kernel_ms(fn, reps=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main(reps=5):
    torch.manual_seed(0)
    gen = CasNetGenerator((1,) + ROI, 6, dimensions=3, device="cuda")
    x = torch.rand(1, 1, *SHAPE, device="cuda") * 2 - 1
    gen.train()
    with torch.no_grad():
        gen(x[..., :128, :128, :128].contiguous())
    gen.eval()
    plan = inf.plan_windows(SHAPE, ROI, OVERLAP)
    total = plan.num_windows
    print(f"volume {SHAPE}, roi {ROI}, sw_batch_size {SW}, overlap {OVERLAP}: {total} windows, "
          f"{(total + SW - 1) // SW} predictor calls")
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    rvol = ROI[0] * ROI[1] * ROI[2]
    pvol = plan.padded[0] * plan.padded[1] * plan.padded[2]
    for mode in ("constant", "gaussian"):
        with torch.no_grad():
            for _ in range(2):
                inf.sliding_window_inference(x, ROI, SW, gen, overlap=OVERLAP, mode=mode)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                inf.sliding_window_inference(x, ROI, SW, gen, overlap=OVERLAP, mode=mode)
            torch.cuda.synchronize()
            tot = (time.perf_counter() - t) / reps * 1e3
            tp = Timed(gen)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            inf.sliding_window_inference(x, ROI, SW, tp, overlap=OVERLAP, mode=mode)
            b.record()
            torch.cuda.synchronize()
            one, pred = a.elapsed_time(b), tp.ms()
        print(f"\n[{mode}] total {tot:.2f} ms (host clock, mean of {reps}); one run by events {one:.2f} ms, "
              f"predictor {pred:.2f} ms ({100 * pred / one:.1f} %), everything else {one - pred:.2f} ms "
              f"({100 * (one - pred) / one:.1f} %)")

        # each window kernel alone, at the shapes of this run
        imp = inf._device_importance(plan.roi, mode, 0.125, x.device)
        ip = None if imp is None else imp.data_ptr()
        g, keep = inf._geometry(plan, 1, x.device)
        gp = C.byref(g)
        win = torch.empty((SW, 1) + ROI, device="cuda")
        pred_t = torch.rand((SW, 1) + ROI, device="cuda")
        count = torch.empty(plan.padded, device="cuda")
        acc = torch.zeros((1, 1) + plan.padded, device="cuda")
        out = torch.empty((1, 1) + SHAPE, device="cuda")
        # the second call (windows 4..7) as the representative blend and gather; bytes of the voxels it covers
        first = SW
        cov = torch.zeros(plan.padded, dtype=torch.bool)
        for s in plan.windows()[first:first + SW]:
            cov[s[0]:s[0] + ROI[0], s[1]:s[1] + ROI[1], s[2]:s[2] + ROI[2]] = True
        covered = int(cov.sum())
        imp_bytes = 0 if imp is None else 4 * rvol
        rows = [
            ("sw_gather", lambda: L.mpgan_sw_gather(gp, x.data_ptr(), 1, first, SW, 0.0, win.data_ptr(), st),
             2 * 4 * SW * rvol, "read + write of 4 windows"),
            ("sw_count", lambda: L.mpgan_sw_count(gp, ip, count.data_ptr(), st),
             4 * pvol + imp_bytes, "count map write (+ map read)"),
            ("sw_blend", lambda: L.mpgan_sw_blend(gp, pred_t.data_ptr(), 1, first, SW, ip, acc.data_ptr(), st),
             4 * SW * rvol + 8 * covered + imp_bytes, "pred read, covered acc read + write (+ map)"),
            ("sw_finalize", lambda: L.mpgan_sw_finalize(gp, acc.data_ptr(), 1, count.data_ptr(), out.data_ptr(), st),
             4 * 3 * pvol, "acc + count read, out write"),
        ]
        for name, fn, nbytes, what in rows:
            ms = kernel_ms(fn)
            bw = nbytes / (ms * 1e-3)
            print(f"  {name:12s} {ms * 1e3:8.1f} us  {nbytes / 1e6:8.1f} MB ({what})  {bw / 1e12:5.2f} TB/s "
                  f"= {100 * bw / ACHIEVABLE:4.0f} % of 6.3 TB/s")
        visits = total * rvol
        if imp is not None:
            print(f"  sw_count visits {visits / pvol:.2f} covering windows per voxel on average: with the map it reads "
                  f"{4 * visits / 1e6:.0f} MB of it from L2 / MALL (the 8 MB map is cache-resident), not counted above")
        print("  sw_finalize reads acc and count just written by the repetitions before it: a figure above the HBM "
              "rate is served partly by the 256 MB MALL")
        n_calls = (total + SW - 1) // SW
        print(f"  per run: 1 count + {n_calls} gathers + {n_calls} blends + 1 finalize (+ zeroing the accumulator)")


if __name__ == "__main__":
    main()
