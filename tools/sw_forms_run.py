#!/usr/bin/env python3
"""Two small sliding-window calls in each blend mode, for a kernel trace: the labels mpgan_sw_kernel_name gives for
their launches are printed, to be held against the names in the profiler's statistics.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/sw_forms_run.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpgan_amd import inference as inf  # noqa: E402

ALIGNED = 16        # stand-in for the buffers the call allocates itself


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    names = set()
    # (input, roi, input offset in elements): scalar count / blend / finalize; everything in quads, unaligned input
    for shape, roi, off in (((1, 1, 20, 22, 26), (8, 8, 12), 0), ((2, 1, 16, 16, 24), (8, 8, 16), 1)):
        buf = torch.empty(off + torch.Size(shape).numel(), device=dev)
        x = buf[off:].view(shape).copy_(torch.rand(shape, generator=g))
        plan = inf.plan_windows(shape[2:], roi, 0.25)
        geom, keep = inf._geometry(plan, shape[0], dev)
        for mode in ("constant", "gaussian"):
            inf.sliding_window_inference(x, roi, 3, lambda w: w * 0.5, overlap=0.25, mode=mode)
            imp = None if mode == "constant" else ALIGNED
            names |= {inf.sw_kernel_name("gather", geom, x.data_ptr(), ALIGNED),
                      inf.sw_kernel_name("count", geom, imp, ALIGNED),
                      inf.sw_kernel_name("blend", geom, ALIGNED, imp, ALIGNED),
                      inf.sw_kernel_name("finalize", geom, ALIGNED, ALIGNED, ALIGNED)}
    torch.cuda.synchronize()
    for n in sorted(names):
        print(n)


if __name__ == "__main__":
    main()
