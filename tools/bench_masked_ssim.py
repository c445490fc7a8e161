#!/usr/bin/env python3
"""The masked SSIM loss (forward + backward) beside the unmasked SSIMLoss and the torch composition, on the device
(needs an MI355X).

    python tools/bench_masked_ssim.py [--iters 10] [--repeats 7] [--mask none explicit threshold]

Rows: (4, 1, 128, 128, 128) and (16, 1, 256, 256), value range (-1, 1), gradient for the first tensor (the generator's
case).  Paths, their windows alternating in one process:
  none       losses.ssim_loss without a mask: the plain kernels;
  explicit   ... with a uint8 mask (target > 0, a little over a third of the voxels of the structured pair);
  threshold  ... with threshold=0.0: the same foreground read from the staged target, no mask tensor; the threshold is
             a number, so that the row times the two SSIM kernels and not Otsu's histogram in front of them;
  torch      tests/masked_ssim_ref.py with the explicit mask, on the device in fp32 with autograd.
Each figure: HIP events around `iters` calls after a warm-up, per call; median of `repeats` windows, spread = max - min
of the windows.  ssim_map rides along: metrics.ssim_map of one 128^3 volume and one 256^2 slice beside the map of the
torch composition."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import masked_ssim_ref  # noqa: E402
import ssim_loss_ref  # noqa: E402
from bench_ssim_loss import measure  # noqa: E402
from mpgan_amd import losses, metrics  # noqa: E402

RANGE = (-1.0, 1.0)
MODES = ("none", "explicit", "threshold")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--mask", nargs="+", choices=MODES, default=list(MODES))
    args = ap.parse_args()
    print(f"ms per forward + backward (grad pred): median of {args.repeats} windows x {args.iters} calls (+- = max - min)")
    for label, shape in (("4x128^3", (4, 1, 128, 128, 128)), ("16x256^2", (16, 1, 256, 256))):
        pred, target = (x.cuda() for x in ssim_loss_ref.structured_pair(shape, seed=1))
        mask = (target > 0).to(torch.uint8)
        p = pred.clone().requires_grad_(True)
        source = {"none": {}, "explicit": {"mask": mask}, "threshold": {"threshold": 0.0}}
        paths = {mode: (lambda kw=source[mode]: torch.autograd.grad(losses.ssim_loss(p, target, RANGE, **kw), (p,)))
                 for mode in args.mask}
        paths["torch"] = lambda: torch.autograd.grad(
            masked_ssim_ref.loss(p, target, mask, RANGE, dtype=torch.float32), (p,))
        if "explicit" in paths:
            go, gt = paths["explicit"](), paths["torch"]()
            if float((go[0] - gt[0]).abs().max()) > 1e-3 * float(gt[0].abs().max()):
                raise SystemExit(f"{label}: the kernel path and the torch composition disagree")
            if "threshold" in paths and not torch.equal(paths["threshold"]()[0], go[0]):
                raise SystemExit(f"{label}: threshold mode and the explicit mask disagree")
            del go, gt
        med, spr = measure(paths, args.iters, args.repeats)
        print(f"{label}: foreground {float(mask.float().mean()):.3f} of the voxels")
        for k in paths:
            rel = f"  {med[k] / med['none']:5.3f} x none" if "none" in med and k != "none" else ""
            print(f"  {k:10s} {med[k]:9.4f} +-{spr[k]:6.4f}{rel}")
        a, b = pred[0, 0] + 1.0, target[0, 0] + 1.0
        maps = {"ssim_map": lambda: metrics.ssim_map(a, b, 2.0),
                "torch map": lambda: masked_ssim_ref.ssim_map(a[None, None], b[None, None], (0.0, 2.0), torch.float32)}
        med, spr = measure(maps, args.iters, args.repeats)
        for k in maps:
            print(f"  {k:10s} {med[k]:9.4f} +-{spr[k]:6.4f}   (one image, forward only)")
        del pred, target, mask, p, paths, maps, a, b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
