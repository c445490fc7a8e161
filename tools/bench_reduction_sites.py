"""HIP-event timing of the entry points whose kernels end in a block sum of csrc/reduce.h and that bench.py does not
run: forward + backward at 4x1x128^3 and 16x1x256x256, 5 warm-ups, 30 timed calls, median and minimum ms.

    python tools/bench_reduction_sites.py LABEL OUT.txt        (appends one row per entry point and shape)

The library is whatever MPGAN_LIB_PATH names: alternate two builds, one process each (profiles/README.md,
r24_refactor_timing.txt)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mpgan_amd import losses, metrics, ops  # noqa: E402
from mpgan_amd.gan import reconstruction_loss  # noqa: E402

label, out = sys.argv[1], sys.argv[2]
WARM, ITERS = 5, 30


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


rows = []
for shape in ((4, 1, 128, 128, 128), (16, 1, 256, 256)):
    g = torch.Generator().manual_seed(1)
    t = (torch.rand(shape, generator=g) * 2 - 1).cuda()
    p = (0.7 * t + 0.3 * (torch.rand(shape, generator=g).cuda() * 2 - 1)).requires_grad_(True)

    def fb(mod):
        def run():
            p.grad = None
            mod(p, t).backward()
        return run

    rows.append(("ssim_loss fwd+bwd", shape, timed(fb(losses.SSIMLoss((-1.0, 1.0))))))
    rows.append(("edge_loss fwd+bwd", shape, timed(fb(losses.EdgeLoss()))))
    rows.append(("l1 fwd+bwd", shape, timed(fb(reconstruction_loss))))
    flat = t.reshape(-1)
    ws = torch.empty(ops.grad_norm_workspace(flat.numel()) // 8 + 1, dtype=torch.float64, device="cuda")
    out2 = torch.empty(2, device="cuda")
    rows.append(("grad_norm", shape, timed(lambda: ops.grad_norm(flat, out2, ws, 1.0, 1.0))))
    # the metrics take one (D, H, W) volume or one (H, W) slice: the batch's first item
    a = torch.round((t[0, 0] + 1) * 127.5)
    b = torch.round((p.detach()[0, 0] + 1) * 127.5)
    rows.append(("metrics.ssim", tuple(a.shape), timed(lambda: metrics.ssim(a, b, 256.0))))
    rows.append(("metrics.image_errors", tuple(a.shape), timed(lambda: metrics.image_errors(a, b))))
    rows.append(("metrics.mutual_information", tuple(a.shape), timed(lambda: metrics.mutual_information(a, b))))

with open(out, "a") as f:
    for name, shape, (med, lo) in rows:
        f.write(f"{label} | {name} | {shape} | median {med:.4f} ms | min {lo:.4f} ms\n")
print(f"{label}: {len(rows)} rows -> {out}")
