"""sha256 of the raw bytes of every output that passes through a block sum of csrc/reduce.h (the pair losses with both
gradients, the metrics, grad_norm, l1_loss, adv_loss, DiffAugment, both heads) or through the image statistics of
csrc/image_stats.h (Otsu, the foreground mask / box / count, the masked L1, errors and SSIM, the banded joint
histogram), inputs from fixed CPU seeds.

    python tools/reduction_bits.py OUT.txt

The library is whatever MPGAN_LIB_PATH names (unset: the tree's own): run it once per build in a fresh process and
compare the two files (profiles/README.md, r24_bits.txt)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from mpgan_amd import losses, metrics, ops, preprocess  # noqa: E402
from mpgan_amd.augment import DiffAugment  # noqa: E402
from mpgan_amd.gan import reconstruction_loss  # noqa: E402
import metric_small_ref as MS  # noqa: E402
import ssim_loss_ref as SR  # noqa: E402

lines = []


def rec(name, t):
    t = t.detach().contiguous().cpu()
    h = hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"").hexdigest()
    lines.append(f"{name} {tuple(t.shape)} {t.dtype} {h}")


def pair(shape, seed):
    p, t = SR.structured_pair(shape, seed=seed)
    return p.cuda(), t.cuda()


def pair_loss(tag, make, shapes):
    for shape in shapes:
        for red in ("mean", "sum", "none"):
            p, t = pair(shape, 7)
            p.requires_grad_(True); t.requires_grad_(True)
            loss = make(red)(p, t)
            rec(f"{tag} {shape} {red} loss", loss)
            loss.sum().backward()
            rec(f"{tag} {shape} {red} grad_pred", p.grad)
            rec(f"{tag} {shape} {red} grad_target", t.grad)


pair_loss("ssim_loss", lambda r: losses.SSIMLoss((-1.0, 1.0), r), [(2, 2, 136, 544), (2, 2, 9, 17, 39)])
pair_loss("edge_loss", lambda r: losses.EdgeLoss(reduction=r), [(2, 2, 136, 544), (2, 2, 9, 17, 39)])
for bins in (23, 32):
    pair_loss(f"mi_loss bins{bins}", lambda r, b=bins: losses.GlobalMutualInformationLoss(b, reduction=r, value_range=(-1.0, 1.0)),
              [(3, 1, 136, 544)])
rec("parzen_joint", losses.parzen_joint_histogram(*pair((3, 1, 136, 544), 7), 23, value_range=(-1.0, 1.0)))

# metrics
for shape in ((136, 544), (9, 17, 39)):
    g = torch.Generator().manual_seed(11)
    a = torch.round(torch.rand(shape, generator=g) * 255)
    b = torch.round(0.8 * a + 0.2 * torch.rand(shape, generator=g) * 255)
    a, b = a.cuda(), b.cuda()
    rec(f"metrics.ssim {shape}", metrics.ssim(a, b, 256.0))
    for k, v in metrics.mutual_information(a, b).items():
        rec(f"metrics.mi {shape} {k}", v)
    for k, v in metrics.image_errors(a, b).items():
        rec(f"metrics.errors {shape} {k}", v)
    for k, v in metrics.score_volume(a * 0.01 - 1, b * 0.01 - 1, mutual_information=True).items():
        rec(f"metrics.score_volume {shape} {k}", v)
    m = (torch.rand(shape, generator=g) < 0.6).cuda()
    for k, v in metrics.image_errors(a, b, mask=m).items():
        rec(f"metrics.errors masked {shape} {k}", v)
    rec(f"metrics.ssim_map {shape}", metrics.ssim_map(a, b, 256.0))
    rec(f"metrics.ssim masked {shape}", metrics.ssim(a, b, 256.0, mask=m))
    rec(f"metrics.joint_histogram bins200 masked {shape}", metrics.joint_histogram(a, b, 200, mask=m))

for shape in MS.SSIM_SHAPES:                              # every tile edge of the SSIM forward, every degenerate pair
    for kind in MS.SSIM_KINDS:
        a, b, data_range = MS.ssim_pair(shape, kind)
        rec(f"metrics.ssim small {shape} {kind}", metrics.ssim(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), data_range))

# grad_norm
for n in (300003, 1000):
    g = (torch.rand(n, generator=torch.Generator().manual_seed(3)) - 0.5).cuda()
    ws = torch.empty(ops.grad_norm_workspace(n) // 8 + 1, dtype=torch.float64, device="cuda")
    for max_norm in (0.0, 1.0):
        rec(f"grad_norm {n} max {max_norm}", ops.grad_norm(g, torch.empty(2, device="cuda"), ws, 0.5, max_norm))

# l1 loss with gradient
p, t = pair((2, 1, 136, 544), 5)
p.requires_grad_(True)
l1 = reconstruction_loss(p, t)
rec("l1 loss", l1)
l1.backward()
rec("l1 grad", p.grad)

# adversarial objectives
for kind in ("bce_logits", "lsgan"):
    for n in (7, 70003):
        g = torch.Generator().manual_seed(n)
        z = ((torch.rand(n, generator=g) - 0.5) * 8).cuda()
        y = (torch.rand(n, generator=g) < 0.5).float().cuda()
        part = torch.empty(ops.adv_loss_partials(n), dtype=torch.float64, device="cuda")
        grad = torch.empty_like(z)
        rec(f"adv_loss {kind} {n} loss", ops.adv_loss(z, y, kind, part, torch.empty((), device="cuda"), grad))
        rec(f"adv_loss {kind} {n} grad", grad)

# DiffAugment with the contrast op
gen = torch.Generator(device="cuda").manual_seed(9)
x = (torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(4)) * 2 - 1).cuda().requires_grad_(True)
aug = DiffAugment("color,translation,cutout", generator=gen)
y = aug(x)
rec("diffaug color", aug.last_params.color)
rec("diffaug geom", aug.last_params.geom)
rec("diffaug forward", y)
up = (torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(6)) - 0.5).cuda()
y.backward(up)
rec("diffaug backward", x.grad)

# heads at the shapes of tests/test_map_head_gpu.py
import test_map_head_gpu as T  # noqa: E402
for name in T.CASES:
    case = T._case(name)
    logit, prob = T._forward(case)
    rec(f"maphead {name} logit", logit)
    rec(f"maphead {name} prob", prob)
    for beta in (0.0, 0.5):
        G, W, B = T._backward(case, beta=beta)
        rec(f"maphead {name} beta{beta} g_a", G)
        rec(f"maphead {name} beta{beta} dw", W)
        rec(f"maphead {name} beta{beta} dbias", B)
case = T._case("2d_map_1x1")
z, pro, k, wp, b, dl = T._device(case)
n = case["n"]
logit, prob = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
ops.linear1_forward(z, pro, wp, b, torch.empty(ops.linear1_partials(n), device="cuda"), logit, prob)
rec("linear1 logit", logit)
rec("linear1 prob", prob)
loss, dlogit = torch.empty((), device="cuda"), torch.empty(n, device="cuda")
ops.sigmoid_bce(logit, 1.0, 1.0, None, loss, dlogit)
rec("sigmoid_bce loss", loss)
rec("sigmoid_bce dlogit", dlogit)
g_a, dw, db = torch.empty_like(z), torch.empty_like(wp), torch.empty(1, device="cuda")
ops.linear1_backward(z, pro, wp, dlogit, g_a, dw, db)
rec("linear1 g_a", g_a)
rec("linear1 dw", dw)
rec("linear1 dbias", db)

# foreground statistics and the masked losses: the mask form and the threshold form
for shape in ((2, 2, 136, 544), (2, 2, 9, 17, 39)):
    _, t = pair(shape, 7)
    for bins in (64, 256):
        rec(f"otsu {shape} bins{bins}", preprocess.otsu_threshold(t, bins))
    rec(f"foreground_mask {shape}", preprocess.foreground_mask(t))
    rec(f"foreground_bbox {shape}", preprocess.foreground_bbox(t, margin=1))
    rec(f"foreground_count {shape}", preprocess.foreground_count(t))
    m = (torch.rand(shape, generator=torch.Generator().manual_seed(13)) < 0.6).cuda()
    for tag, kw in (("mask", dict(mask=m)), ("otsu", dict(threshold="otsu"))):
        pair_loss(f"masked_l1 {tag}", lambda r, kw=kw: lambda p, t: losses.masked_l1_loss(p, t, bg_weight=0.25, reduction=r, **kw),
                  [shape])
        pair_loss(f"ssim_loss {tag}", lambda r, kw=kw: lambda p, t: losses.ssim_loss(p, t, (-1.0, 1.0), r, **kw), [shape])

torch.cuda.synchronize()
with open(sys.argv[1], "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"{len(lines)} digests -> {sys.argv[1]} (library: {os.environ.get('MPGAN_LIB_PATH', 'the tree')})")
