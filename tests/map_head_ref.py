"""TEST INFRASTRUCTURE (imported by tests/ only, never by the product path).

Torch restatement of variant A's Markovian (PatchGAN) head and of the discriminator that ends in it.  The reference
has no such head (it lists it as a TODO, code/GAN/GAN_final.py:125), so parity is against this restatement run in
float64: F.conv2d / F.conv3d on the activated tensor for the head, nn.BatchNorm / LeakyReLU(0.2) for the stack
(code/GAN/GAN_final.py:159-196).  The closed forms of the head's backward are what the kernels are written from; they
are pinned to autograd in tests/test_map_head_host.py."""
import torch
import torch.nn as nn
import torch.nn.functional as F

HEAD_KERNEL = 4


def _conv(dims):
    return F.conv2d if dims == 2 else F.conv3d


def activate(z, scale, shift, slope=0.2):
    """a = LeakyReLU(z*scale + shift) on an NC(D)HW tensor; scale / shift of shape (C,) or per sample (N, C)."""
    dims = z.dim() - 2
    shp = ([1, -1] if scale.dim() == 1 else [z.shape[0], -1]) + [1] * dims
    y = z * scale.reshape(shp) + shift.reshape(shp)
    return torch.where(y > 0, y, y * slope)


def head_forward(a, w, b):
    """a: activated NC(D)HW; w: (1, C, *k); b: (1,).  Returns (logit, prob), each (N, 1, *map)."""
    logit = _conv(a.dim() - 2)(a, w, b)
    return logit, torch.sigmoid(logit)


def head_backward(a, w, dlogit):
    """Closed forms of the head's backward for dlogit of shape (N, 1, *map):
         g_a[n][c][q]  = sum_tap dlogit[n][q - tap] * w[c][tap]   over the taps that land inside the map
         dw[c][tap]    = sum_{n,p} dlogit[n][p] * a[n][c][p + tap]
         dbias         = sum dlogit
    written as explicit loops over the taps (no conv call)."""
    dims = a.dim() - 2
    k = tuple(w.shape[2:])
    out = tuple(dlogit.shape[2:])
    g_a = torch.zeros_like(a)
    dw = torch.zeros_like(w)
    taps = [()]
    for kd in k:
        taps = [t + (i,) for t in taps for i in range(kd)]
    for tap in taps:
        win = (slice(None), slice(None)) + tuple(slice(t, t + o) for t, o in zip(tap, out))
        wt = w[(0, slice(None)) + tap]                                    # (C,)
        g_a[win] += dlogit * wt.reshape([1, -1] + [1] * dims)
        dw[(0, slice(None)) + tap] = (dlogit * a[win]).sum(dim=[0] + list(range(2, 2 + dims)))
    return g_a, dw, dlogit.sum().reshape(1)


class MarkovianDiscriminator(nn.Module):
    """4 x (valid conv -> BatchNorm -> LeakyReLU 0.2) -> Conv(256, 1, 4) -> Sigmoid, with the state_dict keys of
    mpgan_amd.networks.Discriminator(..., head="markovian")."""

    def __init__(self, dimensions=3):
        super().__init__()
        Cv = {2: nn.Conv2d, 3: nn.Conv3d}[dimensions]
        Bn = {2: nn.BatchNorm2d, 3: nn.BatchNorm3d}[dimensions]
        self.model_conv = nn.Sequential(
            Cv(1, 64, 3, 1), Bn(64), nn.LeakyReLU(0.2),
            Cv(64, 128, 3, 1), Bn(128), nn.LeakyReLU(0.2),
            Cv(128, 256, 4, 2), Bn(256), nn.LeakyReLU(0.2),
            Cv(256, 256, 4, 2), Bn(256), nn.LeakyReLU(0.2))
        self.model_head = nn.Sequential(Cv(256, 1, kernel_size=HEAD_KERNEL, stride=1, bias=True), nn.Sigmoid())

    def forward(self, img):
        return self.model_head(self.model_conv(img))


def bce(p, t):
    return F.binary_cross_entropy(p, t)


def step_losses_g(gen, disc, batch):
    """The generator branch of GAN.training_step (code/GAN/GAN_final.py:254-273) with labels of D's output shape."""
    fake = gen(batch["t1w"])
    d = disc(fake)
    g_adv = bce(d, torch.ones_like(d))
    g_rec = F.l1_loss(fake, batch["t2w"])
    return {"g_adv_loss": g_adv, "g_recon_loss": g_rec, "g_loss": g_adv + g_rec}


def step_loss_d(gen, disc, batch, one_sided=0.9):
    """The discriminator branch (code/GAN/GAN_final.py:276-296) with labels of D's output shape."""
    d_real = disc(batch["t2w"])
    d_fake = disc(gen(batch["t1w"]).detach())
    return (bce(d_real, torch.full_like(d_real, one_sided)) + bce(d_fake, torch.zeros_like(d_fake))) / 2
