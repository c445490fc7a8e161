"""TEST INFRASTRUCTURE (imported by tests/ only, never by the product path).

Torch restatement of the conditional (pix2pix) discriminator: the reference's Discriminator
(code/GAN/GAN_final.py:159-209) with Conv(2, 64, 3) as its first layer, applied to torch.cat([img, cond], 1) -- plain
nn modules, run in float64 by the tests.  Input channel 0 is the image and channel 1 the condition, and the state_dict
keys are those of mpgan_amd.networks.Discriminator(..., conditional=True) with either head.  Also the first conv alone
with its closed-form error scales, and the bf16-storage restatement of a whole step for both heads (oracle/bf16_emul.py's
contract: fp32 arithmetic, one bf16 rounding wherever the HIP path stores a tensor)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HEAD_KERNEL = 4


def _conv(dims):
    return F.conv2d if dims == 2 else F.conv3d


def feature_sizes(spatial):
    sizes = [tuple(spatial)]
    for k, s in ((3, 1), (3, 1), (4, 2), (4, 2)):
        sizes.append(tuple((n - k) // s + 1 for n in sizes[-1]))
    return sizes


class CondDiscriminator(nn.Module):
    """4 x (valid conv -> BatchNorm -> LeakyReLU 0.2) on cat(img, cond), then Flatten -> Linear -> Sigmoid
    (head="linear") or Conv(256, 1, 4) -> Sigmoid (head="markovian"); logits=True leaves the Sigmoid out of forward."""

    def __init__(self, spatial, head="linear", logits=False, in_channels=2):
        super().__init__()
        dims = len(spatial)
        Cv = {2: nn.Conv2d, 3: nn.Conv3d}[dims]
        Bn = {2: nn.BatchNorm2d, 3: nn.BatchNorm3d}[dims]
        self.head, self.logits = head, logits
        self.model_conv = nn.Sequential(
            Cv(in_channels, 64, 3, 1), Bn(64), nn.LeakyReLU(0.2),
            Cv(64, 128, 3, 1), Bn(128), nn.LeakyReLU(0.2),
            Cv(128, 256, 4, 2), Bn(256), nn.LeakyReLU(0.2),
            Cv(256, 256, 4, 2), Bn(256), nn.LeakyReLU(0.2))
        if head == "markovian":
            self.model_head = nn.Sequential(Cv(256, 1, kernel_size=HEAD_KERNEL, stride=1, bias=True), nn.Sigmoid())
        else:
            self.model_linear = nn.Sequential(nn.Flatten(), nn.Linear(256 * int(np.prod(feature_sizes(spatial)[-1])), 1),
                                              nn.Sigmoid())

    def head_logit(self, a):
        return self.model_head[0](a) if self.head == "markovian" else self.model_linear[1](a.flatten(1))

    def forward(self, img, cond=None):
        x = img if cond is None else torch.cat([img, cond], 1)
        logit = self.head_logit(self.model_conv(x))
        return logit if self.logits else torch.sigmoid(logit)


def objective(v, target: float, kind: str):
    """The adversarial objective on D's output v against a constant target: "bce" on probabilities, "lsgan" /
    "bce_logits" on logits (mpgan_amd.gan.adversarial_loss's kinds)."""
    t = torch.full_like(v, target)
    if kind == "bce":
        return F.binary_cross_entropy(v, t)
    if kind == "lsgan":
        return F.mse_loss(v, t)
    return F.binary_cross_entropy_with_logits(v, t)


# ---- the first conv alone ---------------------------------------------------------------------------------------------
def conv1(img, cond, w, b):
    """y = conv(cat(img, cond), w) + b for NC(D)HW planes with one channel each and w of shape (64, 2, k...)."""
    return _conv(img.dim() - 2)(torch.cat([img, cond], 1), w, b)


def conv1_scale(img, cond, w, b):
    """|w| * |x| + |b|: the magnitude a rounding error of the forward is relative to."""
    return conv1(img.abs(), cond.abs(), w.abs(), b.abs())


def conv1_grads(img, cond, w, dy):
    """(dx of the image plane = channel 0 of the input gradient, dW (64, 2, k...), dbias) by autograd."""
    x = torch.cat([img, cond], 1).clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = torch.zeros(w.shape[0], dtype=w.dtype, requires_grad=True)
    _conv(img.dim() - 2)(x, wr, br).backward(dy)
    return x.grad[:, :1], wr.grad, br.grad


def conv1_wgrad_scale(img, cond, dy):
    """sum |dy| |x| per weight element: the magnitude a rounding error of the weight gradient is relative to."""
    return conv1_grads(img.abs(), cond.abs(), torch.zeros(dy.shape[1], 2, *([3] * (img.dim() - 2)), dtype=img.dtype),
                       dy.abs())[1]


# ---- trainer ----------------------------------------------------------------------------------------------------------
def step_losses_g(gen, disc, batch, kind):
    """The generator branch of GAN.training_step (code/GAN/GAN_final.py:254-273) with a conditional discriminator."""
    fake = gen(batch["t1w"])
    g_adv = objective(disc(fake, batch["t1w"]), 1.0, kind)
    g_rec = F.l1_loss(fake, batch["t2w"])
    return {"g_adv_loss": g_adv, "g_recon_loss": g_rec, "g_loss": g_adv + g_rec}


def step_loss_d(gen, disc, batch, kind, one_sided=0.9):
    """The discriminator branch (code/GAN/GAN_final.py:276-296): D(t2w, t1w) and D(G(t1w).detach(), t1w)."""
    d_real = disc(batch["t2w"], batch["t1w"])
    d_fake = disc(gen(batch["t1w"]).detach(), batch["t1w"])
    return (objective(d_real, one_sided, kind) + objective(d_fake, 0.0, kind)) / 2


# ---- bf16 storage -----------------------------------------------------------------------------------------------------
def rb(t):
    return t.to(torch.bfloat16).float()


def bf16_step(disc: CondDiscriminator, x, target: float, kind: str = "bce", eps=1e-5, slope=0.2):
    """oracle/bf16_emul.disc_step's contract for a CondDiscriminator with either head and any objective: fp32
    arithmetic; the raw conv outputs z_i, the activations a_0..a_2, the gradients dz_i and g_a_0..2 and the dense
    layers' weights are rounded to bf16 where the HIP path stores them; the first layer's weights, the last activation,
    the head and every statistic stay fp32.  x: the (N, 2, ...) fp32 input, channel 0 the image.
    Returns dict(validity, loss, zs, grad_x (N, 2, ...), grads{name: tensor})."""
    dims = x.dim() - 2
    conv = _conv(dims)
    convs = [disc.model_conv[i] for i in (0, 3, 6, 9)]
    bns = [disc.model_conv[i] for i in (1, 4, 7, 10)]
    red = [0] + list(range(2, 2 + dims))
    shp = [1, -1] + [1] * dims
    a, saved = x, []
    for i, (cv, bn) in enumerate(zip(convs, bns)):
        w = cv.weight.detach() if i == 0 else rb(cv.weight.detach())
        z32 = conv(a, w, cv.bias.detach(), stride=cv.stride)
        mean, var = z32.mean(red), z32.var(red, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + eps)
        scale = bn.weight.detach() * invstd
        shift = bn.bias.detach() - mean * scale
        z = rb(z32)
        y = z * scale.view(shp) + shift.view(shp)
        act = torch.where(y < 0, y * slope, y)
        saved.append((a, w, z, y, mean, invstd, scale, cv))
        a = act if i == 3 else rb(act)
    head = disc.model_head[0] if disc.head == "markovian" else disc.model_linear[1]
    a_req = a.clone().requires_grad_(True)
    hw, hb = head.weight.detach().clone().requires_grad_(True), head.bias.detach().clone().requires_grad_(True)
    logit = conv(a_req, hw, hb) if disc.head == "markovian" else a_req.flatten(1) @ hw.t() + hb
    validity = logit if disc.logits else torch.sigmoid(logit)
    loss = objective(validity, target, kind)
    g, ghw, ghb = torch.autograd.grad(loss, (a_req, hw, hb))
    hname = "model_head.0" if disc.head == "markovian" else "model_linear.1"
    grads = {hname + ".weight": ghw, hname + ".bias": ghb}
    for i in range(3, -1, -1):
        a_in, w, z, y, mean, invstd, scale, cv = saved[i]
        gy = torch.where(y < 0, g * slope, g)
        zh = (z - mean.view(shp)) * invstd.view(shp)
        cnt = z.numel() / z.shape[1]
        s1, s2 = gy.sum(red), (gy * zh).sum(red)
        grads[f"model_conv.{3 * i + 1}.weight"], grads[f"model_conv.{3 * i + 1}.bias"] = s2, s1
        dz = rb(scale.view(shp) * (gy - (s1 / cnt).view(shp) - zh * (s2 / cnt).view(shp)))
        grads[f"model_conv.{3 * i}.bias"] = dz.sum(red)
        ar, wr = a_in.clone().requires_grad_(True), w.clone().requires_grad_(True)
        ga, gw = torch.autograd.grad(conv(ar, wr, None, stride=cv.stride), (ar, wr), dz)
        grads[f"model_conv.{3 * i}.weight"] = gw
        g = ga if i == 0 else rb(ga)
    return dict(validity=validity.detach(), loss=loss.detach(), zs=[s[2] for s in saved], grad_x=g, grads=grads)
