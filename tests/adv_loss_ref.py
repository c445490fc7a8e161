"""TEST INFRASTRUCTURE (imported by tests/ only, never by the product path).

Float64 restatement of the two adversarial objectives computed on logits (include/mpgan_hip.h) with their
closed-form gradients, a float32 restatement of the probability chain they stand beside (Sigmoid -> bce_forward ->
bce_backward -> sigmoid_backward, formulas from the header), the inputs the kernel tests share, and the trainer's step
restated on logits.  The closed forms are pinned to autograd in tests/test_adv_loss_host.py."""
import functools

import torch
import torch.nn.functional as F

EPS = 2.0 ** -23
KINDS = ("bce_logits", "lsgan")


def sigmoid(z):
    """sigma(z) with exp of a non-positive argument only."""
    e = torch.exp(-z.abs())
    return torch.where(z >= 0, torch.ones_like(e), e) / (1 + e)


def objective(kind, z, t):
    """(loss, dloss/dz) of the mean objective over all elements; z and t of one shape, computed in their dtype."""
    n = z.numel()
    if kind == "bce_logits":
        term = z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
        return term.sum() / n, (sigmoid(z) - t) / n
    if kind == "lsgan":
        d = z - t
        return (d * d).sum() / n, 2 * d / n
    raise ValueError(kind)


def torch_objective(kind, z, t):
    """The torch function each kind restates."""
    return F.binary_cross_entropy_with_logits(z, t) if kind == "bce_logits" else F.mse_loss(z, t)


def prob_chain_f32(z, t):
    """(loss, dloss/dlogit) of the probability chain in float32, operation by operation as the header states it."""
    z, t = z.float(), t.float()
    n = z.numel()
    one = torch.ones((), dtype=torch.float32)
    p = one / (one + torch.exp(-z))
    loss = (-(t * torch.log(p).clamp(min=-100.0) + (one - t) * torch.log(one - p).clamp(min=-100.0))).sum() / n
    dprob = (p - t) / ((one - p) * p).clamp(min=1e-12) * (one / n)
    return loss, dprob * (one - p) * p


# logit -100 and -88 sit where the cycle 0, 0.9, 1 gives target 1; 2.1972246 (sigma ~ 0.9) where it gives 0.9
SPECIAL_LOGITS = (0.0, 2.1972246, -100.0, -0.0, 100.0, -88.0, 30.0, -30.0, 88.0, 1e-8)
SIZES = (1, 3, 63, 64, 65, 257, 1025, 1797, 70304)


@functools.lru_cache(maxsize=None)
def inputs(n, seed=11):
    """(logits, targets) as float32 CPU tensors: uniform in +-12, the first entries replaced by SPECIAL_LOGITS; targets
    cycle 0, 0.9, 1.  Shared by the tests and never modified."""
    gen = torch.Generator().manual_seed(seed + n)
    z = (torch.rand(n, generator=gen) * 2 - 1) * 12
    k = min(n, len(SPECIAL_LOGITS))
    z[:k] = torch.tensor(SPECIAL_LOGITS[:k])
    t = torch.tensor([0.0, 0.9, 1.0]).repeat(n // 3 + 1)[:n].clone()
    return z, t


@functools.lru_cache(maxsize=None)
def reference(kind, n):
    """(loss, grad) of inputs(n) in float64."""
    z, t = inputs(n)
    return objective(kind, z.double(), t.double())


# ---- the discriminator up to its logits, and the trainer's step on them -------------------------------------------
def disc_logits(disc, x):
    """A restated discriminator (oracle.refmodel.Discriminator, map_head_ref.MarkovianDiscriminator) without its final
    Sigmoid."""
    head = disc.model_head if hasattr(disc, "model_head") else disc.model_linear
    return head[:-1](disc.model_conv(x))


def _labels(d, value, head):
    return torch.full_like(d, value) if head == "markovian" else torch.full((d.shape[0], 1), value, dtype=d.dtype)


def step_losses_g(gen, disc, batch, kind, head):
    """The generator branch of GAN.training_step (code/GAN/GAN_final.py:254-273) with the objective on D's logits."""
    fake = gen(batch["t1w"])
    d = disc_logits(disc, fake)
    g_adv = objective(kind, d, _labels(d, 1.0, head))[0]
    g_rec = F.l1_loss(fake, batch["t2w"])
    return {"g_adv_loss": g_adv, "g_recon_loss": g_rec, "g_loss": g_adv + g_rec}


def step_loss_d(gen, disc, batch, kind, head, one_sided=0.9):
    """The discriminator branch (code/GAN/GAN_final.py:276-296) likewise."""
    d_real = disc_logits(disc, batch["t2w"])
    d_fake = disc_logits(disc, gen(batch["t1w"]).detach())
    return (objective(kind, d_real, _labels(d_real, one_sided, head))[0]
            + objective(kind, d_fake, _labels(d_fake, 0.0, head))[0]) / 2
