"""The reference's GAN LightningModule without Lightning: same methods, same
two-optimizer step (code/GAN/GAN_final.py:212-317; Lightning 1.2.1 loop restated
in SURVEY.md Appendix B), every FLOP in HIP kernels.
"""
from __future__ import annotations

import contextlib
import inspect
import re
import types
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import ops
from .augment import DiffAugment, PairAugment, affine_options, parse_policy
from .losses import EdgeLoss, ForegroundL1Loss, ForegroundSSIMLoss, GlobalMutualInformationLoss, SSIMLoss
from .preprocess import check_threshold
from .networks import CasNetGenerator, Discriminator, _EngineModule


# --------------------------------------------------------------------------
# loss hooks (autograd nodes around the loss kernels)
# --------------------------------------------------------------------------
class _BCEFn(torch.autograd.Function):
    """F.binary_cross_entropy(y_hat, y) (mean), log clamped at -100."""

    @staticmethod
    def forward(ctx, y_hat, y):
        p = y_hat.contiguous()
        t = y.contiguous()
        loss = torch.empty((), device=p.device)
        ops.bce_forward(p, t, loss)
        ctx.save_for_backward(p, t)
        return loss

    @staticmethod
    def backward(ctx, gout):
        p, t = ctx.saved_tensors
        dprob = torch.empty_like(p)
        ops.bce_backward(p, t, gout.contiguous(), dprob)
        return dprob, None


class _L1Fn(torch.autograd.Function):
    """F.l1_loss(y_hat, y) (mean); backward = gout * sign(y_hat - y) / numel."""

    @staticmethod
    def forward(ctx, y_hat, y):
        a, b = y_hat.contiguous(), y.contiguous()
        loss = torch.empty((), device=a.device)
        part = torch.empty(ops.l1_partials(), device=a.device)
        grad = torch.empty_like(a) if (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) else None
        ops.l1_loss(a, b, part, loss, grad, 1.0)
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, gout):
        g = torch.empty_like(ctx.grad)          # a fresh tensor: a second backward (retain_graph) sees the unscaled sign
        ops.scale_by_device_scalar(ctx.grad, gout.contiguous(), g)
        gb = ops.axpby(g, -1.0, None, 0.0, torch.empty_like(g)) if ctx.needs_input_grad[1] else None   # d/dy = -d/dy_hat
        return (g if ctx.needs_input_grad[0] else None), gb


class _AdvLogitFn(torch.autograd.Function):
    """An objective on the discriminator's logits (ops.adv_loss: "bce_logits" = F.binary_cross_entropy_with_logits,
    "lsgan" = F.mse_loss), mean; dL/dlogit is written by the forward launch and the backward scales it by gout."""

    @staticmethod
    def forward(ctx, y_hat, y, kind):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("adversarial_loss: the target is a label, no gradient is offered for it")
        z, t = y_hat.contiguous(), y.contiguous()
        loss = torch.empty((), device=z.device)
        part = torch.empty(ops.adv_loss_partials(z.numel()), device=z.device, dtype=torch.float64)
        grad = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        ops.adv_loss(z, t, kind, part, loss, grad)
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, gout):
        g = torch.empty_like(ctx.grad)          # a fresh tensor, as in _L1Fn
        ops.scale_by_device_scalar(ctx.grad, gout.contiguous(), g)
        return g, None, None


class _AxpbyFn(torch.autograd.Function):
    """alpha*a + beta*b on device scalars (the loss sums of training_step) through the library's own
    pointwise kernel, so that no torch elementwise kernel sits on the step path."""

    @staticmethod
    def forward(ctx, a, alpha, b, beta):
        ctx.alpha, ctx.beta = alpha, beta
        out = torch.empty_like(a)
        ops.axpby(a.contiguous(), alpha, b.contiguous(), beta, out)
        return out

    @staticmethod
    def backward(ctx, gout):
        gout = gout.contiguous()
        ga = ops.axpby(gout, ctx.alpha, None, 0.0, torch.empty_like(gout)) if ctx.needs_input_grad[0] else None
        gb = ops.axpby(gout, ctx.beta, None, 0.0, torch.empty_like(gout)) if ctx.needs_input_grad[2] else None
        return ga, None, gb, None


def scalar_axpby(a, alpha, b, beta):
    return _AxpbyFn.apply(a, float(alpha), b, float(beta))


ADV_LOSSES = ("bce", "bce_logits", "lsgan")


def adversarial_loss(y_hat, y, kind="bce"):
    """code/GAN/GAN_final.py:244-245 (kind="bce": y_hat holds probabilities).  kind="bce_logits" | "lsgan": y_hat holds
    the logits of a Discriminator(output="logit"), see _AdvLogitFn and DESIGN.md 7d."""
    if kind == "bce":
        return _BCEFn.apply(y_hat, y)
    if kind not in ADV_LOSSES:
        raise ValueError(f"adversarial_loss: kind must be one of {ADV_LOSSES}, got {kind!r}")
    return _AdvLogitFn.apply(y_hat, y, kind)


def reconstruction_loss(y_hat, y):
    """code/GAN/GAN_final.py:247-248."""
    return _L1Fn.apply(y_hat, y)


@contextlib.contextmanager
def eval_modes(*modules):
    """Every sub-module of `modules` in eval mode inside the block (what Lightning does around validation_step /
    test_step), each one's own previous mode restored afterwards."""
    was = [(m, m.training) for top in modules for m in top.modules()]
    try:
        for top in modules:
            top.eval()
        yield
    finally:
        for m, flag in was:
            m.training = flag


# --------------------------------------------------------------------------
# optimiser
# --------------------------------------------------------------------------
class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam(lr, betas, eps=1e-8, weight_decay=0) as ONE kernel over
    the network's flat parameter buffer (code/GAN/GAN_final.py:306-307).
    `grad_scale` (e.g. 1/world_size after a sum all-reduce) is applied on load.

    Opt-in, on the same pass over the flat buffer; with none of them given step() is the one
    ops.adam_step launch:
      max_grad_norm      torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) in front of the step: the norm of
                         grad_scale * flat_grad and its coefficient stay on the device (no host sync)
      measure_grad_norm  the norm alone; either way `opt.grad_norm` is the device scalar of the pre-clip norm
      ema                a twin of `net` (same class and layout) whose flat parameters become
                         lerp(ema, p_new, 1 - ema_decay_at(step, ema_decay, ema_warmup)) inside the Adam kernel, and
                         whose buffers follow net's in one more launch (num_batches_tracked is copied)"""

    def __init__(self, net: _EngineModule, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, *, max_grad_norm=None,
                 measure_grad_norm: bool = False, ema: Optional[_EngineModule] = None, ema_decay: float = 0.999,
                 ema_warmup: bool = True):
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"FusedAdam: max_grad_norm must be > 0 or None, got {max_grad_norm!r}")
        if ema is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"FusedAdam: ema_decay must be in [0, 1), got {ema_decay!r}")
        if ema is not None and ema is net:
            raise ValueError("FusedAdam: ema must be a twin of net, not net itself")
        self.net = net
        super().__init__(list(net.parameters()), dict(lr=lr, betas=betas, eps=eps))
        self._version = -1
        self.step_count = 0
        self.grad_scale = 1.0
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.measure_grad_norm = bool(measure_grad_norm)
        self.ema, self.ema_decay, self.ema_warmup = ema, float(ema_decay), bool(ema_warmup)
        self.grad_norm: Optional[torch.Tensor] = None    # device scalar: the last step's pre-clip norm
        self._norm_out = self._norm_ws = None
        self._norm_numel = -1
        self._ema_key = None
        self._buf_slots = self._buf_key = self._buf_table = None
        self._buf_max = 0

    def _state(self):
        store = self.net.store
        if self._version != store.version:
            # the flat layout is a function of the module tree only: a re-created store (.to()/.cuda()/.float()
            # after the first step) keeps the moments; a different layout restarts Adam as a whole
            old_m, old_v = getattr(self, "exp_avg", None), getattr(self, "exp_avg_sq", None)
            self.exp_avg = torch.zeros_like(store.flat)
            self.exp_avg_sq = torch.zeros_like(store.flat)
            if old_m is not None and old_m.numel() == store.flat.numel():
                self.exp_avg.copy_(old_m)
                self.exp_avg_sq.copy_(old_v)
            elif old_m is not None:
                import warnings
                warnings.warn("FusedAdam: parameter layout changed; moments and step count reset")
                self.step_count = 0
            self._version = store.version
        return store

    # torch.optim.Adam's state_dict format (per-parameter step / exp_avg / exp_avg_sq), so that a
    # Lightning-style 'optimizer_states' entry round-trips and a torch Adam state loads here
    def state_dict(self):
        store = self._state()
        params = list(self.net.parameters())
        state = {}
        if self.step_count > 0:
            for i, p in enumerate(params):
                o = store.offset(p)
                state[i] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": self.exp_avg[o:o + p.numel()].view(p.shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + p.numel()].view(p.shape).clone()}
        g = self.param_groups[0]
        return {"state": state,
                "param_groups": [{"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": 0,
                                  "amsgrad": False, "params": list(range(len(params)))}]}

    def load_state_dict(self, sd):
        store = self._state()
        params = list(self.net.parameters())
        g = sd["param_groups"][0]
        # validate everything before touching the moments: a checkpoint of a differently shaped network must leave
        # this optimizer as it was
        names = [n for n, _ in self.net.named_parameters()]
        for i, st in sd["state"].items():
            if not 0 <= int(i) < len(params):
                raise ValueError(f"FusedAdam.load_state_dict: state entry {i} but the network has {len(params)} parameters")
            p = params[int(i)]
            for key in ("exp_avg", "exp_avg_sq"):
                if key not in st or st[key].numel() != p.numel():
                    got = tuple(st[key].shape) if key in st else None
                    raise ValueError(f"FusedAdam.load_state_dict: {key} of parameter {int(i)} ({names[int(i)]}, shape "
                                     f"{tuple(p.shape)}) has shape {got}")
        self.param_groups[0].update(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"])
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.step_count = 0
        for i, st in sd["state"].items():
            p = params[int(i)]
            o = store.offset(p)
            self.exp_avg[o:o + p.numel()].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + p.numel()].copy_(st["exp_avg_sq"].reshape(-1))
            self.step_count = max(self.step_count, int(float(st["step"])))

    def zero_grad(self, set_to_none: bool = False):
        store = self._state()
        store.flat_grad.zero_()
        store.attach_grads()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        store = self._state()
        g = self.param_groups[0]
        ema_flat = self._ema_flat(store) if self.ema is not None else None     # ValueError before anything is stepped
        self.step_count += 1
        want_norm = self.max_grad_norm is not None or self.measure_grad_norm
        if not want_norm and self.ema is None:
            ops.adam_step(store.flat, store.flat_grad, self.exp_avg, self.exp_avg_sq, g["lr"], g["betas"][0],
                          g["betas"][1], g["eps"], self.step_count, self.grad_scale)
            store.touch()                           # the packed weights are stale now
            return loss
        coef = None
        if want_norm:
            out2 = self._norm_buffers(store)
            ops.grad_norm(store.flat_grad, out2, self._norm_ws, self.grad_scale, self.max_grad_norm or 0.0)
            self.grad_norm = out2[0]
            coef = out2[1:2] if self.max_grad_norm is not None else None
        w = 1.0 - ema_decay_at(self.step_count, self.ema_decay, self.ema_warmup) if self.ema is not None else 0.0
        ops.adam_step_ex(store.flat, store.flat_grad, self.exp_avg, self.exp_avg_sq, g["lr"], g["betas"][0],
                         g["betas"][1], g["eps"], self.step_count, self.grad_scale, coef=coef, ema=ema_flat,
                         ema_weight=w)
        store.touch()
        if self.ema is not None:
            table, n, max_elems = self._buffer_table()
            ops.ema_buffers(table, n, max_elems, w)
            self.ema.store.touch()                  # the twin's packed weights are stale too
        return loss

    def _norm_buffers(self, store):
        dev, numel = store.flat.device, store.flat_grad.numel()
        if self._norm_out is None or self._norm_out.device != dev or self._norm_numel != numel:
            self._norm_out = torch.zeros(2, device=dev)
            self._norm_ws = torch.empty(ops.grad_norm_workspace(numel) // 8, device=dev, dtype=torch.float64)
            self._norm_numel = numel
        return self._norm_out

    def _ema_flat(self, store):
        """The twin's flat buffer, after checking (once per pair of stores) that it has the live layout."""
        estore = self.ema.store
        k = self._ema_key
        if k is None or k[0] is not store or k[1] != store.version or k[2] is not estore or k[3] != estore.version:
            live, twin = list(self.net.parameters()), list(self.ema.parameters())
            same = (len(live) == len(twin) and estore.flat.numel() == store.flat.numel()
                    and estore.flat.device == store.flat.device
                    and all(p.shape == q.shape and store.offset(p) == estore.offset(q) for p, q in zip(live, twin)))
            if not same:
                raise ValueError("FusedAdam: the ema module's flat parameter layout differs from the network's "
                                 f"({estore.flat.numel()} vs {store.flat.numel()} floats): it must be a twin built "
                                 "with the same constructor arguments")
            for q in twin:                          # the twin is never trained: no gradient views on it
                q.grad = None
            self._ema_key = (store, store.version, estore, estore.version)
        return estore.flat

    def _buffer_table(self):
        """Device table [src_ptr, dst_ptr, numel, kind] of ops.ema_buffers over zip(net.buffers(), ema.buffers()),
        rebuilt when either store or any buffer's storage changed.  The per-step check is one data_ptr() per buffer
        through the owning modules' _buffers dicts (found once per pair of stores: walking ~1000 modules twice per
        step would cost more host time than the step's kernels take)."""
        if self._buf_slots is None or self._buf_slots[0] is not self._ema_key:
            slots = [[(m._buffers, k) for m in net.modules() for k, t in m._buffers.items() if t is not None]
                     for net in (self.net, self.ema)]
            if len(slots[0]) != len(slots[1]):
                raise ValueError(f"FusedAdam: the ema module has {len(slots[1])} buffers, the network {len(slots[0])}")
            self._buf_slots = (self._ema_key, slots[0], slots[1])
            self._buf_key = None
        live = [d[k] for d, k in self._buf_slots[1]]
        twin = [d[k] for d, k in self._buf_slots[2]]
        key = [t.data_ptr() for t in live] + [t.data_ptr() for t in twin]
        if key != self._buf_key:
            rows = []
            for a, b in zip(live, twin):
                if a.shape != b.shape or a.dtype != b.dtype or not (a.is_contiguous() and b.is_contiguous()):
                    raise ValueError(f"FusedAdam: buffer mismatch between the network and its ema twin: "
                                     f"{tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}")
                if a.dtype not in (torch.float32, torch.int64):
                    raise ValueError(f"FusedAdam: no EMA for a buffer of dtype {a.dtype}")
                if a.numel() > 0:
                    rows.append([a.data_ptr(), b.data_ptr(), a.numel(), 0 if a.dtype == torch.float32 else 1])
            self._buf_table = (torch.tensor(rows, dtype=torch.int64, device=self.net.store.flat.device)
                               if rows else None)
            self._buf_max = max((r[2] for r in rows), default=0)
            self._buf_key = key
        n = 0 if self._buf_table is None else self._buf_table.shape[0]
        return self._buf_table, n, self._buf_max


def ema_decay_at(step: int, decay: float, warmup: bool = True) -> float:
    """The EMA decay of optimiser step `step` (1-based): min(decay, (1 + t) / (10 + t)) with t = step - 1 when
    `warmup` is set (0.1 at the first step, so an average started from the initial weights forgets them quickly),
    else `decay`."""
    if not warmup:
        return float(decay)
    t = max(int(step) - 1, 0)
    return min(float(decay), (1.0 + t) / (10.0 + t))


# --------------------------------------------------------------------------
# the GAN module
# --------------------------------------------------------------------------
def _pair_augment_module(options: Optional[dict]) -> Optional[PairAugment]:
    """GAN(pair_augment=...): None, or the keywords of augment.PairAugment (its generator is the GAN's aug_generator)."""
    if options is None:
        return None
    known = [k for k in inspect.signature(PairAugment.__init__).parameters if k not in ("self", "generator")]
    unknown = sorted(set(options) - set(known)) if isinstance(options, dict) else None
    if unknown is None or unknown:
        raise ValueError(f"pair_augment: a dict of PairAugment keywords {known}, got {options!r}")
    return PairAugment(**options)


class _HParams(types.SimpleNamespace):
    """GAN.hparams.  `adv_loss` reads "bce" unless the constructor was given another objective, and only then is it an
    entry of vars(hparams): a default GAN lists exactly the hyper-parameters it listed before the option existed.
    `conditional` likewise reads False unless the constructor was given True, and `diff_augment` "" (with
    `diff_augment_fill` 0.0) unless it was given a policy, `diff_augment_affine` None unless that policy has the word
    "affine" (then the keywords its maps are drawn with), and `ema_decay` 0.0 / `ema_warmup` True / `grad_clip` 0.0 /
    `log_grad_norm` False unless the constructor was given another value, and `pair_augment` None unless it was given
    the keywords of a PairAugment."""
    adv_loss = "bce"
    conditional = False
    diff_augment = ""
    diff_augment_fill = 0.0
    diff_augment_affine = None
    ema_decay = 0.0
    ema_warmup = True
    grad_clip = 0.0
    log_grad_norm = False
    pair_augment = None


class GAN(nn.Module):
    """code/GAN/GAN_final.py:212-317.  `training_step(batch, batch_idx,
    optimizer_idx)` has the reference's body; `fit_batch` is Lightning's
    per-batch loop (toggle_optimizer -> zero_grad -> training_step -> backward
    -> optimizer.step for optimizer 0 (G) then 1 (D))."""

    def __init__(self, channels, width, height, depth=None, latent_dim: int = 100, d_lr: float = 0.0005,
                 g_lr: float = 0.0005, b1: float = 0.5, b2: float = 0.999, batch_size: int = 64, example_data=None,
                 one_sided_label_value=0.9, *, dimensions: Optional[int] = None, norm: str = "batch",
                 n_unet_blocks: int = 6, unet_channels=(16, 32, 64, 128), unet_strides=(2, 2, 2), device="cuda",
                 storage_dtype: str = "f32", mi_weight: float = 0.0, mi_bins: int = 23,
                 ssim_weight: float = 0.0, d_head: str = "linear", adv_loss: str = "bce", conditional: bool = False,
                 diff_augment: str = "", diff_augment_fill: float = 0.0, ema_decay: float = 0.0,
                 ema_warmup: bool = True, grad_clip: float = 0.0, log_grad_norm: bool = False,
                 pair_augment: Optional[dict] = None, edge_weight: float = 0.0, edge_eps: float = 1e-6,
                 fg_weight: float = 0.0, fg_threshold="otsu", fg_ssim_weight: float = 0.0,
                 diff_augment_affine: Optional[dict] = None, **kwargs):
        super().__init__()
        if adv_loss not in ADV_LOSSES:
            raise ValueError(f"adv_loss must be one of {ADV_LOSSES}, got {adv_loss!r}")
        if mi_weight < 0:
            raise ValueError(f"mi_weight must be >= 0, got {mi_weight!r}")
        if ssim_weight < 0:
            raise ValueError(f"ssim_weight must be >= 0, got {ssim_weight!r}")
        if edge_weight < 0:
            raise ValueError(f"edge_weight must be >= 0, got {edge_weight!r}")
        if not fg_weight >= 0:
            raise ValueError(f"fg_weight must be >= 0, got {fg_weight!r}")
        if not fg_ssim_weight >= 0:
            raise ValueError(f"fg_ssim_weight must be >= 0, got {fg_ssim_weight!r}")
        if isinstance(fg_threshold, torch.Tensor):
            raise ValueError('fg_threshold must be "otsu" or a finite number, got a tensor')
        check_threshold(fg_threshold, "GAN: fg_threshold")
        if not 0.0 <= ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay!r}")
        if not grad_clip >= 0:
            raise ValueError(f"grad_clip must be >= 0, got {grad_clip!r}")
        aug_ops = parse_policy(diff_augment)         # ValueError on an unknown policy word, before anything is built
        aug_affine = affine_options(diff_augment, diff_augment_affine)     # likewise: options without the word, an unknown key
        pair_module = _pair_augment_module(pair_augment)    # likewise on an unknown keyword or a value out of range
        if dimensions is None:
            dimensions = 3 if depth is not None else 2
        self.hparams = _HParams(latent_dim=latent_dim, g_lr=g_lr, d_lr=d_lr, b1=b1, b2=b2,
                                batch_size=batch_size, one_sided_label_value=one_sided_label_value, d_head=d_head)
        if adv_loss != _HParams.adv_loss:
            self.hparams.adv_loss = adv_loss
        if conditional:
            self.hparams.conditional = True
        if aug_ops:
            self.hparams.diff_augment = str(diff_augment)
            self.hparams.diff_augment_fill = float(diff_augment_fill)
        if aug_affine is not None:
            self.hparams.diff_augment_affine = dict(aug_affine)
        for name, value in (("ema_decay", float(ema_decay)), ("ema_warmup", bool(ema_warmup)),
                            ("grad_clip", float(grad_clip)), ("log_grad_norm", bool(log_grad_norm))):
            if value != getattr(_HParams, name):
                setattr(self.hparams, name, value)
        if pair_module is not None:
            self.hparams.pair_augment = dict(pair_augment)
        data_shape = (channels, width, height) + ((depth,) if dimensions == 3 else ())
        # storage_dtype="bf16" is config C5: the discriminator stores its activations in bf16 and the generator's
        # matrix products take bf16 operands (fp32 storage: its launches are matrix-bound, not byte-bound)
        self.generator = CasNetGenerator(data_shape, n_unet_blocks, dimensions=dimensions, norm=norm,
                                         channels=unet_channels, strides=unet_strides, device=device,
                                         matmul_dtype="bf16" if storage_dtype == "bf16" else "f32")
        # adv_loss="bce" is the reference's objective on the Sigmoid's output; the other two are computed on the logits
        # (their gradient does not vanish when the discriminator wins), which the discriminator then returns.
        # conditional=True is pix2pix's discriminator: it judges the (T1, T2) PAIR, D(cat(t2w, t1w))
        self.discriminator = Discriminator(data_shape, dimensions=dimensions, device=device,
                                           storage_dtype=storage_dtype, head=d_head,
                                           output="prob" if adv_loss == "bce" else "logit", conditional=conditional)
        # ema_decay > 0: the averaged generator (the one to score and ship), a twin that opt_g's step
        # writes; it stays in eval mode, takes no gradient, and its keys are generator_ema.*.  With the default 0.0
        # there is no module, no state_dict key and no launch.  (Built last: the live networks draw the same initial
        # weights from a seed with or without it.)
        self.generator_ema = None
        if ema_decay > 0:
            self.generator_ema = CasNetGenerator(data_shape, n_unet_blocks, dimensions=dimensions, norm=norm,
                                                 channels=unet_channels, strides=unet_strides, device=device,
                                                 matmul_dtype="bf16" if storage_dtype == "bf16" else "f32")
            self.generator_ema.requires_grad_(False)
            self.generator_ema.eval()
            self.reset_ema()
        # opt-in auxiliary generator loss (not in the reference's trainer): mi_weight * (-MI(G(t1w), t2w)) from Parzen
        # windows over the tanh output's range; with the default 0 no launch and no logged name is added
        self.mi_weight = float(mi_weight)
        self.mi_loss = (GlobalMutualInformationLoss(mi_bins, value_range=(-1.0, 1.0)) if self.mi_weight > 0 else None)
        # likewise ssim_weight * (1 - SSIM(G(t1w), t2w)), the loss form of the figure metrics.ssim scores a volume with
        self.ssim_weight = float(ssim_weight)
        self.ssim_loss = SSIMLoss(value_range=(-1.0, 1.0)) if self.ssim_weight > 0 else None
        # and edge_weight * mean |m(G(t1w)) - m(t2w)| over the Sobel edge-magnitude maps, Ea-GAN's generator term
        # (DESIGN.md 7i); like every generator term it sees the pair fit_batch hands over, never DiffAugment's output
        self.edge_weight = float(edge_weight)
        self.edge_loss = EdgeLoss(eps=edge_eps) if self.edge_weight > 0 else None
        # and fg_weight * mean |G(t1w) - t2w| over the foreground of t2w, t2w > fg_threshold ("otsu": found per image on
        # the device, no host sync): the anatomy weighted above the air around it
        self.fg_weight = float(fg_weight)
        self.fg_loss = ForegroundL1Loss(fg_threshold) if self.fg_weight > 0 else None
        # and fg_ssim_weight * (1 - SSIM(G(t1w), t2w)) over the windows whose centre lies in that foreground (DESIGN.md
        # 7l): the whole-image SSIM is mostly air, whose flat windows score 1 and give the generator no signal
        self.fg_ssim_weight = float(fg_ssim_weight)
        self.fg_ssim_loss = ForegroundSSIMLoss(fg_threshold) if self.fg_ssim_weight > 0 else None
        # the active terms as (log name, weight, module), in the order _add_generator_terms adds them to g_loss
        self._generator_terms = [(name, weight, module) for name, weight, module in (
            ("g_mi_loss", self.mi_weight, self.mi_loss), ("g_ssim_loss", self.ssim_weight, self.ssim_loss),
            ("g_edge_loss", self.edge_weight, self.edge_loss), ("g_fg_loss", self.fg_weight, self.fg_loss),
            ("g_fg_ssim_loss", self.fg_ssim_weight, self.fg_ssim_loss)) if module is not None]
        # opt-in differentiable augmentation of everything D sees in training_step (augment.py); with the
        # default "" there is no module and no launch.  aug_generator: a torch.Generator on the images' device, or None
        # for torch's global one (data-parallel runs: every rank seeds its own, or all ranks draw the same parameters)
        self.augment = DiffAugment(diff_augment, fill=diff_augment_fill, affine=diff_augment_affine) if aug_ops else None
        self.aug_generator: Optional[torch.Generator] = None
        # opt-in augmentation of the training pair itself (augment.PairAugment): fit_batch warps t1w and
        # t2w under one draw, with noise on the input, before the G step; both steps see that pair.  It draws from
        # aug_generator too, ahead of the step's DiffAugment draws.  With the default None there is no module and no launch.
        self.pair_augment = pair_module
        self.logged: Dict[str, torch.Tensor] = {}
        self.ddp = None  # set by parallel.DataParallelGAN

    def forward(self, x):
        return self.generator(x)

    def reset_ema(self):
        """Restart the average from the live generator: its weights and buffers copied into generator_ema."""
        if self.generator_ema is None:
            raise RuntimeError("reset_ema: this GAN was built without ema_decay")
        self.generator_ema.load_state_dict(self.generator.state_dict())

    def train(self, mode: bool = True):
        super().train(mode)
        if self.generator_ema is not None:
            self.generator_ema.eval()               # the averaged generator is only ever evaluated
        return self

    def adversarial_loss(self, y_hat, y):
        return adversarial_loss(y_hat, y, kind=self.hparams.adv_loss)

    def reconstruction_loss(self, y_hat, y):
        return reconstruction_loss(y_hat, y)

    def _labels(self, validity, value: float):
        """The target of one discriminator output: (B, 1) as in the reference; with d_head="markovian" the shape of
        the validity map, every verdict getting the same label."""
        if self.hparams.d_head == "markovian":
            return torch.full_like(validity, float(value))
        return torch.full((validity.shape[0], 1), float(value), device=validity.device, dtype=validity.dtype)

    def _judge(self, images, t1w_images, augment: bool = False):
        """The discriminator's verdict on `images`; a conditional one sees the T1 input they belong to beside them.
        augment (training_step only) and a diff_augment policy: one fresh draw T per call, D sees T(images) and the
        condition under T's spatial ops; the gradient of `images` flows back through T."""
        cond = t1w_images.detach() if self.hparams.conditional else None
        if augment and self.augment is not None:
            self.augment.generator = self.aug_generator
            if cond is None:
                images = self.augment(images)
            else:
                images, cond = self.augment(images, cond)
        if cond is not None:
            return self.discriminator(images, cond)
        return self.discriminator(images)

    def log(self, name, value, **kw):
        """Lightning's self.log: scalars stay on the device (no per-step sync)."""
        self.logged[name] = value.detach()

    def _add_generator_terms(self, g_loss, generated_imgs, t2w_images, terms: dict):
        """g_loss plus weight * term for every opt-in generator term, one scalar_axpby each in the list's order (that
        order is the bits of g_loss); the terms' values go into `terms` under their log names."""
        for name, weight, module in self._generator_terms:
            terms[name] = module(generated_imgs, t2w_images)
            g_loss = scalar_axpby(g_loss, 1.0, terms[name], weight)
        return g_loss

    def training_step(self, batch, batch_idx, optimizer_idx):
        t1w_images, t2w_images = batch["t1w"], batch["t2w"]
        if optimizer_idx == 0:                      # GAN_final.py:254-273
            generated_imgs = self(t1w_images)
            self.generated_imgs = generated_imgs
            d_fake = self._judge(generated_imgs, t1w_images, augment=True)
            g_adv_loss = self.adversarial_loss(d_fake, self._labels(d_fake, 1.0))
            self.log("g_adv_loss", g_adv_loss)
            g_recon_loss = self.reconstruction_loss(generated_imgs, t2w_images)
            self.log("g_recon_loss", g_recon_loss)
            g_loss = scalar_axpby(g_adv_loss, 1.0, g_recon_loss, 1.0)
            terms = {}
            g_loss = self._add_generator_terms(g_loss, generated_imgs, t2w_images, terms)
            for name, value in terms.items():
                self.log(name, value)
            self.log("g_loss", g_loss)
            return g_loss
        if optimizer_idx == 1:                      # GAN_final.py:276-296
            # (D(real) and G(t1w) are independent, and rounds 1-3 carried an opt-in mode that ran the generator's
            #  forward on a high-priority stream underneath D(real).  It measured nothing beyond run-to-run spread
            #  -- 59.1 vs 58.6 ms at C3, 174.3 vs 175.8 ms at C5 -- while stretching D's kernels up to 3x, and its first
            #  use in a process once ended in a host SIGSEGV inside hipStreamWaitEvent on that stream: removed in
            #  round 4)
            d_real = self._judge(t2w_images, t1w_images, augment=True)
            real_loss = self.adversarial_loss(d_real, self._labels(d_real, self.hparams.one_sided_label_value))
            generated = self(t1w_images).detach()
            d_fake = self._judge(generated, t1w_images, augment=True)
            fake_loss = self.adversarial_loss(d_fake, self._labels(d_fake, 0.0))
            d_loss = scalar_axpby(real_loss, 0.5, fake_loss, 0.5)
            self.log("d_loss", d_loss)
            return d_loss

    def validation_step(self, batch, batch_idx):
        """Lightning's validation hook (the reference builds a val_dataloader, GAN_final.py:427-431, and defines no
        step for it): the losses of training_step (:250-296) on a held-out batch from ONE generator pass, with generator
        and discriminator in eval mode (running-statistics BatchNorm) under no_grad -- no parameter, buffer, gradient or
        optimizer state is touched.  Logs and returns val_g_adv_loss, val_g_recon_loss, val_g_loss, val_d_loss as
        device scalars (no host sync); with mi_weight > 0 also val_g_mi_loss, with ssim_weight > 0 also
        val_g_ssim_loss, with edge_weight > 0 also val_g_edge_loss, with fg_weight > 0 also val_g_fg_loss and with
        fg_ssim_weight > 0 also val_g_fg_ssim_loss, which val_g_loss then includes; with
        ema_decay > 0 also val_ema_g_recon_loss, the L1 of generator_ema(t1w) against t2w."""
        t1w_images, t2w_images = batch["t1w"], batch["t2w"]
        with torch.no_grad(), eval_modes(self.generator, self.discriminator):
            generated_imgs = self(t1w_images)
            d_fake = self._judge(generated_imgs, t1w_images)
            g_adv_loss = self.adversarial_loss(d_fake, self._labels(d_fake, 1.0))
            g_recon_loss = self.reconstruction_loss(generated_imgs, t2w_images)
            g_loss = scalar_axpby(g_adv_loss, 1.0, g_recon_loss, 1.0)
            terms = {}
            g_loss = self._add_generator_terms(g_loss, generated_imgs, t2w_images, terms)
            d_real = self._judge(t2w_images, t1w_images)
            real_loss = self.adversarial_loss(d_real, self._labels(d_real, self.hparams.one_sided_label_value))
            fake_loss = self.adversarial_loss(d_fake, self._labels(d_fake, 0.0))
            d_loss = scalar_axpby(real_loss, 0.5, fake_loss, 0.5)
            if self.generator_ema is not None:
                ema_recon_loss = self.reconstruction_loss(self.generator_ema(t1w_images), t2w_images)
        out = {"val_g_adv_loss": g_adv_loss, "val_g_recon_loss": g_recon_loss, "val_g_loss": g_loss, "val_d_loss": d_loss}
        out.update(("val_" + name, value) for name, value in terms.items())
        if self.generator_ema is not None:
            out["val_ema_g_recon_loss"] = ema_recon_loss
        for name, value in out.items():
            self.log(name, value)
        return out

    def configure_optimizers(self):                 # GAN_final.py:298-308
        h = self.hparams
        norm_opts = dict(max_grad_norm=h.grad_clip if h.grad_clip > 0 else None, measure_grad_norm=h.log_grad_norm)
        opt_g = FusedAdam(self.generator, lr=h.g_lr, betas=(h.b1, h.b2), ema=self.generator_ema,
                          ema_decay=h.ema_decay, ema_warmup=h.ema_warmup, **norm_opts)
        opt_d = FusedAdam(self.discriminator, lr=h.d_lr, betas=(h.b1, h.b2), **norm_opts)
        return [opt_g, opt_d], []

    def fit_batch(self, batch, batch_idx, optimizers) -> Dict[str, torch.Tensor]:
        # (Measured and dropped: pulling the D step's real branch forward onto a background stream
        #  underneath the generator's backward gains 0.7 ms of 60 -- matrix-bound kernels and chains
        #  of small launches contend for the same CUs -- and stretches D's forward kernels by 20 %.)
        nets: List[_EngineModule] = [self.generator, self.discriminator]
        if self.pair_augment is not None:           # once per batch: training_step and validation_step never augment
            self.pair_augment.generator = self.aug_generator
            with torch.no_grad():
                batch = self.pair_augment(batch)
        for idx, opt in enumerate(optimizers):
            other = nets[1 - idx]
            for p in other.parameters():            # toggle_optimizer
                p.requires_grad_(False)
            opt.zero_grad()
            loss = self.training_step(batch, batch_idx, idx)
            loss.backward()
            if self.ddp is not None:
                self.ddp.reduce_gradients(nets[idx], opt)
            opt.step()
            if getattr(opt, "grad_norm", None) is not None:     # clipping or measuring is on: a snapshot of the scalar
                self.log(("g_grad_norm", "d_grad_norm")[idx], opt.grad_norm.clone())
            for p in other.parameters():
                p.requires_grad_(True)
        return dict(self.logged)


_UNSUPPORTED_GLOBAL = re.compile(r"GLOBAL ([\w\.]+) was not an allowed global")


def _inert_stub(full_path: str):
    """A placeholder class carrying the module / name of a global the checkpoint's pickle refers to
    (e.g. `pytorch_lightning.callbacks.model_checkpoint.ModelCheckpoint`, which Lightning 1.2.1 uses as
    a KEY of checkpoint['callbacks']).  Nothing is imported and nothing from the file runs: the
    weights-only unpickler resolves the name to this class, whose construction ignores its arguments.
    Dict-like names come back as plain dicts so that their items can still be read."""
    module, _, name = full_path.rpartition(".")
    ns = {"__module__": module, "__init__": lambda self, *a, **k: None, "__setstate__": lambda self, state: None}
    if name.endswith("Dict") or name.endswith("dict"):
        ns["__new__"] = staticmethod(lambda cls, *a, **k: {})
    return type(name, (object,), ns)


def load_checkpoint_blob(path: str):
    """`torch.load(path, weights_only=True)` that also accepts the reference's real checkpoint format:
    Lightning writes class objects and small helper types into the pickle next to the tensors, which the
    weights-only unpickler refuses by name.  Each refused name is mapped to an inert stub (above) through
    `torch.serialization.safe_globals` and the load is retried; the stubs never leave this function's scope."""
    stubs = []
    for _ in range(64):
        try:
            with torch.serialization.safe_globals(stubs):
                return torch.load(path, map_location="cpu", weights_only=True)
        except Exception as e:          # pickle.UnpicklingError from the weights-only unpickler
            m = _UNSUPPORTED_GLOBAL.search(str(e))
            if m is None or any(f"{c.__module__}.{c.__name__}" == m.group(1) for c in stubs):
                raise
            stubs.append(_inert_stub(m.group(1)))
    raise RuntimeError(f"{path}: more than 64 distinct non-tensor globals in the pickle")


def load_reference_checkpoint(model: nn.Module, path: str, strict: bool = False, optimizers=None):
    """Load a Lightning checkpoint written by the reference's trainer (code/GAN/inferrence.py:97-106:
    `torch.load(ckpt)['state_dict']`, `load_state_dict(..., strict=False)`) into `model` (a GAN, or a
    bare generator / discriminator: then the `generator.` / `discriminator.` prefix is stripped).
    The file is read with `weights_only=True`: nothing in it is executed (see load_checkpoint_blob for
    how the trainer's non-tensor entries -- `callbacks` keyed by the ModelCheckpoint class,
    `hyper_parameters`, `optimizer_states` -- are tolerated).  `optimizers` (the list
    `configure_optimizers` returned) additionally restores Adam's moments from `optimizer_states`."""
    blob = load_checkpoint_blob(path)
    sd = blob["state_dict"] if isinstance(blob, dict) and "state_dict" in blob else blob
    if not isinstance(model, GAN):
        want = set(model.state_dict().keys())
        for prefix in ("generator.", "discriminator."):
            sub = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
            if sub and set(sub) & want:
                sd = sub
                break
    res = model.load_state_dict(sd, strict=strict)
    if (isinstance(model, GAN) and model.generator_ema is not None
            and not any(k.startswith("generator_ema.") for k in sd)):
        model.reset_ema()                           # a checkpoint without an average: start it from the loaded weights
    if optimizers is not None and isinstance(blob, dict) and blob.get("optimizer_states"):
        states = blob["optimizer_states"]
        if len(states) != len(optimizers):
            raise ValueError(f"{path}: {len(states)} optimizer_states for {len(optimizers)} optimizers "
                             "(configure_optimizers order: generator, discriminator)")
        for opt, st in zip(optimizers, states):
            opt.load_state_dict(st)
    return res
