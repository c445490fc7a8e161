"""Thin Python wrappers over the C ABI: shape/pitch checks on the host, raw
device pointers and the current torch stream into the HIP library.

Activations are channels-last tensors of shape (N, D, H, W, C) whose last
dimension may be a slice of a wider buffer (pitch = stride of W).  Nothing in
here computes: every function ends in exactly one C call.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from ._lib import ConvGeomC, NormFoldC, PeerTapsBF16C, PeerTapsC, PrologueC, check, lib

ACT_NONE = 0
ACT_LEAKY = 1


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _clx(t: torch.Tensor, dtype, what: str) -> Tuple[int, int, int]:
    """Validate a channels-last (N,D,H,W,C) view of the given dtype; return (n, pixels/sample, ld)."""
    if t.dim() != 5 or t.dtype != dtype or not t.is_cuda:
        raise ValueError(f"{what}: need a CUDA {dtype} (N,D,H,W,C) tensor, got {tuple(t.shape)} {t.dtype} {t.device}")
    n, d, h, w, c = t.shape
    st = t.stride()
    # pitch from the innermost dimension that actually has extent (size-1 dims carry arbitrary strides)
    ld = st[3] if w > 1 else (st[2] if h > 1 else (st[1] if d > 1 else (st[0] if n > 1 else c)))
    want = (d * h * w * ld, h * w * ld, w * ld, ld, 1)
    if not (ld >= c and all(sz == 1 or a == b for sz, a, b in zip(t.shape, st, want))):
        raise ValueError(f"{what}: not a pixel-contiguous channels-last view: shape {tuple(t.shape)} strides {st}")
    return n, d * h * w, ld


def _cl(t: torch.Tensor, what: str) -> Tuple[int, int, int]:
    return _clx(t, torch.float32, what)


@dataclass(frozen=True)
class ConvGeom:
    """Geometry of one nn.ConvNd / nn.ConvTransposeNd (depth dim unused in 2-D)."""
    n: int
    in_dhw: Tuple[int, int, int]
    cin: int
    cout: int
    k: Tuple[int, int, int]
    stride: Tuple[int, int, int]
    pad: Tuple[int, int, int]
    transposed: bool = False
    out_pad: Tuple[int, int, int] = (0, 0, 0)
    mm_bf16: bool = False      # MPGAN_CONV_MM_BF16: matrix operands rounded to bf16, fp32 storage and accumulation
    min_blocks: int = 0        # launch size from which the big-tile forms serve this conv (0: the library's 1024)

    @property
    def out_dhw(self) -> Tuple[int, int, int]:
        if not self.transposed:
            return tuple((i + 2 * p - k) // s + 1 for i, p, k, s in zip(self.in_dhw, self.pad, self.k, self.stride))
        return tuple((i - 1) * s - 2 * p + k + op
                     for i, p, k, s, op in zip(self.in_dhw, self.pad, self.k, self.stride, self.out_pad))

    @property
    def taps(self) -> int:
        return self.k[0] * self.k[1] * self.k[2]

    def c(self) -> ConvGeomC:
        g = ConvGeomC()
        g.n = self.n
        g.in_dhw[:] = self.in_dhw
        g.out_dhw[:] = self.out_dhw
        g.cin, g.cout = self.cin, self.cout
        g.k[:] = self.k
        g.stride[:] = self.stride
        g.pad[:] = self.pad
        g.transposed = 1 if self.transposed else 0
        g.flags = 1 if self.mm_bf16 else 0
        g.min_blocks = int(self.min_blocks)
        return g

    def with_n(self, n: int) -> "ConvGeom":
        return dataclasses.replace(self, n=n)


@dataclass
class Prologue:
    """a = act(z*scale + shift) applied on load (norm + PReLU/LeakyReLU of the producer)."""
    scale: torch.Tensor
    shift: torch.Tensor
    n_stride: int = 0
    act: int = ACT_NONE
    slope: float = 1.0
    slope_t: Optional[torch.Tensor] = None  # device scalar (PReLU alpha)

    def c(self) -> PrologueC:
        p = PrologueC()
        p.scale = self.scale.data_ptr()
        p.shift = self.shift.data_ptr()
        p.n_stride = self.n_stride
        p.act = self.act
        p.slope = self.slope
        p.slope_ptr = None if self.slope_t is None else self.slope_t.data_ptr()
        return p


def _pro(p: Optional[Prologue]):
    return None if p is None else C.byref(p.c())


@dataclass
class PeerTaps:
    """The other pass of a perceptual-loss pair (see mpgan_peer_taps)."""
    z: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    coef: torch.Tensor  # device float[3]

    def c(self) -> PeerTapsC:
        t = PeerTapsC()
        t.z_peer = self.z.data_ptr()
        t.ld_peer = _cl(self.z, "peer z")[2]
        t.scale_peer = self.scale.data_ptr()
        t.shift_peer = self.shift.data_ptr()
        t.coef = self.coef.data_ptr()
        return t


def _peer(t: Optional[PeerTaps]):
    return None if t is None else C.byref(t.c())


ACC_WORDS = 4
ACC_REPLICAS = 8


def conv_acc_supported(g: ConvGeom, has_prologue) -> bool:
    gc = g.c()
    return bool(lib().mpgan_conv_acc_supported(C.byref(gc), int(has_prologue)))


def conv_fold_supported(g: ConvGeom) -> bool:
    gc = g.c()
    return bool(lib().mpgan_conv_fold_supported(C.byref(gc)))


def make_fold(acc, replicas, cstride, count, norm_mod, scale, shift, mean, invstd) -> NormFoldC:
    """mpgan_norm_fold for a torch BatchNorm module's parameters / buffers and a plan's output vectors."""
    f = NormFoldC()
    f.acc = acc.data_ptr()
    f.replicas, f.cstride, f.count = int(replicas), int(cstride), int(count)
    f.gamma, f.beta = _ptr(norm_mod.weight), _ptr(norm_mod.bias)
    f.eps, f.momentum = float(norm_mod.eps), float(norm_mod.momentum if norm_mod.momentum is not None else 0.1)
    f.running_mean = _ptr(getattr(norm_mod, "running_mean", None))
    f.running_var = _ptr(getattr(norm_mod, "running_var", None))
    f.num_batches_tracked = _ptr(getattr(norm_mod, "num_batches_tracked", None))
    f.scale, f.shift, f.mean, f.invstd = scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr()
    return f


def _check_in_out(g: ConvGeom, x: torch.Tensor, y: torch.Tensor, what: str):
    if tuple(x.shape) != (g.n, *g.in_dhw, g.cin):
        raise ValueError(f"{what}: input shape {tuple(x.shape)} != {(g.n, *g.in_dhw, g.cin)}")
    if tuple(y.shape) != (g.n, *g.out_dhw, g.cout):
        raise ValueError(f"{what}: output shape {tuple(y.shape)} != {(g.n, *g.out_dhw, g.cout)}")


def conv_stats_rows(g: ConvGeom, has_prologue) -> int:
    """Partial rows the conv's fused statistics leave (0: none).  has_prologue: False/True, or the C
    code 0 none / 1 per-channel / 2 per-(sample, channel) / 3 per-channel fast LeakyReLU."""
    gc = g.c()
    return int(lib().mpgan_conv_stats_rows(C.byref(gc), int(has_prologue)))


def conv_variant(g: ConvGeom, backward_data: bool, has_prologue) -> int:
    gc = g.c()
    return int(lib().mpgan_conv_variant(C.byref(gc), int(backward_data), int(has_prologue)))


def conv_forward(g: ConvGeom, x, w_packed, bias, y, *, pro: Optional[Prologue] = None, resid=None,
                 tanh_out: bool = False, stats_partials=None):
    _check_in_out(g, x, y, "conv_forward")
    _, _, ldx = _cl(x, "conv_forward x")
    _, _, ldy = _cl(y, "conv_forward y")
    ldr = 0
    if resid is not None:
        if resid.shape != y.shape:
            raise ValueError("conv_forward: resid shape mismatch")
        _, _, ldr = _cl(resid, "conv_forward resid")
    if w_packed.numel() < g.cout * g.cin * g.taps:
        raise ValueError("conv_forward: packed weight too small")
    gc = g.c()
    if stats_partials is not None and stats_partials.numel() < conv_stats_rows(
            g, 0 if pro is None else (2 if pro.n_stride else 1)) * 2 * g.cout:
        raise ValueError("conv_forward: stats_partials too small")
    check(lib().mpgan_conv_forward(C.byref(gc), x.data_ptr(), ldx, w_packed.data_ptr(), _ptr(bias), _pro(pro),
                                   _ptr(resid), ldr, int(tanh_out), _ptr(stats_partials), y.data_ptr(), ldy,
                                   _stream()), "conv_forward")
    return y


def conv_forward_act(g: ConvGeom, x, w_packed, scale, shift, slope, y, *, resid=None, tanh_out: bool = False):
    """Eval-mode inference conv (code/GAN/inferrence.py:97-110): y = prelu(conv(x) * scale + shift, slope) (+ resid) (tanh),
    everything behind the matrix product applied in the conv's epilogue (include/mpgan_hip.h: mpgan_conv_forward_act)."""
    _check_in_out(g, x, y, "conv_forward_act")
    _, _, ldx = _cl(x, "conv_forward_act x")
    _, _, ldy = _cl(y, "conv_forward_act y")
    ldr = 0
    if resid is not None:
        if resid.shape != y.shape:
            raise ValueError("conv_forward_act: resid shape mismatch")
        _, _, ldr = _cl(resid, "conv_forward_act resid")
    if w_packed.numel() < g.cout * g.cin * g.taps:
        raise ValueError("conv_forward_act: packed weight too small")
    for v in (scale, shift, slope):
        if v.numel() < g.cout or v.dtype != torch.float32 or not v.is_contiguous():
            raise ValueError("conv_forward_act: scale / shift / slope must be contiguous fp32 vectors of cout elements")
    gc = g.c()
    check(lib().mpgan_conv_forward_act(C.byref(gc), x.data_ptr(), ldx, w_packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                       slope.data_ptr(), _ptr(resid), ldr, int(tanh_out), y.data_ptr(), ldy, _stream()),
          "conv_forward_act")
    return y


def conv_backward_data(g: ConvGeom, dy, w_packed_bwd, dx, *, resid=None):
    _check_in_out(g, dx, dy, "conv_backward_data")
    _, _, lddy = _cl(dy, "conv_backward_data dy")
    _, _, lddx = _cl(dx, "conv_backward_data dx")
    ldr = 0
    if resid is not None:
        if resid.shape != dx.shape:
            raise ValueError("conv_backward_data: resid shape mismatch")
        _, _, ldr = _cl(resid, "conv_backward_data resid")
    gc = g.c()
    check(lib().mpgan_conv_backward_data(C.byref(gc), dy.data_ptr(), lddy, w_packed_bwd.data_ptr(), _ptr(resid), ldr,
                                         dx.data_ptr(), lddx, _stream()), "conv_backward_data")
    return dx


def conv_bwd_stats_rows(g: ConvGeom) -> int:
    """Partial rows conv_backward_data_stats leaves for this geometry (0: no fused sums for it)."""
    gc = g.c()
    return int(lib().mpgan_conv_bwd_stats_rows(C.byref(gc)))


def conv_backward_data_stats(g: ConvGeom, dy, w_packed_bwd, dx, z, scale, shift, mean, invstd, act: int, slope: float,
                             partials):
    """dx = conv_backward_data(dy) and, from the same launch, the norm-backward partial sums of dx against z
    (partials[rows][3][Cin]; see include/mpgan_hip.h)."""
    _check_in_out(g, dx, dy, "conv_backward_data_stats")
    _, _, lddy = _cl(dy, "conv_backward_data_stats dy")
    _, _, lddx = _cl(dx, "conv_backward_data_stats dx")
    _, _, ldz = _cl(z, "conv_backward_data_stats z")
    rows = conv_bwd_stats_rows(g)
    if z.shape != dx.shape or partials.numel() < rows * 3 * g.cin:
        raise ValueError("conv_backward_data_stats: z must match dx and partials hold rows*3*Cin floats")
    gc = g.c()
    check(lib().mpgan_conv_backward_data_stats(C.byref(gc), dy.data_ptr(), lddy, w_packed_bwd.data_ptr(), dx.data_ptr(),
                                               lddx, z.data_ptr(), ldz, scale.data_ptr(), shift.data_ptr(),
                                               mean.data_ptr(), invstd.data_ptr(), int(act), float(slope),
                                               partials.data_ptr(), _stream()), "conv_backward_data_stats")
    return rows


def conv_wgrad_workspace(g: ConvGeom) -> int:
    gc = g.c()
    return int(lib().mpgan_conv_wgrad_workspace(C.byref(gc)))


def conv_backward_weight(g: ConvGeom, x, dy, dw, workspace, *, pro: Optional[Prologue] = None, beta: float = 0.0,
                         dbias=None):
    _check_in_out(g, x, dy, "conv_backward_weight")
    _, _, ldx = _cl(x, "conv_backward_weight x")
    _, _, lddy = _cl(dy, "conv_backward_weight dy")
    if dw.numel() != g.cout * g.cin * g.taps or not dw.is_contiguous():
        raise ValueError("conv_backward_weight: dw must be the contiguous torch-layout weight gradient")
    gc = g.c()
    check(lib().mpgan_conv_backward_weight(C.byref(gc), x.data_ptr(), ldx, _pro(pro), dy.data_ptr(), lddy,
                                           dw.data_ptr(), _ptr(dbias), float(beta), workspace.data_ptr(),
                                           workspace.numel() * workspace.element_size(), _stream()),
          "conv_backward_weight")
    return dw


def pack_weights(flat_params, packed, table, n_entries: int, max_elems: int):
    check(lib().mpgan_pack_weights(flat_params.data_ptr(), packed.data_ptr(), table.data_ptr(), n_entries, max_elems,
                                   _stream()), "pack_weights")


def stats_chunks(pixels_per_sample: int, c: int) -> int:
    return int(lib().mpgan_stats_chunks(pixels_per_sample, c))


def channel_stats(z, partials):
    n, P, ld = _cl(z, "channel_stats")
    c = z.shape[-1]
    if partials.numel() < n * stats_chunks(P, c) * 2 * c:
        raise ValueError("channel_stats: partials too small")
    check(lib().mpgan_channel_stats(z.data_ptr(), ld, n, P, c, partials.data_ptr(), _stream()), "channel_stats")


def norm_finalize(partials, n, chunks, c, P, instance, gamma, beta, eps, momentum, running_mean, running_var, nbt,
                  scale, shift, mean, invstd):
    check(lib().mpgan_norm_finalize(partials.data_ptr(), n, chunks, c, P, int(instance), _ptr(gamma), _ptr(beta),
                                    float(eps), float(momentum), _ptr(running_mean), _ptr(running_var), _ptr(nbt),
                                    scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                    _stream()), "norm_finalize")


def norm_act_add(z, pz: Optional[Prologue], r, pr: Optional[Prologue], out, *, tanh_out=False):
    n, P, ldz = _cl(z, "norm_act_add z")
    _, _, ldo = _cl(out, "norm_act_add out")
    ldr = 0
    if r is not None:
        _, _, ldr = _cl(r, "norm_act_add r")
        if r.shape != z.shape:
            raise ValueError("norm_act_add: r shape mismatch")
    if out.shape != z.shape:
        raise ValueError("norm_act_add: out shape mismatch")
    check(lib().mpgan_norm_act_add(z.data_ptr(), ldz, _pro(pz), _ptr(r), ldr, _pro(pr), n, P, z.shape[-1],
                                   int(tanh_out), out.data_ptr(), ldo, _stream()), "norm_act_add")
    return out


def norm_bwd_reduce(g, z, p: Prologue, mean, invstd, partials, peer: Optional[PeerTaps] = None):
    n, P, ldz = _cl(z, "norm_bwd_reduce z")
    _, _, ldg = _cl(g, "norm_bwd_reduce g")
    if g.shape != z.shape:
        raise ValueError("norm_bwd_reduce: shape mismatch")
    c = z.shape[-1]
    if partials.numel() < n * stats_chunks(P, c) * (3 * c + 1):
        raise ValueError("norm_bwd_reduce: partials too small (need n*chunks*(3*c + 1) floats)")
    check(lib().mpgan_norm_bwd_reduce(g.data_ptr(), ldg, z.data_ptr(), ldz, _pro(p), mean.data_ptr(),
                                      invstd.data_ptr(), _peer(peer), n, P, c, partials.data_ptr(), _stream()),
          "norm_bwd_reduce")


def norm_bwd_finalize(partials, n, chunks, c, P, instance, dgamma, dbeta, dslope, c1, c2):
    check(lib().mpgan_norm_bwd_finalize(partials.data_ptr(), n, chunks, c, P, int(instance), _ptr(dgamma), _ptr(dbeta),
                                        _ptr(dslope), c1.data_ptr(), c2.data_ptr(), _stream()), "norm_bwd_finalize")


def norm_bwd_apply(g, z, p: Prologue, mean, invstd, c1, c2, dz, peer: Optional[PeerTaps] = None):
    n, P, ldz = _cl(z, "norm_bwd_apply z")
    _, _, ldg = _cl(g, "norm_bwd_apply g")
    _, _, lddz = _cl(dz, "norm_bwd_apply dz")
    if g.shape != z.shape or dz.shape != z.shape:
        raise ValueError("norm_bwd_apply: shape mismatch")
    check(lib().mpgan_norm_bwd_apply(g.data_ptr(), ldg, z.data_ptr(), ldz, _pro(p), mean.data_ptr(),
                                     invstd.data_ptr(), c1.data_ptr(), c2.data_ptr(), _peer(peer), n, P, z.shape[-1],
                                     dz.data_ptr(), lddz, _stream()), "norm_bwd_apply")
    return dz


def tap_l1_partials() -> int:
    return int(lib().mpgan_tap_l1_partials())


def tap_l1(za, pa: Prologue, zb, pb: Prologue, partials, out3):
    """out3 = mean |z_a-z_b|, |y_a-y_b|, |a_a-a_b| of one conv+BN+act layer of two passes."""
    n, P, lda = _cl(za, "tap_l1 a")
    _, _, ldb = _cl(zb, "tap_l1 b")
    if za.shape != zb.shape:
        raise ValueError("tap_l1: shape mismatch")
    check(lib().mpgan_tap_l1(za.data_ptr(), lda, _pro(pa), zb.data_ptr(), ldb, _pro(pb), n * P, za.shape[-1],
                             partials.data_ptr(), out3.data_ptr(), _stream()), "tap_l1")
    return out3


def conv_splitk_workspace(g: ConvGeom) -> int:
    gc = g.c()
    return int(lib().mpgan_conv_splitk_workspace(C.byref(gc)))


def conv_forward_splitk(g: ConvGeom, x, w_packed, bias, y, workspace, *, pro: Optional[Prologue] = None):
    _check_in_out(g, x, y, "conv_forward_splitk")
    _, _, ldx = _cl(x, "conv_forward_splitk x")
    _, _, ldy = _cl(y, "conv_forward_splitk y")
    gc = g.c()
    check(lib().mpgan_conv_forward_splitk(C.byref(gc), x.data_ptr(), ldx, w_packed.data_ptr(), _ptr(bias), _pro(pro),
                                          workspace.data_ptr(), workspace.numel() * 4, y.data_ptr(), ldy, _stream()),
          "conv_forward_splitk")
    return y


def sigmoid_forward(logit, prob):
    check(lib().mpgan_sigmoid_forward(logit.data_ptr(), logit.numel(), prob.data_ptr(), _stream()), "sigmoid_forward")
    return prob


def reduce_partials(partials, rows, row_stride, c, out, beta=0.0):
    check(lib().mpgan_reduce_partials(partials.data_ptr(), rows, row_stride, c, out.data_ptr(), float(beta),
                                      _stream()), "reduce_partials")


def add_tanh(a, b, y, apply_tanh: bool):
    check(lib().mpgan_add_tanh(a.data_ptr(), _ptr(b), a.numel(), int(apply_tanh), y.data_ptr(), _stream()),
          "add_tanh")
    return y


def tanh_backward(g, y, dx):
    check(lib().mpgan_tanh_backward(g.data_ptr(), y.data_ptr(), y.numel(), dx.data_ptr(), _stream()),
          "tanh_backward")
    return dx


def axpby(a, alpha, b, beta, y):
    check(lib().mpgan_axpby(a.data_ptr(), float(alpha), _ptr(b), float(beta), a.numel(), y.data_ptr(), _stream()),
          "axpby")
    return y


def copy_slice(src, dst, accumulate=False):
    n, P, lds = _cl(src, "copy_slice src")
    _, _, ldd = _cl(dst, "copy_slice dst")
    if src.shape != dst.shape:
        raise ValueError("copy_slice: shape mismatch")
    check(lib().mpgan_copy_slice(src.data_ptr(), lds, dst.data_ptr(), ldd, n * P, src.shape[-1], int(accumulate),
                                 _stream()), "copy_slice")
    return dst


def linear1_partials(n: int) -> int:
    return int(lib().mpgan_linear1_partials(n))


def linear1_forward(z, p: Optional[Prologue], w_perm, bias, partials, logit, prob=None):
    n, P, ld = _cl(z, "linear1_forward z")
    c = z.shape[-1]
    if ld != c:
        raise ValueError("linear1_forward: z must be dense")
    check(lib().mpgan_linear1_forward(z.data_ptr(), _pro(p), n, P, c, w_perm.data_ptr(), _ptr(bias),
                                      partials.data_ptr(), logit.data_ptr(), _ptr(prob), _stream()),
          "linear1_forward")
    return logit


def linear1_backward(z, p: Optional[Prologue], w_perm, dlogit, g_a, dw, dbias, beta=0.0):
    n, P, ld = _cl(z, "linear1_backward z")
    c = z.shape[-1]
    if ld != c or (g_a is not None and (g_a.shape != z.shape or not g_a.is_contiguous())):
        raise ValueError("linear1_backward: z / g_a must be dense and same shape")
    check(lib().mpgan_linear1_backward(z.data_ptr(), _pro(p), n, P, c, w_perm.data_ptr(), dlogit.data_ptr(),
                                       _ptr(g_a), _ptr(dw), _ptr(dbias), float(beta), _stream()), "linear1_backward")


def sigmoid_bce(logit, target: float, loss_scale: float, prob, loss, dlogit):
    check(lib().mpgan_sigmoid_bce(logit.data_ptr(), logit.numel(), float(target), float(loss_scale), _ptr(prob),
                                  _ptr(loss), _ptr(dlogit), _stream()), "sigmoid_bce")


def bce_forward(prob, target, loss):
    check(lib().mpgan_bce_forward(prob.data_ptr(), target.data_ptr(), prob.numel(), loss.data_ptr(), _stream()),
          "bce_forward")


def bce_backward(prob, target, gout, dprob):
    check(lib().mpgan_bce_backward(prob.data_ptr(), target.data_ptr(), prob.numel(), gout.data_ptr(),
                                   dprob.data_ptr(), _stream()), "bce_backward")


def _i3(v: Sequence[int]):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def maphead_workspace(n: int, in_dhw: Sequence[int], c: int, k_dhw: Sequence[int]) -> int:
    """Bytes of scratch maphead_backward needs for dw."""
    need = int(lib().mpgan_maphead_workspace(n, _i3(in_dhw), c, _i3(k_dhw)))
    if need < 0:
        check(-2, "maphead_workspace")
    return need


def maphead_forward(z, p: Optional[Prologue], k_dhw: Sequence[int], w_perm, bias, logit, prob=None):
    """The Markovian head's valid conv C -> 1 on the channels-last (N,D,H,W,C) z read through `p`: logit and
    prob = sigmoid(logit), both (N, D-kd+1, H-kh+1, W-kw+1)."""
    n, P, ld = _cl(z, "maphead_forward z")
    c = z.shape[-1]
    if ld != c:
        raise ValueError("maphead_forward: z must be dense")
    check(lib().mpgan_maphead_forward(z.data_ptr(), _pro(p), n, _i3(z.shape[1:4]), c, _i3(k_dhw), w_perm.data_ptr(),
                                      _ptr(bias), logit.data_ptr(), _ptr(prob), _stream()), "maphead_forward")
    return logit


def maphead_backward(z, p: Optional[Prologue], k_dhw: Sequence[int], w_perm, dlogit, g_a, dw, dbias, beta=0.0,
                     workspace=None):
    """g_a (w.r.t. the activated tensor), dw (torch order, beta-accumulated) and dbias of maphead_forward; each may be
    None.  workspace: a tensor of at least maphead_workspace(...) bytes (dw only)."""
    n, P, ld = _cl(z, "maphead_backward z")
    c = z.shape[-1]
    if ld != c or (g_a is not None and (g_a.shape != z.shape or not g_a.is_contiguous())):
        raise ValueError("maphead_backward: z / g_a must be dense and same shape")
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    check(lib().mpgan_maphead_backward(z.data_ptr(), _pro(p), n, _i3(z.shape[1:4]), c, _i3(k_dhw), w_perm.data_ptr(),
                                       dlogit.data_ptr(), _ptr(g_a), _ptr(dw), _ptr(dbias), float(beta),
                                       _ptr(workspace), ws_bytes, _stream()), "maphead_backward")


def sigmoid_backward(dprob, prob, dlogit):
    check(lib().mpgan_sigmoid_backward(dprob.data_ptr(), prob.data_ptr(), prob.numel(), dlogit.data_ptr(), _stream()),
          "sigmoid_backward")


def scale_by_device_scalar(x, scalar, y):
    check(lib().mpgan_scale_by_device_scalar(x.data_ptr(), scalar.data_ptr(), x.numel(), y.data_ptr(), _stream()),
          "scale_by_device_scalar")
    return y


def weighted_sum(v, w, out):
    """out[0] = sum_i v[i] * w[i] (device vectors of equal length, index order)."""
    if v.numel() != w.numel() or not v.is_contiguous() or not w.is_contiguous():
        raise ValueError("weighted_sum: v and w must be contiguous and of equal length")
    check(lib().mpgan_weighted_sum(v.data_ptr(), w.data_ptr(), v.numel(), out.data_ptr(), _stream()), "weighted_sum")
    return out


def l1_partials() -> int:
    return int(lib().mpgan_l1_partials())


def l1_loss(a, b, partials, loss, grad_a=None, grad_scale: float = 1.0):
    if a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("l1_loss: a and b must be contiguous and same shape")
    check(lib().mpgan_l1_loss(a.data_ptr(), b.data_ptr(), a.numel(), float(grad_scale), partials.data_ptr(),
                              loss.data_ptr(), _ptr(grad_a), _stream()), "l1_loss")


ADV_KINDS = {"bce_logits": 0, "lsgan": 1}      # MPGAN_ADV_BCE_LOGITS, MPGAN_ADV_LSGAN


def adv_loss_partials(n: int) -> int:
    """Doubles of scratch adv_loss needs for n logits."""
    need = int(lib().mpgan_adv_loss_partials(int(n)))
    if need < 0:
        check(-1, "adv_loss_partials")
    return need


def adv_loss(logit, target, kind: str, partials, loss, grad=None):
    """loss = the mean objective `kind` ("bce_logits" | "lsgan") of fp32 logits against targets of the same shape;
    grad (optional) = dL/dlogit for an upstream gradient of 1.  partials: float64, >= adv_loss_partials(n)."""
    if kind not in ADV_KINDS:
        raise ValueError(f"adv_loss: kind must be one of {sorted(ADV_KINDS)}, got {kind!r}")
    if logit.shape != target.shape or not logit.is_contiguous() or not target.is_contiguous():
        raise ValueError("adv_loss: logit and target must be contiguous and same shape")
    if logit.dtype != torch.float32 or target.dtype != torch.float32 or partials.dtype != torch.float64:
        raise ValueError("adv_loss: logit / target must be float32 and partials float64")
    if grad is not None and (grad.shape != logit.shape or not grad.is_contiguous() or grad.dtype != torch.float32):
        raise ValueError("adv_loss: grad must be a contiguous float32 tensor of logit's shape")
    if not all(t.is_cuda for t in (logit, target, partials, loss) + ((grad,) if grad is not None else ())):
        raise ValueError("adv_loss: every tensor must be on the GPU (there is no CPU path)")
    n = logit.numel()
    if n >= 2 ** 31:
        raise ValueError(f"adv_loss: {n} elements exceed the 32-bit count of mpgan_adv_loss")
    if n > 0 and partials.numel() < adv_loss_partials(n):
        raise ValueError(f"adv_loss: partials holds {partials.numel()} doubles, needs {adv_loss_partials(n)}")
    check(lib().mpgan_adv_loss(logit.data_ptr(), target.data_ptr(), n, ADV_KINDS[kind], partials.data_ptr(),
                               loss.data_ptr(), _ptr(grad), _stream()), "adv_loss")
    return loss


def adam_step(p, g, m, v, lr, b1, b2, eps, step: int, grad_scale: float = 1.0):
    if not (p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()):
        raise ValueError("adam_step: flat buffers must be contiguous")
    if not (p.numel() == g.numel() == m.numel() == v.numel()):
        raise ValueError("adam_step: size mismatch")
    check(lib().mpgan_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr),
                                float(b1), float(b2), float(eps), int(step), float(grad_scale), _stream()),
          "adam_step")


def _flat_f32(t, what: str, name: str):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous float32 tensor on the GPU (there is no CPU path), "
                         f"got {t.dtype} on {t.device}")


def grad_norm_workspace(numel: int) -> int:
    """Bytes of scratch grad_norm needs for numel elements."""
    need = int(lib().mpgan_grad_norm_workspace(int(numel)))
    if need < 0:
        check(-1, "grad_norm_workspace")
    return need


def grad_norm(g, out2, workspace, grad_scale: float = 1.0, max_norm: float = 0.0):
    """out2[0] = ||g * grad_scale||_2 (fp64 sums), out2[1] = clip_grad_norm_'s coefficient for max_norm (1 when
    max_norm <= 0); both stay on the device.  workspace: >= grad_norm_workspace(g.numel()) bytes."""
    _flat_f32(g, "grad_norm", "g")
    _flat_f32(out2, "grad_norm", "out2")
    if out2.numel() < 2:
        raise ValueError(f"grad_norm: out2 holds {out2.numel()} floats, needs 2")
    if not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("grad_norm: workspace must be a contiguous tensor on the GPU")
    ws_bytes = workspace.numel() * workspace.element_size()
    if g.numel() > 0 and ws_bytes < grad_norm_workspace(g.numel()):
        raise ValueError(f"grad_norm: workspace holds {ws_bytes} bytes, needs {grad_norm_workspace(g.numel())}")
    check(lib().mpgan_grad_norm(g.data_ptr(), g.numel(), float(grad_scale), float(max_norm), workspace.data_ptr(),
                                ws_bytes, out2.data_ptr(), _stream()), "grad_norm")
    return out2


def adam_step_ex(p, g, m, v, lr, b1, b2, eps, step: int, grad_scale: float = 1.0, coef=None, ema=None,
                 ema_weight: float = 0.0):
    """adam_step with the gradient also multiplied by the device scalar `coef` (grad_norm's out2[1:2]) and, with `ema`,
    ema = lerp(ema, p_new, ema_weight) written in the same pass."""
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)) + ((("ema", ema),) if ema is not None else ()):
        _flat_f32(t, "adam_step_ex", name)
        if t.numel() != p.numel():
            raise ValueError(f"adam_step_ex: size mismatch ({name} has {t.numel()} elements, p {p.numel()})")
    if coef is not None:
        _flat_f32(coef, "adam_step_ex", "coef")
        if coef.numel() != 1:
            raise ValueError(f"adam_step_ex: coef must hold one float, got {coef.numel()}")
    check(lib().mpgan_adam_step_ex(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr),
                                   float(b1), float(b2), float(eps), int(step), float(grad_scale), _ptr(coef),
                                   _ptr(ema), float(ema_weight), _stream()), "adam_step_ex")


def ema_buffers(table, n_entries: int, max_elems: int, ema_weight: float):
    """One launch over `table` (int64 [n][4] on the device: src_ptr, dst_ptr, numel, kind): fp32 rows (kind 0) are
    dst = lerp(dst, src, ema_weight), int64 rows (kind 1) are copied."""
    if n_entries > 0:
        if table.dtype != torch.int64 or not table.is_cuda or not table.is_contiguous():
            raise ValueError("ema_buffers: table must be a contiguous int64 tensor on the GPU")
        if table.numel() < 4 * n_entries:
            raise ValueError(f"ema_buffers: table holds {table.numel()} values, needs {4 * n_entries}")
    check(lib().mpgan_ema_buffers(_ptr(table) if n_entries > 0 else None, int(n_entries), int(max_elems),
                                  float(ema_weight), _stream()), "ema_buffers")


def _i3(v: Sequence[int]):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def patch_gather(vol, corners, samples: int, roi, patches):
    """vol (B,1,D,H,W) or (B,D,H,W,1); corners int32 (B*S,3)."""
    b = vol.shape[0]
    dhw = vol.shape[2:] if vol.shape[1] == 1 and vol.dim() == 5 and vol.shape[-1] != 1 else vol.shape[1:4]
    if corners.dtype != torch.int32 or corners.numel() != b * samples * 3:
        raise ValueError("patch_gather: corners must be int32 (B*S,3)")
    check(lib().mpgan_patch_gather(vol.data_ptr(), b, _i3(dhw), corners.data_ptr(), samples, _i3(roi),
                                   patches.data_ptr(), _stream()), "patch_gather")
    return patches


def patch_scatter_add(dpatches, corners, samples: int, roi, dvol):
    b = dvol.shape[0]
    dhw = dvol.shape[2:] if dvol.shape[1] == 1 and dvol.dim() == 5 and dvol.shape[-1] != 1 else dvol.shape[1:4]
    check(lib().mpgan_patch_scatter_add(dpatches.data_ptr(), b, _i3(dhw), corners.data_ptr(), samples, _i3(roi),
                                        dvol.data_ptr(), _stream()), "patch_scatter_add")
    return dvol


def pack_weight(w: torch.Tensor, *, transposed: bool = False, for_dgrad: bool = False) -> torch.Tensor:
    """Pack ONE torch-layout conv / convT / linear weight (convenience for tests
    and small callers; networks pack all their weights with one table launch)."""
    w = w.contiguous()
    if transposed:
        cin, cout = w.shape[0], w.shape[1]
    else:
        cout, cin = w.shape[0], w.shape[1]
    taps = w.numel() // (cin * cout)
    table = torch.tensor([[0, 0, cout, cin, taps, int(transposed), int(for_dgrad), 0]], dtype=torch.int64,
                         device=w.device)
    packed = torch.empty(w.numel(), dtype=torch.float32, device=w.device)
    pack_weights(w, packed, table, 1, w.numel())
    return packed


# --------------------------------------------------------------------------
# bf16 storage path (BASELINE config C5): activations / packed weights bf16, fp32 accumulate + statistics
# --------------------------------------------------------------------------
BF16 = torch.bfloat16


def _check_shapes(g: ConvGeom, x, y, what):
    if tuple(x.shape) != (g.n, *g.in_dhw, g.cin) or tuple(y.shape) != (g.n, *g.out_dhw, g.cout):
        raise ValueError(f"{what}: shapes {tuple(x.shape)} / {tuple(y.shape)} do not match the geometry")


def conv_stats_rows_bf16(g: ConvGeom) -> int:
    gc = g.c()
    return int(lib().mpgan_conv_stats_rows_bf16(C.byref(gc)))


def conv_forward_bf16(g: ConvGeom, x, w_packed, bias, y, *, stats_partials=None):
    _check_shapes(g, x, y, "conv_forward_bf16")
    _, _, ldx = _clx(x, BF16, "conv_forward_bf16 x")
    _, _, ldy = _clx(y, BF16, "conv_forward_bf16 y")
    if w_packed.dtype != BF16 or w_packed.numel() < g.cout * g.cin * g.taps:
        raise ValueError("conv_forward_bf16: packed weight must be bf16 and complete")
    if stats_partials is not None and stats_partials.numel() < conv_stats_rows_bf16(g) * 2 * g.cout:
        raise ValueError("conv_forward_bf16: stats_partials too small")
    gc = g.c()
    check(lib().mpgan_conv_forward_bf16(C.byref(gc), x.data_ptr(), ldx, w_packed.data_ptr(), _ptr(bias),
                                        _ptr(stats_partials), y.data_ptr(), ldy, _stream()), "conv_forward_bf16")
    return y


def conv_backward_data_bf16(g: ConvGeom, dy, w_packed_bwd, dx):
    _check_shapes(g, dx, dy, "conv_backward_data_bf16")
    _, _, lddy = _clx(dy, BF16, "conv_backward_data_bf16 dy")
    _, _, lddx = _clx(dx, BF16, "conv_backward_data_bf16 dx")
    if w_packed_bwd.dtype != BF16:
        raise ValueError("conv_backward_data_bf16: packed weight must be bf16")
    gc = g.c()
    check(lib().mpgan_conv_backward_data_bf16(C.byref(gc), dy.data_ptr(), lddy, w_packed_bwd.data_ptr(), dx.data_ptr(),
                                              lddx, _stream()), "conv_backward_data_bf16")
    return dx


def conv_wgrad_workspace_bf16(g: ConvGeom) -> int:
    gc = g.c()
    return int(lib().mpgan_conv_wgrad_workspace_bf16(C.byref(gc)))


def conv_backward_weight_bf16(g: ConvGeom, x, dy, dw, workspace, *, beta: float = 0.0):
    _check_shapes(g, x, dy, "conv_backward_weight_bf16")
    _, _, ldx = _clx(x, BF16, "conv_backward_weight_bf16 x")
    _, _, lddy = _clx(dy, BF16, "conv_backward_weight_bf16 dy")
    if dw.dtype != torch.float32 or dw.numel() != g.cout * g.cin * g.taps or not dw.is_contiguous():
        raise ValueError("conv_backward_weight_bf16: dw must be the contiguous fp32 torch-layout weight gradient")
    gc = g.c()
    check(lib().mpgan_conv_backward_weight_bf16(C.byref(gc), x.data_ptr(), ldx, dy.data_ptr(), lddy, dw.data_ptr(),
                                                float(beta), workspace.data_ptr(),
                                                workspace.numel() * workspace.element_size(), _stream()),
          "conv_backward_weight_bf16")
    return dw


def conv_forward_f32_to_bf16(g: ConvGeom, x, w_packed, bias, y, *, stats_partials=None):
    _check_shapes(g, x, y, "conv_forward_f32_to_bf16")
    _, _, ldx = _cl(x, "conv_forward_f32_to_bf16 x")
    _, _, ldy = _clx(y, BF16, "conv_forward_f32_to_bf16 y")
    gc = g.c()
    check(lib().mpgan_conv_forward_f32_to_bf16(C.byref(gc), x.data_ptr(), ldx, w_packed.data_ptr(), _ptr(bias),
                                               _ptr(stats_partials), y.data_ptr(), ldy, _stream()),
          "conv_forward_f32_to_bf16")
    return y


def _check_epi(g: ConvGeom, scale, shift, slope, what):
    for v in (scale, shift, slope):
        if v.dtype != torch.float32 or not v.is_cuda or v.numel() < g.cout or not v.is_contiguous():
            raise ValueError(f"{what}: scale / shift / slope must be contiguous CUDA fp32 vectors of >= cout elements")


def conv_forward_act_bf16(g: ConvGeom, x, w_packed, scale, shift, slope, y):
    """Eval-mode bf16 forward: y = lrelu(acc * scale[c] + shift[c], slope[c]) from the fp32 accumulator, stored once --
    as bf16, or as fp32 when `y` is an fp32 tensor (the layer the Linear head reads)."""
    what = "conv_forward_act_bf16"
    _check_shapes(g, x, y, what)
    _, _, ldx = _clx(x, BF16, what + " x")
    if y.dtype not in (BF16, torch.float32):
        raise ValueError(f"{what}: y must be bf16 or fp32")
    _, _, ldy = _clx(y, y.dtype, what + " y")
    if w_packed.dtype != BF16 or w_packed.numel() < g.cout * g.cin * g.taps:
        raise ValueError(f"{what}: packed weight must be bf16 and complete")
    _check_epi(g, scale, shift, slope, what)
    gc = g.c()
    check(lib().mpgan_conv_forward_act_bf16(C.byref(gc), x.data_ptr(), ldx, w_packed.data_ptr(), scale.data_ptr(),
                                            shift.data_ptr(), slope.data_ptr(), None, y.data_ptr(), ldy,
                                            int(y.dtype == torch.float32), _stream()), what)
    return y


def conv_forward_act_f32_to_bf16(g: ConvGeom, x, w_packed, scale, shift, slope, y):
    """The 1-input-channel first layer in eval mode: fp32 image in, activated bf16 out."""
    what = "conv_forward_act_f32_to_bf16"
    _check_shapes(g, x, y, what)
    _, _, ldx = _cl(x, what + " x")
    _, _, ldy = _clx(y, BF16, what + " y")
    _check_epi(g, scale, shift, slope, what)
    gc = g.c()
    check(lib().mpgan_conv_forward_act_f32_to_bf16(C.byref(gc), x.data_ptr(), ldx, w_packed.data_ptr(), scale.data_ptr(),
                                                   shift.data_ptr(), slope.data_ptr(), None, y.data_ptr(), ldy,
                                                   _stream()), what)
    return y


def conv_backward_data_bf16_to_f32(g: ConvGeom, dy, w_packed_bwd, dx):
    _check_shapes(g, dx, dy, "conv_backward_data_bf16_to_f32")
    _, _, lddy = _clx(dy, BF16, "conv_backward_data_bf16_to_f32 dy")
    _, _, lddx = _cl(dx, "conv_backward_data_bf16_to_f32 dx")
    gc = g.c()
    check(lib().mpgan_conv_backward_data_bf16_to_f32(C.byref(gc), dy.data_ptr(), lddy, w_packed_bwd.data_ptr(),
                                                     dx.data_ptr(), lddx, _stream()), "conv_backward_data_bf16_to_f32")
    return dx


def conv_wgrad_workspace_bf16dy(g: ConvGeom) -> int:
    gc = g.c()
    return int(lib().mpgan_conv_wgrad_workspace_bf16dy(C.byref(gc)))


def conv_backward_weight_bf16dy(g: ConvGeom, x, dy, dw, workspace, *, beta: float = 0.0, dbias=None):
    _check_shapes(g, x, dy, "conv_backward_weight_bf16dy")
    _, _, ldx = _cl(x, "conv_backward_weight_bf16dy x")
    _, _, lddy = _clx(dy, BF16, "conv_backward_weight_bf16dy dy")
    gc = g.c()
    check(lib().mpgan_conv_backward_weight_bf16dy(C.byref(gc), x.data_ptr(), ldx, dy.data_ptr(), lddy, dw.data_ptr(),
                                                  _ptr(dbias), float(beta), workspace.data_ptr(),
                                                  workspace.numel() * workspace.element_size(), _stream()),
          "conv_backward_weight_bf16dy")
    return dw


def pack_weight_bf16(w: torch.Tensor, *, for_dgrad: bool = False) -> torch.Tensor:
    """One fp32 ConvNd weight -> bf16 [Cout][tap][Cin] (or [Cin][tap][Cout] for backward-data)."""
    w = w.contiguous()
    cout, cin = w.shape[0], w.shape[1]
    taps = w.numel() // (cin * cout)
    table = torch.tensor([[0, 0, cout, cin, taps, 0, int(for_dgrad), 0]], dtype=torch.int64, device=w.device)
    packed = torch.empty(w.numel(), dtype=BF16, device=w.device)
    check(lib().mpgan_pack_weights_bf16(w.data_ptr(), packed.data_ptr(), table.data_ptr(), 1, w.numel(), _stream()),
          "pack_weights_bf16")
    return packed


def norm_act_bf16(z, scale, shift, slope: float, out):
    n, P, ldz = _clx(z, BF16, "norm_act_bf16 z")
    if out.shape != z.shape or out.dtype not in (BF16, torch.float32):
        raise ValueError("norm_act_bf16: out must match z and be bf16 or fp32")
    _, _, ldo = _clx(out, out.dtype, "norm_act_bf16 out")
    check(lib().mpgan_norm_act_bf16(z.data_ptr(), ldz, scale.data_ptr(), shift.data_ptr(), float(slope), n * P,
                                    z.shape[-1], out.data_ptr(), ldo, int(out.dtype == torch.float32), _stream()),
          "norm_act_bf16")
    return out


def norm_bwd_rows_bf16(rows: int, c: int) -> int:
    return int(lib().mpgan_norm_bwd_rows_bf16(rows, c))


@dataclass
class PeerTapsBF16:
    """The other pass of a perceptual-loss pair in bf16 storage (see mpgan_peer_taps_bf16): its stored bf16 z."""
    z: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    coef: torch.Tensor  # device float[3]

    def c(self) -> PeerTapsBF16C:
        t = PeerTapsBF16C()
        t.z_peer = self.z.data_ptr()
        t.ld_peer = _clx(self.z, BF16, "peer z")[2]
        t.scale_peer = self.scale.data_ptr()
        t.shift_peer = self.shift.data_ptr()
        t.coef = self.coef.data_ptr()
        return t


def _peer_arg(peer: Optional[PeerTapsBF16], z, what):
    """The descriptor argument of a `_peer` entry (none for the plain one) and the entry's name."""
    if peer is None:
        return (), what
    if peer.z.shape != z.shape:
        raise ValueError(f"{what}_peer: peer z must match z")
    return (C.byref(peer.c()),), what + "_peer"


def norm_bwd_reduce_bf16(g, z, scale, shift, mean, invstd, slope: float, partials, peer: Optional[PeerTapsBF16] = None):
    pe, what = _peer_arg(peer, z, "norm_bwd_reduce_bf16")
    n, P, ldz = _clx(z, BF16, what + " z")
    _, _, ldg = _clx(g, g.dtype, what + " g")
    c = z.shape[-1]
    if partials.numel() < norm_bwd_rows_bf16(n * P, c) * 3 * c + c:
        raise ValueError(what + ": partials too small")
    check(getattr(lib(), "mpgan_" + what)(g.data_ptr(), int(g.dtype == torch.float32), ldg, z.data_ptr(), ldz,
                                          scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), *pe,
                                          float(slope), n * P, c, partials.data_ptr(), _stream()), what)


def norm_bwd_apply_bf16(g, z, scale, shift, mean, invstd, c1, c2, slope: float, dz, bias_partials=None,
                        peer: Optional[PeerTapsBF16] = None):
    pe, what = _peer_arg(peer, z, "norm_bwd_apply_bf16")
    n, P, ldz = _clx(z, BF16, what + " z")
    _, _, ldg = _clx(g, g.dtype, what + " g")
    _, _, lddz = _clx(dz, BF16, what + " dz")
    c = z.shape[-1]
    check(getattr(lib(), "mpgan_" + what)(g.data_ptr(), int(g.dtype == torch.float32), ldg, z.data_ptr(), ldz,
                                          scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                          c1.data_ptr(), c2.data_ptr(), *pe, float(slope), n * P, c, dz.data_ptr(), lddz,
                                          _ptr(bias_partials), _stream()), what)
    return dz


def norm_bwd_reduce_bf16_peer(g, z, scale, shift, mean, invstd, peer: PeerTapsBF16, slope: float, partials):
    norm_bwd_reduce_bf16(g, z, scale, shift, mean, invstd, slope, partials, peer=peer)


def norm_bwd_apply_bf16_peer(g, z, scale, shift, mean, invstd, c1, c2, peer: PeerTapsBF16, slope: float, dz,
                             bias_partials=None):
    return norm_bwd_apply_bf16(g, z, scale, shift, mean, invstd, c1, c2, slope, dz, bias_partials, peer=peer)


def tap_l1_bf16(za, scale_a, shift_a, zb, scale_b, shift_b, slope: float, partials, out3):
    """out3 = (mean|z_a-z_b|, mean|y_a-y_b|, mean|a_a-a_b|) over two passes' stored bf16 z (mpgan_tap_l1_bf16)."""
    n, P, lda = _clx(za, BF16, "tap_l1_bf16 a")
    _, _, ldb = _clx(zb, BF16, "tap_l1_bf16 b")
    if za.shape != zb.shape:
        raise ValueError("tap_l1_bf16: shape mismatch")
    if partials.numel() < tap_l1_partials():
        raise ValueError("tap_l1_bf16: partials too small")
    check(lib().mpgan_tap_l1_bf16(za.data_ptr(), lda, scale_a.data_ptr(), shift_a.data_ptr(), zb.data_ptr(), ldb,
                                  scale_b.data_ptr(), shift_b.data_ptr(), float(slope), n * P, za.shape[-1],
                                  partials.data_ptr(), out3.data_ptr(), _stream()), "tap_l1_bf16")
    return out3


# --------------------------------------------------------------------------
# BatchNorm statistics through accumulators + fold-on-load (csrc/norm_fold.h)
# --------------------------------------------------------------------------
def acc_buffer(c: int, device) -> torch.Tensor:
    """Zeroed int64 accumulators [ACC_REPLICAS][ACC_WORDS][c] for one norm layer fed by a c-channel conv."""
    return torch.zeros(ACC_REPLICAS * ACC_WORDS * c, dtype=torch.int64, device=device)


def conv_forward_fold(g: ConvGeom, x, w_packed, bias, y, *, pro: Optional[Prologue] = None, fold: Optional[NormFoldC] = None,
                      resid=None, tanh_out: bool = False, stats_acc=None):
    _check_in_out(g, x, y, "conv_forward_fold")
    _, _, ldx = _cl(x, "conv_forward_fold x")
    _, _, ldy = _cl(y, "conv_forward_fold y")
    ldr = _cl(resid, "conv_forward_fold resid")[2] if resid is not None else 0
    gc = g.c()
    if stats_acc is not None and (stats_acc.dtype != torch.int64 or stats_acc.numel() < ACC_REPLICAS * ACC_WORDS * g.cout):
        raise ValueError("conv_forward_fold: stats_acc must be int64 [ACC_REPLICAS][4][Cout]")
    check(lib().mpgan_conv_forward_fold(C.byref(gc), x.data_ptr(), ldx, w_packed.data_ptr(), _ptr(bias), _pro(pro),
                                        C.byref(fold) if fold is not None else None, _ptr(resid), ldr, int(tanh_out),
                                        None, _ptr(stats_acc), ACC_REPLICAS if stats_acc is not None else 0,
                                        y.data_ptr(), ldy, _stream()), "conv_forward_fold")
    return y


def norm_act_add_fold(z, pz: Prologue, fold: NormFoldC, r, pr: Optional[Prologue], out, *, tanh_out=False):
    n, P, ldz = _cl(z, "norm_act_add_fold z")
    _, _, ldo = _cl(out, "norm_act_add_fold out")
    ldr = _cl(r, "norm_act_add_fold r")[2] if r is not None else 0
    check(lib().mpgan_norm_act_add_fold(z.data_ptr(), ldz, _pro(pz), C.byref(fold), _ptr(r), ldr, _pro(pr), n, P,
                                        z.shape[-1], int(tanh_out), out.data_ptr(), ldo, _stream()), "norm_act_add_fold")
    return out


# ---- the pair losses (losses.py holds the autograd nodes) ----
_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}


def _nbytes(t) -> int:
    return 0 if t is None else t.numel() * t.element_size()


def _up_stride(upstream) -> int:
    """0: one upstream gradient for every item (a reduced loss); 1: one per batch entry."""
    return 0 if upstream.numel() == 1 else 1


# ---- Parzen-window mutual information (csrc/mi_loss.hip) ----


def parzen_mi_workspace(batch: int, numel_per_item: int, bins: int) -> int:
    need = int(lib().mpgan_parzen_mi_workspace(int(batch), int(numel_per_item), int(bins)))
    if need < 0:
        raise ValueError(f"parzen_mi_workspace: bad geometry (batch {batch}, {numel_per_item} per item, {bins} bins)")
    return need


def parzen_mi_forward(a, b, batch, ranges, bins, sigma_ratio, smooth_nr, smooth_dr, workspace, mi, joint=None,
                      coef=None, reduction="none", loss=None):
    """mi[batch] (float64) of two contiguous fp32 tensors; optionally the joint, the backward's coefficients and
    the reduced loss (see include/mpgan_hip.h)."""
    lo_a, hi_a, lo_b, hi_b = ranges
    check(lib().mpgan_parzen_mi_forward(a.data_ptr(), b.data_ptr(), a.numel() // batch, batch, lo_a, hi_a, lo_b, hi_b,
                                        int(bins), float(sigma_ratio), float(smooth_nr), float(smooth_dr),
                                        workspace.data_ptr(), _nbytes(workspace),
                                        _ptr(joint), mi.data_ptr(), _ptr(coef), _REDUCTIONS[reduction],
                                        _ptr(loss), _stream()), "parzen_mi_forward")
    return mi


def parzen_mi_backward(a, b, batch, ranges, bins, sigma_ratio, coef, upstream, scale, wrt, grad):
    """grad = upstream[item or 0] * scale * d mi[item] / d (a if wrt == 0 else b)."""
    lo_a, hi_a, lo_b, hi_b = ranges
    check(lib().mpgan_parzen_mi_backward(a.data_ptr(), b.data_ptr(), a.numel() // batch, batch, lo_a, hi_a, lo_b, hi_b,
                                         int(bins), float(sigma_ratio), coef.data_ptr(), upstream.data_ptr(),
                                         _up_stride(upstream), float(scale), int(wrt), grad.data_ptr(),
                                         _stream()), "parzen_mi_backward")
    return grad


# ---- SSIM loss (csrc/ssim_loss.hip; losses.py holds the autograd node) ----
def _dhw(spatial):
    return (C.c_int32 * 3)(*((1,) * (3 - len(spatial)) + tuple(int(s) for s in spatial)))


def ssim_loss_workspace(spatial, items: int, grad_mask: int, weighted: bool = False):
    """(workspace bytes, coefficient-buffer bytes) for `items` images of extent `spatial` ((H, W) or (D, H, W)); the
    weighted form (a mask, a threshold or stats) has one more int64 per tile for the counts."""
    coef = C.c_int64(0)
    query = lib().mpgan_masked_ssim_loss_workspace if weighted else lib().mpgan_ssim_loss_workspace
    need = int(query(_dhw(spatial), int(items), int(grad_mask), C.byref(coef)))
    if need < 0:
        raise ValueError(f"ssim_loss_workspace: bad geometry ({items} items of extent {tuple(spatial)}): extents below "
                         "the 7-wide window, or a depth that is neither 1 nor >= 7")
    return need, int(coef.value)


def ssim_loss_forward(a, b, spatial, items, channels, lo, hi, grad_mask, workspace, coef, reduction, loss, *, mask=None,
                      thr=None, stats=None, smap=None):
    """loss (fp32, reduced on the device) of two contiguous fp32 tensors; with grad_mask != 0 also the backward's
    coefficient maps (see include/mpgan_hip.h).  With stats ((items, 2) float64, receives (ssim_item, n_item)) the
    weighted entry point runs: at most one of mask (uint8) and thr (fp32 per item) weights the windows, and smap
    (fp32 [items][M]) receives S of every valid window."""
    head = (a.data_ptr(), b.data_ptr(), _dhw(spatial), int(items), int(channels), float(lo), float(hi))
    buffers = (int(grad_mask), workspace.data_ptr(), _nbytes(workspace), _ptr(coef), _nbytes(coef))
    tail = (_REDUCTIONS[reduction], loss.data_ptr(), _stream())
    if stats is None:
        if mask is not None or thr is not None or smap is not None:
            raise ValueError("ssim_loss_forward: mask, thr and smap need stats")
        check(lib().mpgan_ssim_loss_forward(*head, *buffers, *tail), "ssim_loss_forward")
    else:
        check(lib().mpgan_masked_ssim_loss_forward(*head, _ptr(mask), _ptr(thr), *buffers, stats.data_ptr(), _ptr(smap),
                                                   *tail), "masked_ssim_loss_forward")
    return loss


def ssim_loss_backward(a, b, spatial, items, channels, lo, grad_mask, coef, upstream, scale, wrt, grad, stats=None):
    """grad = upstream[batch entry or 0] * scale * d ssim_item / d (a if wrt == 0 else b); with the weighted forward's
    stats, its per-item divisors are read on the device and an empty item gets 0."""
    head = (a.data_ptr(), b.data_ptr(), _dhw(spatial), int(items), int(channels), float(lo), int(grad_mask),
            coef.data_ptr(), _nbytes(coef))
    tail = (upstream.data_ptr(), _up_stride(upstream), float(scale), int(wrt), grad.data_ptr(), _stream())
    if stats is None:
        check(lib().mpgan_ssim_loss_backward(*head, *tail), "ssim_loss_backward")
    else:
        check(lib().mpgan_masked_ssim_loss_backward(*head, stats.data_ptr(), *tail), "masked_ssim_loss_backward")
    return grad


# The weighted forward under its earlier names and argument order, for tests/test_masked_ssim_gpu.py alone, which calls
# these two (and no backward): no logic here, and nothing in the package uses them.  They go when that file moves to
# the wrappers above.
def masked_ssim_loss_workspace(spatial, items: int, grad_mask: int):
    return ssim_loss_workspace(spatial, items, grad_mask, weighted=True)


def masked_ssim_loss_forward(a, b, spatial, items, channels, lo, hi, mask, thr, grad_mask, workspace, coef, stats, smap,
                             reduction, loss):
    return ssim_loss_forward(a, b, spatial, items, channels, lo, hi, grad_mask, workspace, coef, reduction, loss,
                             mask=mask, thr=thr, stats=stats, smap=smap)


# ---- Sobel edge loss (csrc/edge_loss.hip; losses.py holds the autograd nodes) ----
def sobel_magnitude_forward(x, spatial, items, eps, out):
    """out = m(x), the Sobel edge magnitude of `items` contiguous fp32 images (see include/mpgan_hip.h)."""
    check(lib().mpgan_sobel_magnitude_forward(x.data_ptr(), _dhw(spatial), int(items), float(eps), out.data_ptr(),
                                              _stream()), "sobel_magnitude_forward")
    return out


def sobel_magnitude_backward(x, spatial, items, eps, dy, dx):
    """dx = the adjoint of m at x for the upstream map dy; recomputed from x."""
    check(lib().mpgan_sobel_magnitude_backward(x.data_ptr(), _dhw(spatial), int(items), float(eps), dy.data_ptr(),
                                               dx.data_ptr(), _stream()), "sobel_magnitude_backward")
    return dx


def edge_loss_workspace(spatial, items: int) -> int:
    """Workspace bytes for `items` images of extent `spatial` ((H, W) or (D, H, W))."""
    need = int(lib().mpgan_edge_loss_workspace(_dhw(spatial), int(items)))
    if need < 0:
        raise ValueError(f"edge_loss_workspace: bad geometry ({items} items of extent {tuple(spatial)})")
    return need


def edge_loss_forward(a, b, spatial, items, channels, eps, workspace, reduction, loss):
    """loss (fp32, reduced on the device) of two contiguous fp32 tensors; no magnitude map is written."""
    check(lib().mpgan_edge_loss_forward(a.data_ptr(), b.data_ptr(), _dhw(spatial), int(items), int(channels), float(eps),
                                        workspace.data_ptr(), _nbytes(workspace), _REDUCTIONS[reduction],
                                        loss.data_ptr(), _stream()), "edge_loss_forward")
    return loss


def edge_loss_backward(a, b, spatial, items, channels, eps, upstream, scale, wrt, grad):
    """grad = upstream[batch entry or 0] * scale * d loss_item / d (a if wrt == 0 else b)."""
    check(lib().mpgan_edge_loss_backward(a.data_ptr(), b.data_ptr(), _dhw(spatial), int(items), int(channels),
                                         float(eps), upstream.data_ptr(), _up_stride(upstream),
                                         float(scale), int(wrt), grad.data_ptr(), _stream()), "edge_loss_backward")
    return grad


# ---- foreground masks (csrc/foreground.hip; preprocess.py, losses.py and metrics.py hold the public functions) ----
def otsu_threshold(x, items, lo, hi, bins, thr):
    """thr[items] = Otsu's threshold of every item of the contiguous fp32 tensor x (see include/mpgan_hip.h)."""
    need = int(lib().mpgan_otsu_workspace(int(items), int(bins)))
    if need < 0:
        raise ValueError(f"otsu_threshold: bad geometry ({items} items, {bins} bins; bins must lie in [2, 256])")
    ws = torch.empty(need // 8, dtype=torch.int64, device=x.device)
    check(lib().mpgan_otsu_threshold(x.data_ptr(), x.numel() // int(items), int(items), float(lo), float(hi), int(bins),
                                     ws.data_ptr(), thr.data_ptr(), _stream()), "otsu_threshold")
    return thr


def foreground_mask(x, spatial, items, thr, margin=(0, 0, 0), mask=None, box=None, count=None):
    """Any of mask (uint8, x's shape), box (int32 (items, 2, 3)) and count (int64 (items,)) of x > thr[item]; margin
    is (z, y, x)."""
    mz, my, mx = (int(m) for m in margin)
    check(lib().mpgan_foreground_mask(x.data_ptr(), _dhw(spatial), int(items), thr.data_ptr(),
                                      (C.c_int32 * 3)(mz, my, mx), _ptr(mask), _ptr(box), _ptr(count), _stream()),
          "foreground_mask")


def masked_l1_forward(a, b, items, channels, mask, thr, w_fg, w_bg, den, reduction, loss):
    """loss (fp32, reduced on the device) and den[items] (float64) of the mask-weighted L1; one of mask, thr."""
    per_item = a.numel() // int(items)
    need = int(lib().mpgan_masked_l1_workspace(per_item, int(items)))
    if need < 0:
        raise ValueError(f"masked_l1_forward: bad geometry ({items} items of {per_item} values)")
    ws = torch.empty(need // 8, dtype=torch.float64, device=a.device)
    check(lib().mpgan_masked_l1_forward(a.data_ptr(), b.data_ptr(), per_item, int(items), int(channels), _ptr(mask),
                                        _ptr(thr), float(w_fg), float(w_bg), ws.data_ptr(), _nbytes(ws), den.data_ptr(),
                                        _REDUCTIONS[reduction], loss.data_ptr(), _stream()), "masked_l1_forward")
    return loss


def masked_l1_backward(a, b, items, channels, mask, thr, w_fg, w_bg, den, upstream, scale, da, db):
    """da and / or db = +-upstream[batch entry or 0] * scale * w_i * sign(a - b) / den_item."""
    check(lib().mpgan_masked_l1_backward(a.data_ptr(), b.data_ptr(), a.numel() // int(items), int(items), int(channels),
                                         _ptr(mask), _ptr(thr), float(w_fg), float(w_bg), den.data_ptr(),
                                         upstream.data_ptr(), _up_stride(upstream), float(scale), _ptr(da), _ptr(db),
                                         _stream()), "masked_l1_backward")


def masked_image_errors(a, b, mask, data_range, out4):
    """out4 (float64) = (MAE, MSE, PSNR, count) over the voxels whose mask byte is non-zero."""
    part = torch.empty(int(lib().mpgan_masked_errors_partials(a.numel())), dtype=torch.float64, device=a.device)
    check(lib().mpgan_masked_image_errors(a.data_ptr(), b.data_ptr(), mask.data_ptr(), a.numel(), float(data_range),
                                          part.data_ptr(), out4.data_ptr(), _stream()), "masked_image_errors")
    return out4


# ---- differentiable augmentation (csrc/diffaug.hip; augment.py holds the sampler and the autograd node) ----
DIFFAUG_BRIGHTNESS, DIFFAUG_CONTRAST, DIFFAUG_TRANSLATION, DIFFAUG_CUTOUT = 1, 2, 4, 8      # MPGAN_DIFFAUG_*


def _diffaug_geometry(x, what: str):
    """(n, spatial) of a contiguous fp32 (B, 1, *S) device tensor, S = (H, W) or (D, H, W)."""
    if x.dim() not in (4, 5) or x.shape[1] != 1:
        raise ValueError(f"{what}: need a (B, 1, H, W) or (B, 1, D, H, W) tensor, got {tuple(x.shape)}")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{what}: the image must be contiguous float32, got {x.dtype} with strides {x.stride()}")
    if not x.is_cuda:
        raise ValueError(f"{what}: every tensor must be on the GPU (there is no CPU path)")
    if x.numel() >= 2 ** 31:
        raise ValueError(f"{what}: {x.numel()} elements exceed the 32-bit count of mpgan_diffaug_*")
    return int(x.shape[0]), tuple(int(s) for s in x.shape[2:])


def _table(what: str, name: str, t, dtype, shape, device, required: bool = False):
    """The one check of a table argument: a contiguous `dtype` tensor of `shape` on `device`; None passes unless
    `required`."""
    if t is None and not required:
        return
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous()
            or t.device != device):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else repr(t)
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} {tuple(shape)} tensor on {device}, got {got}")


def _diffaug_tables(x, n, ops_mask, color, geom, workspace, spatial, what):
    if ops_mask & ~15:
        raise ValueError(f"{what}: unknown ops bits {ops_mask:#x}")
    for t, dtype, cols, name, used in ((color, torch.float32, 2, "color", ops_mask & 3), (geom, torch.int32, 9, "geom", ops_mask & 12)):
        if t is None and used:
            raise ValueError(f"{what}: ops {ops_mask:#x} need the {name} table")
        _table(what, name, t, dtype, (n, cols), x.device)
    if ops_mask & DIFFAUG_CONTRAST:
        need = diffaug_workspace(n, spatial)
        if (workspace is None or workspace.dtype != torch.float64 or not workspace.is_contiguous()
                or workspace.device != x.device or workspace.numel() * 8 < need):
            raise ValueError(f"{what}: contrast needs a contiguous float64 workspace of >= {need} bytes on {x.device}")


def diffaug_workspace(n: int, spatial) -> int:
    """Bytes of fp64 block partials diffaug_forward / diffaug_backward need with DIFFAUG_CONTRAST."""
    need = int(lib().mpgan_diffaug_workspace(int(n), _dhw(spatial)))
    if need < 0:
        check(-1, "diffaug_workspace")
    return need


def diffaug_forward(x, ops_mask: int, color, geom, fill: float, workspace, y):
    """y = the augmentation `ops_mask` (DIFFAUG_* bits) of x under the per-sample tables color (B, 2) float32 and
    geom (B, 9) int32 (include/mpgan_hip.h); workspace: float64, only with DIFFAUG_CONTRAST."""
    n, spatial = _diffaug_geometry(x, "diffaug_forward")
    if y.shape != x.shape:
        raise ValueError(f"diffaug_forward: y has shape {tuple(y.shape)}, x {tuple(x.shape)}")
    _diffaug_geometry(y, "diffaug_forward")
    _diffaug_tables(x, n, int(ops_mask), color, geom, workspace, spatial, "diffaug_forward")
    check(lib().mpgan_diffaug_forward(x.data_ptr(), n, _dhw(spatial), int(ops_mask), _ptr(color), _ptr(geom), float(fill),
                                      _ptr(workspace), workspace.numel() * 8 if workspace is not None else 0,
                                      y.data_ptr(), _stream()), "diffaug_forward")
    return y


def diffaug_backward(gy, ops_mask: int, color, geom, workspace, gx):
    """gx = the gradient of diffaug_forward's input for the output gradient gy, same tables (neither x nor y is needed)."""
    n, spatial = _diffaug_geometry(gy, "diffaug_backward")
    if gx.shape != gy.shape:
        raise ValueError(f"diffaug_backward: gx has shape {tuple(gx.shape)}, gy {tuple(gy.shape)}")
    _diffaug_geometry(gx, "diffaug_backward")
    _diffaug_tables(gy, n, int(ops_mask), color, geom, workspace, spatial, "diffaug_backward")
    check(lib().mpgan_diffaug_backward(gy.data_ptr(), n, _dhw(spatial), int(ops_mask), _ptr(color), _ptr(geom),
                                       _ptr(workspace), workspace.numel() * 8 if workspace is not None else 0,
                                       gx.data_ptr(), _stream()), "diffaug_backward")
    return gx


# ---- paired affine augmentation (csrc/pair_augment.hip; augment.py holds the sampler and the module) ----
WARP_CONSTANT, WARP_BORDER = 0, 1                                                            # MPGAN_WARP_*


def _warp_planes(what, names, a0, b0, a1=None, b1=None):
    """The planes of a warp call, `names` = what the caller calls (a0, b0, a1, b1): a0 and b0 are images
    (_diffaug_geometry) of one batch, rank and device; the second plane's a1 and b1 are both tensors or both None and have
    the first plane's shapes and device.  Returns (n, a0's spatial extent, b0's spatial extent)."""
    n, spatial_a = _diffaug_geometry(a0, what)
    _, spatial_b = _diffaug_geometry(b0, what)
    if b0.shape[0] != n or len(spatial_b) != len(spatial_a) or b0.device != a0.device:
        raise ValueError(f"{what}: {names[1]} has shape {tuple(b0.shape)} on {b0.device}, {names[0]} {tuple(a0.shape)} on "
                         f"{a0.device}")
    if (a1 is None) != (b1 is None):
        raise ValueError(f"{what}: {names[2]} and {names[3]} go together")
    if a1 is not None:
        _diffaug_geometry(a1, what)
        _diffaug_geometry(b1, what)
        if a1.shape != a0.shape or b1.shape != b0.shape or a1.device != a0.device or b1.device != a0.device:
            raise ValueError(f"{what}: the second plane has shapes {tuple(a1.shape)} / {tuple(b1.shape)}, the first "
                             f"{tuple(a0.shape)} / {tuple(b0.shape)}")
    return n, spatial_a, spatial_b


def _warp_mode_noise(what, mode, x1, noise0, noise1, sigma):
    """The forward warps' mode, and their one rule for noise: plane 1's field needs plane 1, sigma needs a field and a
    field sigma."""
    if mode not in (WARP_CONSTANT, WARP_BORDER):
        raise ValueError(f"{what}: unknown mode {mode!r}")
    if noise1 is not None and x1 is None:
        raise ValueError(f"{what}: noise1 without a second plane")
    if (sigma is None) != (noise0 is None and noise1 is None):
        raise ValueError(f"{what}: sigma goes with a noise field, and a noise field with sigma")


def _warp_tables(what, n, y0, theta, sigma, noise0, noise1, gamma=None):
    """The forward warps' tables, in the order they have always been checked in."""
    _table(what, "theta", theta, torch.float64, (n, 12), y0.device, required=True)
    _table(what, "sigma", sigma, torch.float32, (n, 2), y0.device)
    _table(what, "gamma", gamma, torch.float64, (n, 2), y0.device)
    _table(what, "noise0", noise0, torch.float32, y0.shape, y0.device)
    _table(what, "noise1", noise1, torch.float32, y0.shape, y0.device)


def affine_warp(x0, x1, theta, mode: int, fill0: float, fill1: float, noise0, noise1, sigma, y0, y1):
    """y_k = the trilinear resampling of x_k at c = A p + t under the per-sample theta (B, 12) float64, plus
    sigma[:, k] * noise_k where plane k has a noise field (include/mpgan_hip.h).  x1 / y1 None: one plane.  The
    outputs may have another spatial extent than the inputs."""
    n, spatial, out_spatial = _warp_planes("affine_warp", ("x0", "y0", "x1", "y1"), x0, y0, x1, y1)
    _warp_mode_noise("affine_warp", mode, x1, noise0, noise1, sigma)
    _warp_tables("affine_warp", n, y0, theta, sigma, noise0, noise1)
    check(lib().mpgan_affine_warp(x0.data_ptr(), _ptr(x1), n, _dhw(spatial), _dhw(out_spatial), theta.data_ptr(), int(mode),
                                  float(fill0), float(fill1), _ptr(noise0), _ptr(noise1), _ptr(sigma), y0.data_ptr(),
                                  _ptr(y1), _stream()), "affine_warp")
    return y0 if y1 is None else (y0, y1)


def affine_warp_backward(gy, theta, mode: int, gx):
    """gx = the gradient of affine_warp's input for the output gradient gy under the same theta (B, 12) float64: the
    exact adjoint of the WARP_CONSTANT forward, a deterministic gather (include/mpgan_hip.h).  gx has the forward's input
    shape and is overwritten everywhere; a sample whose theta is singular or reaches beyond MPGAN_WARP_REACH_MAX gets
    NaN.  WARP_BORDER has no backward."""
    n, out_spatial, spatial = _warp_planes("affine_warp_backward", ("gy", "gx"), gy, gx)
    if mode != WARP_CONSTANT:
        raise ValueError(f"affine_warp_backward: only WARP_CONSTANT ({WARP_CONSTANT}) has a backward, got mode {mode!r}")
    _table("affine_warp_backward", "theta", theta, torch.float64, (n, 12), gy.device, required=True)
    check(lib().mpgan_affine_warp_backward(gy.data_ptr(), n, _dhw(spatial), _dhw(out_spatial), theta.data_ptr(), int(mode),
                                           gx.data_ptr(), _stream()), "affine_warp_backward")
    return gx


def affine_warp_theta_workspace(n: int, out_spatial) -> int:
    """Bytes of fp64 tile partials affine_warp_backward_theta needs for n samples of output extent out_spatial."""
    need = int(lib().mpgan_affine_warp_theta_workspace(int(n), _dhw(out_spatial)))
    if need < 0:
        check(-1, "affine_warp_theta_workspace")
    return need


def affine_warp_backward_theta(x0, x1, gy0, gy1, theta, mode: int, fill0: float, fill1: float, gtheta=None):
    """gtheta (B, 12) float64 = the gradient of affine_warp's theta for the inputs x0 (and x1) and the output gradients
    gy0 (and gy1) under WARP_CONSTANT: fp64 throughout, two launches, no atomics, bitwise reproducible
    (include/mpgan_hip.h).  x1 and gy1 are both tensors or both None.  All eight corners of a cell count, so at an
    integer coordinate the derivative is the right-hand one.  gtheta is overwritten (allocated when None); the
    workspace is allocated here.  WARP_BORDER has no gradient in theta."""
    what = "affine_warp_backward_theta"
    n, spatial, out_spatial = _warp_planes(what, ("x0", "gy0", "x1", "gy1"), x0, gy0, x1, gy1)
    if mode != WARP_CONSTANT:
        raise ValueError(f"{what}: only WARP_CONSTANT ({WARP_CONSTANT}) has a gradient in theta, got mode {mode!r}")
    if gtheta is None:
        gtheta = torch.empty((n, 12), dtype=torch.float64, device=x0.device)
    _table(what, "theta", theta, torch.float64, (n, 12), x0.device, required=True)
    _table(what, "gtheta", gtheta, torch.float64, (n, 12), x0.device, required=True)
    ws = torch.empty(affine_warp_theta_workspace(n, out_spatial) // 8, dtype=torch.float64, device=x0.device)
    check(lib().mpgan_affine_warp_backward_theta(x0.data_ptr(), _ptr(x1), gy0.data_ptr(), _ptr(gy1), n, _dhw(spatial),
                                                 _dhw(out_spatial), theta.data_ptr(), int(mode), float(fill0), float(fill1),
                                                 ws.data_ptr(), ws.numel() * 8, gtheta.data_ptr(), _stream()), what)
    return gtheta


def deform_warp(x0, x1, theta, ctrl, gain, gain_planes: int, gamma, lo: float, hi: float, mode: int, fill0: float,
                fill1: float, noise0, noise1, sigma, y0, y1):
    """affine_warp with c = (A p + t) + u(p), u the cubic B-spline deformation of the lattice ctrl (B, 3, g_d, g_h, g_w)
    float64, then on the planes of the bit mask `gain_planes` v += (v - lo) * expm1(b(p)) with b the B-spline of the
    log-gain lattice gain (B, b_d, b_h, b_w) float64, then v = lo + (hi - lo) * ((v - lo) / (hi - lo)) ** gamma[:, k]
    (gamma (B, 2) float64), then the noise term (include/mpgan_hip.h).  ctrl, gain and gamma may each be None: that
    term is absent.  A 2-D image has lattices with g_d = 1."""
    n, spatial, out_spatial = _warp_planes("deform_warp", ("x0", "y0", "x1", "y1"), x0, y0, x1, y1)
    _warp_mode_noise("deform_warp", mode, x1, noise0, noise1, sigma)
    gain_planes = int(gain_planes)
    if gain_planes & ~3 or (gain is not None and not gain_planes) or (gain_planes & 2 and x1 is None):
        raise ValueError(f"deform_warp: gain_planes {gain_planes:#x} is a mask of the planes given (1 = plane 0, 2 = plane 1), "
                         "not 0 with a gain lattice")
    if (gain is not None or gamma is not None) and not float(hi) > float(lo):
        raise ValueError(f"deform_warp: the value range needs hi > lo, got [{lo}, {hi}]")
    out3 = (1,) * (3 - len(out_spatial)) + tuple(out_spatial)
    grids = {}
    for t, lead, name in ((ctrl, (n, 3), "ctrl"), (gain, (n,), "gain")):
        if t is None:
            grids[name] = None
            continue
        if (not isinstance(t, torch.Tensor) or t.dim() != len(lead) + 3 or tuple(t.shape[:len(lead)]) != lead
                or t.dtype != torch.float64 or not t.is_contiguous() or t.device != x0.device):
            raise ValueError(f"deform_warp: {name} must be a contiguous float64 {lead + ('g_d', 'g_h', 'g_w')} tensor on "
                             f"{x0.device}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")
        g = tuple(int(v) for v in t.shape[len(lead):])
        if any(gk != 1 if sk == 1 else not 4 <= gk <= 64 for gk, sk in zip(g, out3)):
            raise ValueError(f"deform_warp: the {name} lattice {g} over the output extent {out3}: 1 on an axis of extent 1, "
                             "else 4 .. 64")
        grids[name] = g
    _warp_tables("deform_warp", n, y0, theta, sigma, noise0, noise1, gamma)
    check(lib().mpgan_deform_warp(x0.data_ptr(), _ptr(x1), n, _dhw(spatial), _dhw(out_spatial), theta.data_ptr(),
                                  _ptr(ctrl), _dhw(grids["ctrl"]) if ctrl is not None else None,
                                  _ptr(gain), _dhw(grids["gain"]) if gain is not None else None,
                                  gain_planes if gain is not None else 0, _ptr(gamma), float(lo), float(hi), int(mode),
                                  float(fill0), float(fill1), _ptr(noise0), _ptr(noise1), _ptr(sigma), y0.data_ptr(),
                                  _ptr(y1), _stream()), "deform_warp")
    return y0 if y1 is None else (y0, y1)


# --------------------------------------------------------------------------
# conditional discriminator: the first conv over two 1-channel input planes (include/mpgan_hip.h: mpgan_conv2p_*)
# --------------------------------------------------------------------------
def _check_planes(g: ConvGeom, x_img, x_cond, y, ydtype, what):
    """The two input planes (dense fp32, n * prod(in_dhw) elements each, any shape) and the channels-last output."""
    want = g.n * g.in_dhw[0] * g.in_dhw[1] * g.in_dhw[2]
    for name, t in (("x_img", x_img), ("x_cond", x_cond)):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != want:
            raise ValueError(f"{what}: {name} must be a contiguous CUDA fp32 plane of {want} elements, got "
                             f"{tuple(t.shape)} {t.dtype} {t.device}")
    if g.cin != 2:
        raise ValueError(f"{what}: a geometry with two input channels, got cin = {g.cin}")
    if tuple(y.shape) != (g.n, *g.out_dhw, g.cout):
        raise ValueError(f"{what}: output shape {tuple(y.shape)} != {(g.n, *g.out_dhw, g.cout)}")
    return _clx(y, ydtype, what + " y")[2]


def conv2p_stats_rows(g: ConvGeom, out_bf16: bool) -> int:
    gc = g.c()
    return int(lib().mpgan_conv2p_stats_rows(C.byref(gc), int(out_bf16)))


def conv2p_kernel_name(g: ConvGeom, out_bf16: bool) -> str:
    gc = g.c()
    buf = C.create_string_buffer(160)
    check(lib().mpgan_conv2p_kernel_name(C.byref(gc), int(out_bf16), buf, len(buf)), "conv2p_kernel_name")
    return buf.value.decode()


def conv2p_forward(g: ConvGeom, x_img, x_cond, w_packed, bias, y, *, stats_partials=None):
    """y = conv(cat(x_img, x_cond)) + bias; y fp32, or bf16 (then stats_partials may receive the fused statistics rows)."""
    bf = y.dtype == BF16
    what = "conv2p_forward_f32_to_bf16" if bf else "conv2p_forward"
    ldy = _check_planes(g, x_img, x_cond, y, y.dtype, what)
    if w_packed.numel() < g.cout * 2 * g.taps:
        raise ValueError(f"{what}: packed weight too small")
    if stats_partials is not None and stats_partials.numel() < conv2p_stats_rows(g, bf) * 2 * g.cout:
        raise ValueError(f"{what}: stats_partials too small")
    gc = g.c()
    check(getattr(lib(), "mpgan_" + what)(C.byref(gc), x_img.data_ptr(), x_cond.data_ptr(), w_packed.data_ptr(), _ptr(bias),
                                          _ptr(stats_partials), y.data_ptr(), ldy, _stream()), what)
    return y


def conv2p_forward_act(g: ConvGeom, x_img, x_cond, w_packed, scale, shift, slope, y):
    """Eval mode: y = lrelu(conv(cat(x_img, x_cond)) * scale + shift, slope), stored once as fp32 or bf16 (y's dtype)."""
    bf = y.dtype == BF16
    what = "conv2p_forward_act_f32_to_bf16" if bf else "conv2p_forward_act"
    ldy = _check_planes(g, x_img, x_cond, y, y.dtype, what)
    _check_epi(g, scale, shift, slope, what)
    gc = g.c()
    args = (C.byref(gc), x_img.data_ptr(), x_cond.data_ptr(), w_packed.data_ptr(), scale.data_ptr(), shift.data_ptr(),
            slope.data_ptr())
    if bf:
        check(lib().mpgan_conv2p_forward_act_f32_to_bf16(*args, None, y.data_ptr(), ldy, _stream()), what)
    else:
        check(lib().mpgan_conv2p_forward_act(*args, y.data_ptr(), ldy, _stream()), what)
    return y


def conv2p_wgrad_workspace(g: ConvGeom) -> int:
    gc = g.c()
    return int(lib().mpgan_conv2p_wgrad_workspace(C.byref(gc)))


def conv2p_wgrad_kernel_name(g: ConvGeom, bf16_dy: bool) -> str:
    gc = g.c()
    buf = C.create_string_buffer(160)
    check(lib().mpgan_conv2p_wgrad_kernel_name(C.byref(gc), int(bf16_dy), buf, len(buf)), "conv2p_wgrad_kernel_name")
    return buf.value.decode()


def conv2p_backward_weight(g: ConvGeom, x_img, x_cond, dy, dw, workspace, *, beta: float = 0.0, dbias=None):
    """dw (64, 2, k...) = beta*dw + the weight gradient over both planes, dy fp32 or bf16; dbias rides along."""
    what = "conv2p_backward_weight"
    lddy = _check_planes(g, x_img, x_cond, dy, dy.dtype, what)
    if dy.dtype not in (torch.float32, BF16):
        raise ValueError(f"{what}: dy must be fp32 or bf16")
    if dw.dtype != torch.float32 or dw.numel() != g.cout * 2 * g.taps or not dw.is_contiguous():
        raise ValueError(f"{what}: dw must be the contiguous fp32 torch-layout weight gradient")
    gc = g.c()
    check(lib().mpgan_conv2p_backward_weight(C.byref(gc), x_img.data_ptr(), x_cond.data_ptr(), dy.data_ptr(), lddy,
                                             int(dy.dtype == BF16), dw.data_ptr(), _ptr(dbias), float(beta),
                                             workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                             _stream()), what)
    return dw


def pack_weight_plane0_bwd(w: torch.Tensor) -> torch.Tensor:
    """Layout 3 of mpgan_pack_weights for ONE ConvNd weight: [tap][cout] of input channel 0 -- what backward-data of the
    image plane of a two-plane conv consumes (with the geometry's cin set to 1)."""
    w = w.contiguous()
    cout, cin = w.shape[0], w.shape[1]
    taps = w.numel() // (cin * cout)
    table = torch.tensor([[0, 0, cout, cin, taps, 0, 3, 0]], dtype=torch.int64, device=w.device)
    packed = torch.empty(cout * taps, dtype=torch.float32, device=w.device)
    pack_weights(w, packed, table, 1, w.numel())
    return packed
