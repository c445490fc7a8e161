"""A plain high-precision reference of every convolution the HIP kernels compute, and the two check tiers the
full-size launch tests (tests/test_step_launches_gpu.py) hold them to.

The reference shares no code with any convolution library: every operation is a sum over taps of strided-slice
GEMMs, `x[..., tap-shifted view] @ w_tap`, in torch on whatever device the tensors are on.  Tensors are
channels-last (N, D, H, W, C); a 2-D layer is a 3-D one with D = 1 and kernel / stride / pad 1 / 1 / 0 in depth.
Weights are in torch layout: (Cout, Cin, kz, ky, kx) for a ConvNd, (Cin, Cout, kz, ky, kx) for a ConvTransposeNd.
The same routine gives, run on |operands|, `absref` (the magnitude sum behind each output element, the base of
every error budget) and, run in float32 with TF32 off, the fp32 yardstick `ref32`.  The batch is walked one
sample at a time so that the routine's extra memory stays a few sample-sized fp64 tensors.

Check tiers:
  * tier X (exact): operands are small integers (prologue scales +-2^k, shift 0, slope 0.25) chosen so that
    every partial sum of every output is a dyadic number with at most 3 fractional bits below 2^21 in magnitude;
    any fp32 summation order is then exact and the output must equal `ref` (`bf16_rne(ref)` for a bf16 output)
    bit for bit -- no tolerance.  Only the tanh epilogue is held to 2^-20 (the kernel's tanh is not fp64's).
  * tier R (random): operands uniform in (-1, 1), rounded where the contract rounds, and two rules:
      elementwise  |got - ref| <= d_out (|ref| + L 2^-24 absref) + L 2^-24 absref,  d_out = 2^-8 for a bf16 output
                   (0 otherwise; the RNE rounds the fp32 accumulation, not ref), L = K + 2 + (roundings of the fused
                   prologue / epilogue), K the reduction length;
      norm-wise    ||got - ref|| <= 4 ||ref32 - ref|| + 1.1 ||bf16(ref) - ref|| (the last term for bf16 outputs).
Fused reductions (statistics rows, bias gradients, norm-backward sums) are exact in tier X wherever the magnitude sums
allow it (below 2^24 per channel); otherwise they are held to (L + 1) 2^-24 sum|terms| with L the longest fp32 chain
the kernel's row structure allows (row_chain).
"""
from __future__ import annotations

import contextlib
import math

import torch

ACT_NONE, ACT_LEAKY = 0, 1
U = 2.0 ** -24                  # fp32 unit roundoff
EXACT_LIMIT = 2.0 ** 21          # tier X: |partial sums| below this, with <= 3 fractional bits, are exact in fp32


def out_extent(in_dhw, k, stride, pad, transposed=False, out_pad=(0, 0, 0)):
    if transposed:
        return tuple((i - 1) * s - 2 * p + kk + op for i, kk, s, p, op in zip(in_dhw, k, stride, pad, out_pad))
    return tuple((i + 2 * p - kk) // s + 1 for i, kk, s, p in zip(in_dhw, k, stride, pad))


def _taps(k):
    for kz in range(k[0]):
        for ky in range(k[1]):
            for kx in range(k[2]):
                yield (kz, ky, kx), (kz * k[1] + ky) * k[2] + kx


def _sl(start, count, step):
    return slice(start, start + (count - 1) * step + 1, step)


# ------------------------------------------------------------------ the two gathers every operation is made of
def _gather_conv(x, wt, k, stride, pad, out_dhw):
    """y[n, o] = sum_tap x_padded[n, o*s + tap] @ wt[tap]   (x: (N,D,H,W,Ci), wt: (T, Ci, Co))."""
    n, D, H, W, ci = x.shape
    ext = [max(i + 2 * p, (o - 1) * s + kk) for i, p, o, s, kk in zip((D, H, W), pad, out_dhw, stride, k)]
    xp = x.new_zeros(n, *ext, ci)
    xp[:, pad[0]:pad[0] + D, pad[1]:pad[1] + H, pad[2]:pad[2] + W] = x
    y = x.new_zeros(n, *out_dhw, wt.shape[-1])
    for (kz, ky, kx), t in _taps(k):
        v = xp[:, _sl(kz, out_dhw[0], stride[0]), _sl(ky, out_dhw[1], stride[1]), _sl(kx, out_dhw[2], stride[2])]
        y += v @ wt[t]
    return y


def _scatter_conv(x, wt, k, stride, pad, out_dhw):
    """y[n, i*s + tap - pad] += x[n, i] @ wt[tap]   (the transposed gather; x: (N,Di,Hi,Wi,Ci), wt: (T, Ci, Co))."""
    n, D, H, W, ci = x.shape
    ext = [max((i - 1) * s + kk, p + o) for i, s, kk, p, o in zip((D, H, W), stride, k, pad, out_dhw)]
    y = x.new_zeros(n, *ext, wt.shape[-1])
    for (kz, ky, kx), t in _taps(k):
        y[:, _sl(kz, D, stride[0]), _sl(ky, H, stride[1]), _sl(kx, W, stride[2])] += x @ wt[t]
    return y[:, pad[0]:pad[0] + out_dhw[0], pad[1]:pad[1] + out_dhw[1], pad[2]:pad[2] + out_dhw[2]]


def _per_sample(fn, x, *rest):
    return torch.cat([fn(x[i:i + 1], *rest) for i in range(x.shape[0])])


# ------------------------------------------------------------------ the four operations
def conv_forward(a, w, k, stride, pad, out_dhw, transposed=False):
    """Forward of ConvNd (w: (Co, Ci, k..)) or ConvTransposeNd (w: (Ci, Co, k..)) on the activated input a."""
    T = k[0] * k[1] * k[2]
    if transposed:
        wt = w.reshape(w.shape[0], w.shape[1], T).permute(2, 0, 1)
        return _per_sample(_scatter_conv, a, wt, k, stride, pad, out_dhw)
    wt = w.reshape(w.shape[0], w.shape[1], T).permute(2, 1, 0)
    return _per_sample(_gather_conv, a, wt, k, stride, pad, out_dhw)


def conv_backward_data(dy, w, k, stride, pad, in_dhw, transposed=False):
    """Gradient w.r.t. the layer's input: the adjoint of conv_forward."""
    T = k[0] * k[1] * k[2]
    if transposed:
        wt = w.reshape(w.shape[0], w.shape[1], T).permute(2, 1, 0)
        return _per_sample(_gather_conv, dy, wt, k, stride, pad, in_dhw)
    wt = w.reshape(w.shape[0], w.shape[1], T).permute(2, 0, 1)
    return _per_sample(_scatter_conv, dy, wt, k, stride, pad, in_dhw)


def conv_backward_weight(a, dy, k, stride, pad, transposed=False):
    """Weight gradient in torch layout, summed over the batch one sample at a time."""
    T = k[0] * k[1] * k[2]
    ci, co = a.shape[-1], dy.shape[-1]
    dw = a.new_zeros(T, ci, co)
    for i in range(a.shape[0]):
        x, g = a[i:i + 1], dy[i:i + 1]
        if transposed:
            ext = [max((d - 1) * s + kk, p + o) for d, s, kk, p, o in zip(x.shape[1:4], stride, k, pad, g.shape[1:4])]
            gp = g.new_zeros(1, *ext, co)
            gp[:, pad[0]:pad[0] + g.shape[1], pad[1]:pad[1] + g.shape[2], pad[2]:pad[2] + g.shape[3]] = g
            xf = x.reshape(-1, ci).t()
            for (kz, ky, kx), t in _taps(k):
                v = gp[:, _sl(kz, x.shape[1], stride[0]), _sl(ky, x.shape[2], stride[1]), _sl(kx, x.shape[3], stride[2])]
                dw[t] += xf @ v.reshape(-1, co)
        else:
            D, H, W = x.shape[1:4]
            o = g.shape[1:4]
            ext = [max(d + 2 * p, (oo - 1) * s + kk) for d, p, oo, s, kk in zip((D, H, W), pad, o, stride, k)]
            xp = x.new_zeros(1, *ext, ci)
            xp[:, pad[0]:pad[0] + D, pad[1]:pad[1] + H, pad[2]:pad[2] + W] = x
            gf = g.reshape(-1, co)
            for (kz, ky, kx), t in _taps(k):
                v = xp[:, _sl(kz, o[0], stride[0]), _sl(ky, o[1], stride[1]), _sl(kx, o[2], stride[2])]
                dw[t] += v.reshape(-1, ci).t() @ gf
    if transposed:
        return dw.permute(1, 2, 0).reshape(ci, co, *k)
    return dw.permute(2, 1, 0).reshape(co, ci, *k)


def bias_grad(dy):
    return dy.reshape(-1, dy.shape[-1]).sum(0)


# ------------------------------------------------------------------ fused extras
def prologue(z, scale, shift, n_stride=0, act=ACT_NONE, slope=1.0, absolute=False):
    """a = act(z*scale + shift): per channel (n_stride = 0) or per (sample, channel) (scale / shift (N, C)).
    absolute: the magnitude |z||scale| + |shift| that bounds |a| and the rounding of its two fp32 operations."""
    shp = (z.shape[0], 1, 1, 1, z.shape[-1]) if n_stride else (1, 1, 1, 1, z.shape[-1])
    s, t = scale.reshape(shp).to(z.dtype), shift.reshape(shp).to(z.dtype)
    if absolute:
        return z.abs() * s.abs() + t.abs()
    u = z * s + t
    return torch.where(u < 0, u * slope, u) if act == ACT_LEAKY else u


def act_epilogue(y, scale, shift, slope, absolute=False):
    """prelu(y*scale[c] + shift[c], slope[c]) of mpgan_conv_forward_act (absolute: y is a magnitude sum)."""
    s, t, a = (v.reshape(1, 1, 1, 1, -1).to(y.dtype) for v in (scale, shift, slope))
    if absolute:
        return (y * s.abs() + t.abs()) * torch.clamp(a.abs(), min=1.0)
    u = y * s + t
    return torch.where(u < 0, u * a, u)


def stats_sums(y):
    """Fused BatchNorm statistics: (sum y, sum y^2) per channel over every pixel; with the magnitude sums."""
    f = y.reshape(-1, y.shape[-1])
    return torch.stack([f.sum(0), (f * f).sum(0)]), torch.stack([f.abs().sum(0), (f * f).sum(0)])


def norm_bwd_sums(g, z, scale, shift, mean, invstd, slope, third=True):
    """The norm-backward sums a backward-data launch leaves for the BatchNorm + LeakyReLU in front of its output
    (as mpgan_norm_bwd_reduce forms them from the stored gradient g and z): sum gy, sum gy*zhat, sum g*min(y, 0)
    (the third is zero on the bf16 path), gy = g * LeakyReLU'(y), y = z*scale + shift, zhat = (z - mean)*invstd.
    Returns (sums (3, C), magnitude sums (3, C))."""
    c = z.shape[-1]
    g, z = g.reshape(-1, c), z.reshape(-1, c)
    y = z * scale + shift
    neg = y < 0
    gy = torch.where(neg, g * slope, g)
    zh = (z - mean) * invstd
    t3_ = torch.where(neg, g * y, torch.zeros_like(y)) if third else torch.zeros_like(y)
    terms = [gy, gy * zh, t3_]
    return torch.stack([t.sum(0) for t in terms]), torch.stack([t.abs().sum(0) for t in terms])


# ------------------------------------------------------------------ rounding helpers (the contracts of DESIGN.md 3a / 3b)
def bf16_rne(t):
    """Round to bf16 (nearest even) and back, in t's dtype (via fp32: exact for every value tier X produces)."""
    return t.float().to(torch.bfloat16).to(t.dtype)


def bf16_trunc(t):
    """Round toward zero to bf16 (a planted fault: truncation instead of RNE)."""
    b = t.float().contiguous().view(torch.int32) & -65536
    return b.view(torch.float32).to(t.dtype)


def mm16_operands(a, w):
    """bf16 matrix operands (oracle/mm16_emul.py): the activated input and the weights are rounded as they enter the
    matrix cores (the bias gradient sums the unrounded dy)."""
    return bf16_rne(a), bf16_rne(w)


@contextlib.contextmanager
def no_tf32():
    """fp32 GEMMs as fp32 (set and restored explicitly)."""
    old = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = old


# ------------------------------------------------------------------ the two tiers
def check_exact(got, ref, bf16_out=False, tanh=False):
    """Tier X.  got: the kernel's output (any dtype); ref: the fp64 reference of exact operands (pre-tanh when
    `tanh`).  Returns (ok, message)."""
    g = got.double()
    if tanh:
        want = torch.tanh(ref)
        bad = ~((g - want).abs() <= 2.0 ** -20)
    else:
        want = bf16_rne(ref) if bf16_out else ref
        bad = ~(g == want)
    nbad = int(bad.sum().item())
    if not nbad:
        return True, "exact"
    idx = bad.reshape(-1).nonzero()[0].item()
    return False, (f"{nbad}/{bad.numel()} elements differ; first at flat index {idx}: got "
                   f"{g.reshape(-1)[idx].item()!r} want {want.reshape(-1)[idx].item()!r}")


class RandomCheck:
    """Tier R over chunks of one output (the full-size test walks the batch one sample at a time):
      elementwise  |got - ref| <= d_out (|ref| + L 2^-24 absref) + L 2^-24 absref  (+ 2^-21 behind a tanh),
                   the RNE to a bf16 output rounds the fp32 accumulation, which sits within L 2^-24 absref of ref;
      norm-wise    ||got - ref|| <= 4 ||ref32 - ref|| + 1.1 ||bf16(ref) - ref|| (the last term for bf16 outputs).
    ref / absref / ref32 are pre-tanh when `tanh` (tanh is 1-Lipschitz)."""

    def __init__(self, L, bf16_out=False, tanh=False):
        self.L, self.bf16_out, self.tanh = L, bf16_out, tanh
        self.re, self.e2, self.d32, self.dbf, self.finite = 0.0, 0.0, 0.0, 0.0, True

    def add(self, got, ref, absref, ref32):
        g = got.double()
        if self.tanh:
            ref_o, ref32_o, extra = torch.tanh(ref), torch.tanh(ref32.double()), 2.0 ** -21
        else:
            ref_o, ref32_o, extra = ref, ref32.double(), 0.0
        err = (g - ref_o).abs()
        if not bool(torch.isfinite(err).all()):
            self.finite = False
            return
        acc = self.L * U * absref
        bound = (2.0 ** -8 if self.bf16_out else 0.0) * (ref_o.abs() + acc) + acc + extra
        self.re = max(self.re, float((err / bound.clamp_min(1e-300)).max().item()))
        self.e2 += float((err * err).sum().item())
        self.d32 += float(((ref32_o - ref_o) ** 2).sum().item())
        if self.bf16_out:
            self.dbf += float(((bf16_rne(ref_o) - ref_o) ** 2).sum().item())

    def result(self):
        """(ok, elementwise ratio, norm-wise ratio); ok means both ratios are <= 1."""
        if not self.finite:
            return False, math.inf, math.inf
        nb = 4.0 * math.sqrt(self.d32) + 1.1 * math.sqrt(self.dbf)
        rn = math.sqrt(self.e2) / nb if nb > 0 else (0.0 if self.e2 == 0 else math.inf)
        return self.re <= 1.0 and rn <= 1.0, self.re, rn


def check_random(got, ref, absref, ref32, L, bf16_out=False, tanh=False):
    """Tier R on one whole output (RandomCheck with a single chunk)."""
    c = RandomCheck(L, bf16_out, tanh)
    c.add(got, ref, absref, ref32)
    return c.result()


# ------------------------------------------------------------------ fused reductions
ROW_SLACK = 512     # pixels of the largest tile (8x8x8, 512 x 128): a persistent block may walk one tile more than the average


def row_chain(M, rows):
    """Longest fp32 addition chain inside one partial row of a kernel that leaves `rows` rows over M pixels (the rows
    themselves are added in fp64 by the tests): twice the average share -- ragged tiles cover more than M pixels -- plus
    one tile."""
    return 2 * -(-M // rows) + ROW_SLACK


def exact_sums_ok(mag, frac_bits=0):
    """Every partial sum of terms with at most `frac_bits` fractional bits is exact in fp32 when sum|terms| < 2^24."""
    return bool((mag * 2.0 ** frac_bits < 2.0 ** 24).all())


def check_sums(got, want, mag, L, exact=False, extra=None):
    """A fused reduction the kernel sums in fp32.  exact: |terms| are dyadic with sum|terms| below 2^24 (the caller has
    checked it with exact_sums_ok) -- every order is exact and got must equal want.  Otherwise
    |got - want| <= (L + 1) 2^-24 sum|terms| (+ extra: what the kernel's own terms may differ from the reference's),
    L the longest fp32 addition chain.  Returns (ok, ratio); ratio 0 means exact."""
    g = got.double()
    if not bool(torch.isfinite(g).all()):
        return False, math.inf
    err = (g - want).abs()
    if exact:
        return bool((err == 0).all()), (0.0 if bool((err == 0).all()) else math.inf)
    bound = (L + 1) * U * mag + (0.0 if extra is None else extra)
    ratio = float((err / bound.clamp_min(1e-300)).max().item())
    return ratio <= 1.0, ratio


def stats_terms(y_ref, y_abs, L_el):
    """One chunk of a conv output's fused BatchNorm statistics (additive over chunks): the fp64 sums (sum y, sum y^2),
    their magnitude sums, and how far the kernel's sums may sit from them because its own y may differ from y_ref by
    e = L_el 2^-24 y_abs per element (L_el = 0 where y is exact): sum e and sum e (2|y| + e)."""
    want, mag = stats_sums(y_ref)
    f = y_ref.reshape(-1, y_ref.shape[-1])
    e = L_el * U * y_abs.reshape(-1, y_abs.shape[-1])
    return want, mag, torch.stack([e.sum(0), (e * (2 * f.abs() + e)).sum(0)])


def stats_check(got, want, mag, extra, M, rows, exact=False):
    """got: the kernel's partial rows [rows][2][C] added in fp64.  exact: integer y whose magnitude sums are below 2^24
    (checked by the caller) -- got must equal want.  Otherwise a row adds at most row_chain(M, rows) terms and y^2 costs
    one more rounding."""
    if exact:
        return check_sums(got, want, mag, 0, exact=True)
    return check_sums(got, want, mag, row_chain(M, rows) + 1, extra=extra)
