"""A plain fp64 restatement of every non-convolution launch of a training / inference step (BatchNorm statistics and
finalize, norm + activation apply, the norm backward and its bf16 twins, partial-row reductions, the Linear head,
tanh / sigmoid backward, the bf16 weight pack, the eval-mode epilogue vectors, L1 / BCE and Adam), the longest fp32
chain of each reduction as the kernels' code walks it, and the bounds the full-size replay
(tests/test_step_norm_launches_gpu.py) holds them to.

Tensors are (N, P, C): sample, pixel, channel (the channels-last rows the kernels stream, pitch removed).  Everything
here runs in whatever dtype / device the caller passes (fp64 for the reference).  Shared pieces come from conv_ref.

Tiers:
  * tier X (exact): dyadic operands whose magnitude sums stay below 2^24 per channel; every partial row, sum and
    elementwise output must equal the reference bit for bit (after one RNE for a bf16 output).  Finalize outputs,
    which divide and take a square root, are held to 1 ulp (invstd) / 2 ulp (scale, shift, running statistics) of the
    fp64 formula evaluated on the kernel's own fp32 mean and invstd (which allows FMA contraction).
  * tier R (random): offset operands; a sum of fp32 terms is within (L + 1) 2^-24 sum|terms|, L = the longest chain
    (chain_length); the variance E[z^2] - E[z]^2 is within var_bound (its error scales with E[z^2], not with the
    variance) and that error is propagated to invstd, scale, shift and the running variance.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from conv_ref import U, bf16_rne, check_sums, exact_sums_ok, norm_bwd_sums, prologue, stats_sums  # noqa: F401 (re-exported)

ACT_NONE, ACT_LEAKY = 0, 1
COMPACT_ROWS = 32          # partials_compact_kernel's output rows
COMPACT_ABOVE = 16384      # mpgan_norm_finalize_strided folds first when n * chunks exceeds this
WIDE_FINALIZE = 256        # norm_finalize_wide_kernel from this many rows (else one wave per channel)
WIDE_BWD_FINALIZE = 512    # norm_bwd_finalize_wide_kernel from this many rows


# ------------------------------------------------------------------ host geometry (the kernels' own rules)
def stats_chunks(P, C=0):
    """stats_chunks_host (norm_ops.hip): chunks per sample of channel_stats / norm_bwd_reduce."""
    rows = 256
    if C >= 4 and C % 4 == 0:
        R = max(256 // (C // 4), 1)
        rows = min(max(4 * R, 16), 256)
    return int(min(max(P // rows, 1), 256))


def bwd_rows_bf16(rows, C):
    """mpgan_norm_bwd_rows_bf16: blocks (= partial rows) of the bf16 reduce / apply passes."""
    R = 256 // (C // 8)
    return int(min(max(-(-rows // (R * 32)), 1), 2048))


def chunk_per(P, chunks):
    return -(-P // chunks)


def fold_chain(R, W):
    """fold_rows: additions a row slot's value goes through when the block folds R slots of W values."""
    G = 256 // W
    if G >= 2 and R >= 2 * G:
        return -(-R // G) + G
    return R


def finalize_form(n, chunks, instance=False):
    """(form, rows the finalize kernel reads): 'compact' (partials_compact_kernel first, then the narrow kernel over
    32 rows), 'wide' (block per channel) or 'narrow' (wave per channel)."""
    rows = n * chunks
    if not instance and rows > COMPACT_ABOVE:
        return "compact", COMPACT_ROWS
    if not instance and rows >= WIDE_FINALIZE:
        return "wide", rows
    return "narrow", rows


def chain_length(kind, P=0, C=1, vec=True, rows=0, n=1, chunks=0, instance=False):
    """Longest fp32 addition chain of one reduction, following the kernels' code.
      'reduce' (channel_stats, NQ = 2; norm_bwd_reduce, NQ = 3): chunk of per = ceil(P / chunks) pixels, R = 256 / (C / V)
          rows per pass, so ceil(per / R) additions per thread, then fold_rows over R slots of NQ * C values;
      'reduce3': the same with NQ = 3;
      'reduce_bf16' (norm_bwd_reduce_bf16 over `rows` rows): per = ceil(rows / blocks), R = 256 / (C / 8), then R slots;
      'finalize': the rows are added in fp64 (0) unless the compact fold runs first: + ceil(rows / 128) per lane + 3;
      'bias_bf16' (norm_bwd_apply_bf16's bias partials): ceil(rows / (blocks R)) per thread + R slots."""
    if kind in ("reduce", "reduce3"):
        nq = 2 if kind == "reduce" else 3
        V = 4 if vec else 1
        R = 256 // (C // V)
        ch = chunks or stats_chunks(P, C)
        return -(-chunk_per(P, ch) // R) + fold_chain(R, nq * C)
    if kind == "reduce_bf16":
        R = 256 // (C // 8)
        nb = bwd_rows_bf16(rows, C)
        return -(-chunk_per(rows, nb) // R) + R
    if kind == "bias_bf16":
        R = 256 // (C // 8)
        nb = bwd_rows_bf16(rows, C)
        return -(-rows // (nb * R)) + R
    if kind == "finalize":
        form, _ = finalize_form(n, chunks, instance)
        return -(-(n * chunks) // 128) + 3 if form == "compact" else 0
    raise ValueError(kind)


# ------------------------------------------------------------------ row-structured reductions
def chunk_rows(t, chunks):
    """t (N, P, Q): sums over each chunk [k per, min(P, (k+1) per)) of every sample -> (N * chunks, Q)."""
    N, P, Q = t.shape
    per = chunk_per(P, chunks)
    pad = per * chunks - P
    if pad:
        t = torch.cat([t, t.new_zeros(N, pad, Q)], 1)
    return t.reshape(N, chunks, per, Q).sum(2).reshape(N * chunks, Q)


def channel_stats_rows(z, chunks):
    """channel_stats: rows [N*chunks][2][C] of (sum z, sum z^2) and their magnitude rows."""
    C = z.shape[-1]
    rows = chunk_rows(torch.cat([z, z * z], -1), chunks).reshape(-1, 2, C)
    mag = chunk_rows(torch.cat([z.abs(), z * z], -1), chunks).reshape(-1, 2, C)
    return rows, mag


def _bwd_terms(g, z, scale, shift, mean, invstd, act, slope, third=True):
    """Per-pixel terms of the norm backward: gy, gy*zhat, g*y where y < 0 (zero without `third`); scale etc. are
    broadcastable to z (per channel (1, 1, C) or per sample (N, 1, C))."""
    y = z * scale + shift
    neg = (y < 0) if act == ACT_LEAKY else torch.zeros_like(y, dtype=torch.bool)
    gy = torch.where(neg, g * slope, g)
    zh = (z - mean) * invstd
    t3 = torch.where(neg, g * y, torch.zeros_like(y)) if third else torch.zeros_like(y)
    return gy, gy * zh, t3, zh


def norm_bwd_reduce_rows(g, z, scale, shift, mean, invstd, act, slope, chunks, third=True):
    """norm_bwd_reduce (fp32, third=True) / norm_bwd_reduce_bf16 (third=False): rows [N*chunks][3][C], magnitude
    rows, and the per-row slope scalars (each row's third sums added over the channels)."""
    C = z.shape[-1]
    gy, gz, t3, _ = _bwd_terms(g, z, scale, shift, mean, invstd, act, slope, third)
    rows = chunk_rows(torch.cat([gy, gz, t3], -1), chunks).reshape(-1, 3, C)
    mag = chunk_rows(torch.cat([gy.abs(), gz.abs(), t3.abs()], -1), chunks).reshape(-1, 3, C)
    return rows, mag, rows[:, 2].sum(-1)


def reduce_partials(old, beta, partials, rows, row_stride, c):
    """out[c] = beta old[c] + sum_r partials[r * row_stride + c]."""
    p = partials[:rows * row_stride].reshape(rows, row_stride)[:, :c]
    return beta * old + p.sum(0), abs(beta) * old.abs() + p.abs().sum(0)


# ------------------------------------------------------------------ finalize
def norm_finalize(s, ss, cnt, gamma, beta, eps, momentum, rm, rv):
    """From per-channel sums (fp64): mean, biased var, invstd, scale, shift and the running statistics (momentum,
    UNBIASED variance; rm / rv None = not tracked)."""
    m = s / cnt
    var = torch.clamp(ss / cnt - m * m, min=0.0)
    istd = 1.0 / torch.sqrt(var + eps)
    sc = gamma * istd
    out = {"mean": m, "var": var, "invstd": istd, "scale": sc, "shift": beta - m * sc}
    if rm is not None:
        unb = var * cnt / (cnt - 1) if cnt > 1 else var
        out["running_mean"] = (1 - momentum) * rm + momentum * m
        out["running_var"] = (1 - momentum) * rv + momentum * unb
    return out


def finalize_yardstick(mean32, istd32, gamma, beta, var, cnt, momentum, rm, rv):
    """scale / shift / running statistics by the fp64 formula on the kernel's OWN fp32 mean and invstd (fp32
    parameters as the kernel reads them), with each one's magnitude (the base of its ulp bound)."""
    mom = float(np.float32(momentum))
    sc = gamma * istd32
    out = {"scale": (sc, sc.abs()), "shift": (beta - mean32 * sc, beta.abs() + (mean32 * sc).abs())}
    if rm is not None:
        unb = var * cnt / (cnt - 1) if cnt > 1 else var
        out["running_mean"] = ((1 - mom) * rm + mom * mean32, (1 - mom) * rm.abs() + mom * mean32.abs())
        out["running_var"] = ((1 - mom) * rv + mom * unb, (1 - mom) * rv.abs() + mom * unb.abs())
    return out


def var_bound(s_mag, ss, cnt, m, L):
    """Error of var = E[z^2] - E[z]^2 when sum z and sum z^2 each carry (L + 1) 2^-24 of their magnitude sums:
    (L + 1) 2^-24 (E[z^2] + 2 |E[z]| E|z|) (+ the m^2 rounding, below 2^-24 E[z^2])."""
    ez2 = ss / cnt
    return (L + 1) * U * (ez2 + 2 * m.abs() * s_mag / cnt) + U * ez2


def finalize_bounds(ref, s_mag, ss_mag, cnt, eps, gamma, beta, L, momentum=0.1):
    """Tier R: how far each finalize output may sit from `ref` (norm_finalize on the exact sums)."""
    dm = (L + 1) * U * s_mag / cnt
    dv = var_bound(s_mag, ss_mag, cnt, ref["mean"], L)
    ve = ref["var"] + eps
    r_istd = 0.5 * dv / ve * (1 + dv / ve)           # relative error of invstd from dv (first order + margin)
    b = {"mean": dm + U * ref["mean"].abs(),
         "invstd": (r_istd + 2 * U) * ref["invstd"]}
    b["scale"] = (r_istd + 3 * U) * ref["scale"].abs()
    b["shift"] = (b["scale"] * ref["mean"].abs() + gamma.abs() * ref["invstd"] * dm
                  + 3 * U * (beta.abs() + (ref["mean"] * ref["scale"]).abs()))
    if "running_mean" in ref:
        b["running_mean"] = momentum * dm + 3 * U * ref["running_mean"].abs() + 2 * U * momentum * ref["mean"].abs()
        b["running_var"] = momentum * dv * cnt / max(cnt - 1, 1) + 4 * U * (ref["running_var"].abs() + ve)
    return b


def ulp(x):
    """fp32 ulp of |x| (fp64 tensor in, fp64 out)."""
    a = x.abs().double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def within_ulps(got, want, mag, k):
    """|got - want| <= k ulp(mag): (ok, worst ratio)."""
    err = (got.double() - want).abs()
    if not bool(torch.isfinite(got.double()).all()):
        return False, math.inf
    r = float((err / (k * ulp(mag))).max().item())
    return r <= 1.0, r


def within(got, want, bound):
    err = (got.double() - want).abs()
    if not bool(torch.isfinite(got.double()).all()):
        return False, math.inf
    r = float((err / bound.clamp_min(1e-300)).max().item())
    return r <= 1.0, r


# ------------------------------------------------------------------ norm backward finalize / apply
def norm_bwd_finalize(sums, cnt, old_dgamma, old_dbeta, old_dslope, slope_scalars):
    """c1 = sum gy / M, c2 = sum gy*zhat / M; dgamma += sum gy*zhat, dbeta += sum gy, dslope += sum of the per-row
    slope scalars.  sums: (3, C)."""
    out = {"c1": sums[0] / cnt, "c2": sums[1] / cnt}
    if old_dgamma is not None:
        out["dgamma"] = old_dgamma + sums[1]
    if old_dbeta is not None:
        out["dbeta"] = old_dbeta + sums[0]
    if old_dslope is not None:
        out["dslope"] = old_dslope + slope_scalars.sum()
    return out


def norm_bwd_apply(g, z, scale, shift, mean, invstd, c1, c2, act, slope):
    """dz = scale (gy - c1 - zhat c2), and its magnitude |scale| (|gy| + |c1| + |zhat c2|)."""
    gy, _, _, zh = _bwd_terms(g, z, scale, shift, mean, invstd, act, slope, third=False)
    return scale * (gy - c1 - zh * c2), scale.abs() * (gy.abs() + c1.abs() + (zh * c2).abs())


def bias_partials_bf16(dz_bf16, blocks, R):
    """norm_bwd_apply_bf16's bias partial rows: block b sums the rows whose (row // R) % blocks == b (dz as stored)."""
    rows, C = dz_bf16.shape
    span = blocks * R
    J = -(-rows // span)
    t = torch.cat([dz_bf16, dz_bf16.new_zeros(J * span - rows, C)]) if J * span != rows else dz_bf16
    t = t.reshape(J, blocks, R, C)
    return t.sum((0, 2)), t.abs().sum((0, 2))


# ------------------------------------------------------------------ elementwise
def act(y, act_, slope):
    return torch.where(y < 0, y * slope, y) if act_ == ACT_LEAKY else y


def norm_act_add(z, sz, hz, act_z, slope_z, r=None, sr=None, hr=None, act_r=ACT_NONE, slope_r=1.0, tanh=False):
    """out = act(z sz + hz) [+ act(r sr + hr) or + r] [tanh]; sz None = no prologue on that side.  Returns (pre-tanh
    value, magnitude)."""
    if sz is not None:
        o, mag = act(z * sz + hz, act_z, slope_z), (z.abs() * sz.abs() + hz.abs()) * max(abs(slope_z), 1.0)
    else:
        o, mag = z, z.abs()
    if r is not None:
        if sr is not None:
            o = o + act(r * sr + hr, act_r, slope_r)
            mag = mag + (r.abs() * sr.abs() + hr.abs()) * max(abs(slope_r), 1.0)
        else:
            o, mag = o + r, mag + r.abs()
    return o, mag


def norm_act_bf16(z, scale, shift, slope):
    return act(z * scale + shift, ACT_LEAKY, slope)


def linear1_forward(a, w):
    """logit[n] = sum_k a[n, k] w[k] (a: (N, F) activated, w: (F,) in a's order); with the magnitude sums."""
    return a @ w, a.abs() @ w.abs()


def linear1_backward(a, w, dlogit, old_dw, old_db, beta, P, C):
    """g_a = dlogit w; dW (torch order, channel-major) = beta old + sum_n dlogit a; dbias = beta old + sum dlogit."""
    N = a.shape[0]
    g_a = dlogit[:, None] * w[None, :]
    contrib = (dlogit[:, None] * a).sum(0)
    mag = (dlogit.abs()[:, None] * a.abs()).sum(0)
    perm = lambda v: v.reshape(P, C).t().reshape(-1)           # channels-last order -> torch flatten order
    dw = beta * old_dw + perm(contrib)
    dw_mag = abs(beta) * old_dw.abs() + perm(mag)
    db = beta * old_db + dlogit.sum()
    return g_a, dw, dw_mag, db, abs(beta) * old_db.abs() + dlogit.abs().sum(), N


def sigmoid_backward(dprob, prob):
    return dprob * (1 - prob) * prob


def tanh_backward(g, y):
    return g * (1 - y * y)


def pack_weights_bf16(w, layout, transposed=False):
    """w: torch layout (Cout, Cin, T) or (Cin, Cout, T) when transposed -> flat bf16 (RNE) in layout 0 [co][t][ci] or
    1 [ci][t][co]."""
    if transposed:
        w = w.permute(1, 0, 2)
    t = w.permute(0, 2, 1) if layout == 0 else w.permute(1, 2, 0)
    return t.contiguous().reshape(-1).float().to(torch.bfloat16)


def epi_vectors(gamma, beta, rm, rv, bias, alpha, c_norm, c_total, eps):
    """mpgan_epi_vectors_multi for one table row (fp32 in, fp64 out): channels < c_norm: scale = gamma / sqrt(rv + eps),
    shift = beta + (bias - rm) scale, slope = alpha (1 without one); channels >= c_norm: (1, bias, 1)."""
    f = lambda v, d: (v.double() if v is not None else torch.full((c_total,), d, dtype=torch.float64))
    g, b, bi = f(gamma, 1.0), f(beta, 0.0), f(bias, 0.0)
    a = float(alpha) if alpha is not None else 1.0
    sc = torch.ones(c_total, dtype=torch.float64)
    sh = bi.clone()
    sl = torch.ones(c_total, dtype=torch.float64)
    if c_norm:
        v = rv.double()[:c_norm] + float(np.float32(eps))
        sc[:c_norm] = g[:c_norm] / torch.sqrt(v)
        sh[:c_norm] = b[:c_norm] + (bi[:c_norm] - rm.double()[:c_norm]) * sc[:c_norm]
        sl[:c_norm] = a
    return sc, sh, sl


# ------------------------------------------------------------------ losses and Adam (outside the plans)
def l1_loss(a, b, grad_scale=1.0):
    d = a - b
    return d.abs().mean(), torch.sign(d) * grad_scale / d.numel()


def bce_forward(p, t):
    lp = torch.clamp(torch.log(p), min=-100.0)
    lq = torch.clamp(torch.log(1 - p), min=-100.0)
    return -(t * lp + (1 - t) * lq).mean()


def bce_backward(p, t, gout):
    return gout * (p - t) / torch.clamp((1 - p) * p, min=1e-12) / p.numel()


def adam_step(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0):
    """torch.optim.Adam (no weight decay, no amsgrad) on fp64 copies: returns (p, m, v)."""
    g = g * grad_scale
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p - (lr / bc1) * m / (torch.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


# ------------------------------------------------------------------ fp32 emulation of the kernels' summation order
def _f32_chain(x, axis):
    """Sequential fp32 sum along `axis` (numpy, exact fp32 rounding after every addition)."""
    x = np.moveaxis(np.asarray(x, dtype=np.float32), axis, 0)
    acc = np.zeros(x.shape[1:], dtype=np.float32)
    for i in range(x.shape[0]):
        acc = (acc + x[i]).astype(np.float32)
    return acc


def emulate_channel_stats(z, vec=True, chunks=None):
    """channel_stats_kernel's exact fp32 order for one sample: z (P, C) float32 -> rows (chunks, 2, C) float32.
    Thread (r, q) walks pixels beg + r, beg + r + R, ...; fold_rows then adds the R slots as the kernel does."""
    z = np.asarray(z, dtype=np.float32)
    P, C = z.shape
    V = 4 if vec else 1
    R = 256 // (C // V)
    ch = chunks or stats_chunks(P, C)
    per = chunk_per(P, ch)
    W = 2 * C
    G = 256 // W
    out = np.zeros((ch, 2, C), dtype=np.float32)
    for k in range(ch):
        beg, end = k * per, min(P, (k + 1) * per)
        seg = z[beg:end]
        n = -(-max(end - beg, 0) // R) * R
        pad = np.zeros((n, C), dtype=np.float32)
        pad[:end - beg] = seg
        pad = pad.reshape(-1, R, C)                       # [trip][slot][C]
        s = _f32_chain(pad, 0)                            # per slot, in pixel order
        q = _f32_chain(pad * pad, 0)
        slots = np.stack([s, q], 1).reshape(R, W)         # red[R][2][C]
        if G >= 2 and R >= 2 * G:
            grp = np.stack([_f32_chain(slots[gq::G], 0) for gq in range(G)])
            tot = _f32_chain(grp, 0)
        else:
            tot = _f32_chain(slots, 0)
        out[k] = tot.reshape(2, C)
    return out


def emulate_compact(rows_flat):
    """partials_compact_kernel: rows (rows, W) float32 -> (32, W): lane (g, w) adds rows g*4 + w + 128 j in order,
    then the four wave sums are added left to right."""
    rows_flat = np.asarray(rows_flat, dtype=np.float32)
    nr, W = rows_flat.shape
    out = np.zeros((COMPACT_ROWS, W), dtype=np.float32)
    for g in range(COMPACT_ROWS):
        ws = [_f32_chain(rows_flat[g * 4 + w::COMPACT_ROWS * 4], 0) if g * 4 + w < nr else np.zeros(W, np.float32)
              for w in range(4)]
        out[g] = (((ws[0] + ws[1]).astype(np.float32) + ws[2]).astype(np.float32) + ws[3]).astype(np.float32)
    return out


def emulate_finalize(rows, cnt, gamma, beta, eps):
    """The finalize's fp64 combine of fp32 rows (rows, 2, C) and its fp32 outputs."""
    r = torch.from_numpy(np.asarray(rows, dtype=np.float32)).double()
    s, ss = r[:, 0].sum(0), r[:, 1].sum(0)
    m = s / cnt
    var = torch.clamp(ss / cnt - m * m, min=0.0)
    istd = (1.0 / torch.sqrt(var + float(np.float32(eps)))).float()
    sc = (gamma.float() * istd)
    return {"mean": m.float(), "invstd": istd, "scale": sc, "shift": beta.float() - m.float() * sc}


def finalize_check(got, s, s_mag, ss, cnt, eps, gamma, beta, L, exact=False, rm=None, rv=None, momentum=0.1):
    """Every output of one finalize launch against the fp64 reference.  got: dict of fp32 tensors (mean, invstd, scale,
    shift[, running_mean, running_var]); s / s_mag / ss: exact fp64 sum z, sum |z|, sum z^2 per channel; L: the chain of
    the rows' sums (0 when exact).  Returns {output: (ok, ratio)}.
    exact: invstd within 1 ulp of the fp64 formula on the exact sums; mean within 1/2 ulp; scale / shift / running
    statistics within 2 ulp of the yardstick on the kernel's own mean / invstd.  Otherwise the tier-R bounds."""
    eps32 = float(np.float32(eps))
    ref = norm_finalize(s, ss, cnt, gamma, beta, eps32, momentum, rm, rv)
    res = {}
    if exact:
        res["mean"] = within_ulps(got["mean"], ref["mean"], ref["mean"], 0.51)
        res["invstd"] = within_ulps(got["invstd"], ref["invstd"], ref["invstd"], 1)
        ys = finalize_yardstick(got["mean"].double(), got["invstd"].double(), gamma, beta, ref["var"], cnt, momentum,
                                rm, rv)
        for k, (want, mag) in ys.items():
            if k in got:
                res[k] = within_ulps(got[k], want, mag, 2)
        return res
    b = finalize_bounds(ref, s_mag, ss, cnt, eps32, gamma, beta, L, momentum)
    for k in ("mean", "invstd", "scale", "shift", "running_mean", "running_var"):
        if k in got and k in b:
            res[k] = within(got[k], ref[k], b[k])
    return res
