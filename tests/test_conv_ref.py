"""CPU self-test of tests/conv_ref.py, the fp64 convolution reference of the full-size launch tests
(tests/test_step_launches_gpu.py), and the proof that its two check tiers catch real faults.

  * Every operation (forward, transposed forward, backward-data, weight and bias gradient, the prologue, the
    conv-epilogue BatchNorm + PReLU, the fused statistics and norm-backward sums) against torch.nn.functional +
    autograd in float64, at every (k, stride, pad, transposed, output_pad) the generator (MONAI 0.4.0 U-Net,
    oracle/refmodel.py) and the discriminator use, in 2-D and 3-D.
  * Discrimination: an honest result -- torch's fp32 CPU convolution, rounded to bf16 (nearest even) for a bf16
    output -- passes tier X and tier R; each planted fault fails at least one of them."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

# (k, stride, pad, transposed, output_pad): U-Net down conv / strided residual, unit conv, 1x1 residual, up conv;
# the discriminator's valid k3 s1 and k4 s2 convs
GEOMS = [(3, 2, 1, False, 0), (3, 1, 1, False, 0), (1, 1, 0, False, 0), (3, 2, 1, True, 1), (3, 1, 0, False, 0),
         (4, 2, 0, False, 0)]


def _cl(t, dims):
    """NC(D)HW -> channels-last (N, D, H, W, C)."""
    if dims == 2:
        t = t.unsqueeze(2)
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _nc(t, dims):
    y = t.permute(0, 4, 1, 2, 3)
    return y[:, :, 0] if dims == 2 else y


def _w3(w, dims):
    return w.unsqueeze(2) if dims == 2 else w


def _g3(v, dims, fill):
    return (fill,) * (3 - dims) + (v,) * dims


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("k,s,p,tr,op", GEOMS, ids=lambda v: str(v))
def test_reference_matches_torch_in_float64(dims, k, s, p, tr, op):
    gen = torch.Generator().manual_seed(7 + k * 10 + s + 100 * tr)
    n, cin, cout = 2, 3, 5
    sp = (7, 9) if dims == 2 else (5, 6, 7)
    x = (torch.rand(n, cin, *sp, generator=gen, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    wshape = (cin, cout) if tr else (cout, cin)
    w = (torch.rand(*wshape, *([k] * dims), generator=gen, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    b = (torch.rand(cout, generator=gen, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    if tr:
        f = F.conv_transpose2d if dims == 2 else F.conv_transpose3d
        y = f(x, w, b, stride=s, padding=p, output_padding=op)
    else:
        y = (F.conv2d if dims == 2 else F.conv3d)(x, w, b, stride=s, padding=p)
    dy = torch.rand(y.shape, generator=gen, dtype=torch.float64) * 2 - 1
    y.backward(dy)
    k3, s3, p3 = _g3(k, dims, 1), _g3(s, dims, 1), _g3(p, dims, 0)
    in3 = (1,) * (3 - dims) + sp
    out3 = R.out_extent(in3, k3, s3, p3, tr, _g3(op, dims, 0))
    assert out3 == tuple(y.shape[2:]) if dims == 3 else out3 == (1,) + tuple(y.shape[2:])
    xc, dyc, w3 = _cl(x.detach(), dims), _cl(dy, dims), _w3(w.detach(), dims)
    got_y = R.conv_forward(xc, w3, k3, s3, p3, out3, tr) + b.detach()
    got_dx = R.conv_backward_data(dyc, w3, k3, s3, p3, in3, tr)
    got_dw = R.conv_backward_weight(xc, dyc, k3, s3, p3, tr)
    torch.testing.assert_close(_nc(got_y, dims), y.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(_nc(got_dx, dims), x.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got_dw, _w3(w.grad, dims), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.bias_grad(dyc), b.grad, rtol=1e-12, atol=1e-12)
    # the magnitude pass bounds every output and is itself the same routine on |operands|
    absref = R.conv_forward(xc.abs(), w3.abs(), k3, s3, p3, out3, tr)
    assert (got_y - b.detach() <= absref + 1e-12).all() and (absref >= 0).all()


def test_fused_extras_match_torch_in_float64():
    gen = torch.Generator().manual_seed(3)
    c, dt = 6, torch.float64
    z = torch.rand(2, 3, 4, 5, c, generator=gen, dtype=dt) * 2 - 1
    scale, shift = torch.rand(c, generator=gen, dtype=dt) + 0.5, torch.rand(c, generator=gen, dtype=dt) - 0.5
    a = R.prologue(z, scale, shift, 0, R.ACT_LEAKY, 0.2)
    torch.testing.assert_close(a, F.leaky_relu(z * scale + shift, 0.2))
    sn, tn = torch.rand(2, c, generator=gen, dtype=dt), torch.rand(2, c, generator=gen, dtype=dt)
    a2 = R.prologue(z, sn, tn, c, R.ACT_NONE)
    torch.testing.assert_close(a2, z * sn[:, None, None, None, :] + tn[:, None, None, None, :])
    assert (R.prologue(z, scale, shift, 0, R.ACT_LEAKY, 0.2, absolute=True) >= a.abs()).all()
    slope = torch.rand(c, generator=gen, dtype=dt)
    e = R.act_epilogue(z, scale, shift, slope)
    want = F.prelu(_nc(z * scale + shift, 3), slope)
    torch.testing.assert_close(_nc(e, 3), want)
    sums, mag = R.stats_sums(z)
    torch.testing.assert_close(sums[0], z.sum((0, 1, 2, 3)))
    torch.testing.assert_close(sums[1], (z * z).sum((0, 1, 2, 3)))
    # norm-backward sums: sum gy = dL/dbeta and sum gy*zhat = dL/dgamma of BatchNorm (batch statistics held fixed)
    # followed by LeakyReLU; the third, sum g*min(y, 0), is dL/dslope
    mean, invstd = torch.rand(c, generator=gen, dtype=dt) - 0.5, torch.rand(c, generator=gen, dtype=dt) + 0.5
    gamma = (torch.rand(c, generator=gen, dtype=dt) + 0.5).requires_grad_(True)
    beta = (torch.rand(c, generator=gen, dtype=dt) - 0.5).requires_grad_(True)
    sl = torch.tensor(0.2, dtype=dt, requires_grad=True)
    y = (z - mean) * invstd * gamma + beta
    out = torch.where(y < 0, y * sl, y)
    g = torch.rand(z.shape, generator=gen, dtype=dt) * 2 - 1
    out.backward(g)
    s3, _ = R.norm_bwd_sums(g, z, (gamma * invstd).detach(), (beta - mean * gamma * invstd).detach(), mean, invstd, 0.2)
    torch.testing.assert_close(s3[0], beta.grad)
    torch.testing.assert_close(s3[1], gamma.grad)
    torch.testing.assert_close(s3[2].sum(), sl.grad)


def test_rounding_helpers():
    v = torch.tensor([1.0, 257.0, 259.0, -259.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -9], dtype=torch.float64)
    torch.testing.assert_close(R.bf16_rne(v), torch.tensor([1.0, 256.0, 260.0, -260.0, 1.0, 1 + 2.0 ** -7], dtype=torch.float64))
    torch.testing.assert_close(R.bf16_trunc(v), torch.tensor([1.0, 256.0, 258.0, -258.0, 1.0, 1.0], dtype=torch.float64))
    old = torch.backends.cuda.matmul.allow_tf32
    with R.no_tf32():
        assert torch.backends.cuda.matmul.allow_tf32 is False
    assert torch.backends.cuda.matmul.allow_tf32 == old


# ------------------------------------------------------------------ discrimination of the two tiers
N, CI, CO, SP = 2, 8, 6, (11, 13)          # W = 13: a ragged last tile along W for any tile width 4 .. 12
K3, S3, P3 = (1, 3, 3), (1, 1, 1), (0, 1, 1)
OUT3 = (1,) + SP


def _operands(tier, seed):
    gen = torch.Generator().manual_seed(seed)
    dt = torch.float64
    if tier == "X":   # integers wide enough that many outputs carry more than bf16's 8 significant bits
        x = torch.randint(-60, 61, (N, CI, *SP), generator=gen).to(dt) * (torch.rand(N, CI, *SP, generator=gen) < 0.5)
        w = torch.randint(-7, 8, (CO, CI, 3, 3), generator=gen).to(dt)
        dy = torch.randint(-7, 8, (N, CO, *SP), generator=gen).to(dt) * (torch.rand(N, CO, *SP, generator=gen) < 0.5)
    else:
        x = torch.rand(N, CI, *SP, generator=gen, dtype=dt) * 2 - 1
        w = (torch.rand(CO, CI, 3, 3, generator=gen, dtype=dt) * 2 - 1) / math.sqrt(CI * 9)
        dy = torch.rand(N, CO, *SP, generator=gen, dtype=dt) * 2 - 1
    return x, w, dy


def _torch_fwd(x, w):
    return F.conv2d(x.float(), w.float(), padding=1)


def _torch_wgrad(x, w, dy):
    wr = w.float().requires_grad_(True)
    F.conv2d(x.float(), wr, padding=1).backward(dy.float())
    return wr.grad


def _tiers(op, seed, fault=None):
    """(tier X passes, tier R passes) of the torch fp32 result, with `fault` planted in it."""
    res = []
    for tier in ("X", "R"):
        x, w, dy = _operands(tier, seed)
        bf16_out = fault == "truncate-not-rne" or op == "fwd-bf16"
        if op == "wgrad":
            got = _torch_wgrad(x, w, dy.clone().index_fill_(0, torch.tensor([1]), 0) if fault == "wgrad-missing-sample" else dy)
            got = got.unsqueeze(2)
            args = (_cl(x, 2), _cl(dy, 2), K3, S3, P3)
            ref, absref = R.conv_backward_weight(*args), R.conv_backward_weight(_cl(x, 2).abs(), _cl(dy, 2).abs(), K3, S3, P3)
            ref32 = R.conv_backward_weight(_cl(x, 2).float(), _cl(dy, 2).float(), K3, S3, P3)
            L = N * SP[0] * SP[1] + 2
        elif op == "dgrad":
            got = _cl(F.conv_transpose2d(dy.float(), w.float(), padding=1), 2)
            ref = R.conv_backward_data(_cl(dy, 2), w.unsqueeze(2), K3, S3, P3, OUT3)
            absref = R.conv_backward_data(_cl(dy, 2).abs(), w.unsqueeze(2).abs(), K3, S3, P3, OUT3)
            ref32 = R.conv_backward_data(_cl(dy, 2).float(), w.unsqueeze(2).float(), K3, S3, P3, OUT3)
            L = CO * 9 + 2
        else:
            wf = w.clone()
            if fault == "drop-tap":
                wf[2, :, 1, 2] = 0
            if fault == "swap-cin-in-tap":
                wf[:, [0, 3], 0, 1] = w[:, [3, 0], 0, 1]
            xin = x
            if fault == "bf16-operands-in-fp32":
                xin, wf = R.bf16_rne(x), R.bf16_rne(wf)
            y = _torch_fwd(xin, wf)
            r = SP[1] % 8
            if fault == "last-w-tile-shifted":
                y[..., -r:] = y[..., -r - 1:-1].clone()
            if fault == "last-w-tile-unwritten":
                y[..., -r:] = float("nan")
            if bf16_out:
                y = R.bf16_trunc(y) if fault == "truncate-not-rne" else R.bf16_rne(y)
            got = _cl(y, 2)
            ref = R.conv_forward(_cl(x, 2), w.unsqueeze(2), K3, S3, P3, OUT3)
            absref = R.conv_forward(_cl(x, 2).abs(), w.unsqueeze(2).abs(), K3, S3, P3, OUT3)
            ref32 = R.conv_forward(_cl(x, 2).float(), w.unsqueeze(2).float(), K3, S3, P3, OUT3)
            L = CI * 9 + 2
        if tier == "X":
            assert absref.max().item() < R.EXACT_LIMIT
            res.append(R.check_exact(got, ref, bf16_out)[0])
        else:
            ok, re_, rn = R.check_random(got, ref, absref, ref32, L, bf16_out)
            print(f"{op} {fault}: tier R ratios elementwise {re_:.3g} norm-wise {rn:.3g}")
            res.append(ok)
    return tuple(res)


@pytest.mark.parametrize("op", ["fwd", "fwd-bf16", "dgrad", "wgrad"])
def test_honest_results_pass_both_tiers(op):
    assert _tiers(op, 41) == (True, True)


@pytest.mark.parametrize("op,fault", [("fwd", "drop-tap"), ("fwd", "swap-cin-in-tap"), ("fwd", "last-w-tile-shifted"),
                                      ("fwd", "last-w-tile-unwritten"), ("wgrad", "wgrad-missing-sample"),
                                      ("fwd", "bf16-operands-in-fp32"), ("fwd", "truncate-not-rne")],
                         ids=lambda v: str(v))
def test_planted_fault_is_rejected(op, fault):
    x_ok, r_ok = _tiers(op, 41, fault)
    assert not (x_ok and r_ok), f"{fault} passed both tiers"


# ------------------------------------------------------------------ fused statistics rows
def _stats_tiers(fault=None):
    """(tier X passes, tier R passes) of fused BatchNorm statistics rows formed from torch's fp32 forward the way a
    kernel leaves them -- one fp32 row of (sum y, sum y^2) per 16 pixels, rows added in fp64 -- with `fault` planted."""
    res = []
    for tier in ("X", "R"):
        x, w, _ = _operands(tier, 43)
        if tier == "X":              # small integers: sum y^2 per channel stays below 2^24, so every row is exact
            x = torch.sign(x) * (x.abs() % 4)
        b = torch.zeros(CO, dtype=torch.float64) if tier == "X" else torch.rand(CO, generator=torch.Generator().manual_seed(5),
                                                                                  dtype=torch.float64) - 0.5
        y = _cl(F.conv2d(x.float(), w.float(), b.float(), padding=1), 2)
        if fault == "stats-missing-sample":
            y = y.clone()
            y[1] = 0
        f = y.reshape(-1, CO)
        part = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in f.split(16)])
        rows = part.shape[0]
        if fault == "stats-channel-swap-in-row":
            part[3] = part[3][:, [1, 0, 2, 3, 4, 5]]
        if fault == "stats-row-written-twice":
            part[6] = part[5]
        if fault == "stats-last-row-unwritten":
            part[-1] = float("nan")
        got = part.double().sum(0)
        ref = R.conv_forward(_cl(x, 2), w.unsqueeze(2), K3, S3, P3, OUT3) + b
        absref = R.conv_forward(_cl(x, 2).abs(), w.unsqueeze(2).abs(), K3, S3, P3, OUT3) + b.abs()
        M = N * SP[0] * SP[1]
        want, mag, extra = R.stats_terms(ref, absref, 0 if tier == "X" else CI * 9 + 2)
        if tier == "X":
            assert R.exact_sums_ok(mag)
        ok, ratio = R.stats_check(got, want, mag, extra, M, rows, exact=tier == "X")
        print(f"stats {fault}: tier {tier} ratio {ratio:.3g}")
        res.append(ok)
    return tuple(res)


def test_honest_statistics_rows_pass_both_tiers():
    assert _stats_tiers() == (True, True)


@pytest.mark.parametrize("fault", ["stats-missing-sample", "stats-channel-swap-in-row", "stats-row-written-twice",
                                   "stats-last-row-unwritten"])
def test_planted_statistics_fault_is_rejected(fault):
    x_ok, r_ok = _stats_tiers(fault)
    assert not (x_ok and r_ok), f"{fault} passed both tiers"
    if fault != "stats-row-written-twice":       # a misplaced row is caught by the exact tier; the rest by both
        assert not x_ok and not r_ok, (x_ok, r_ok)
