"""CPU checks of tests/norm_ref.py: its restatements agree with torch fp64 autograd, an emulation of the kernels' own fp32
summation order passes its tier-R bounds (so they are not too tight), and planted faults fail a tier (so they are not
too loose)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as N

D = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _all_ok(res):
    return all(ok for ok, _ in res.values())


# ------------------------------------------------------------------ restatements vs torch autograd
@pytest.mark.parametrize("slope", [0.2, 0.25])
def test_norm_forward_backward_match_autograd(slope):
    g_ = _gen(1)
    n, c, P = 3, 8, 50
    z = (torch.rand(n, c, P, generator=g_, dtype=D) * 3 - 1).requires_grad_(True)
    gamma = (torch.rand(c, generator=g_, dtype=D) + 0.5).requires_grad_(True)
    beta = (torch.rand(c, generator=g_, dtype=D) - 0.5).requires_grad_(True)
    alpha = torch.tensor([slope], dtype=D, requires_grad=True)
    rm, rv = torch.rand(c, generator=g_, dtype=D), torch.rand(c, generator=g_, dtype=D) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    y = F.batch_norm(z, rm, rv, gamma, beta, True, 0.1, 1e-5)
    a = F.prelu(y, alpha)
    go = torch.rand(a.shape, generator=g_, dtype=D) * 2 - 1
    a.backward(go)

    zc = z.detach().permute(0, 2, 1)                        # (N, P, C)
    rows, _ = N.channel_stats_rows(zc, N.stats_chunks(P, c))
    s, ss = rows.sum(0)
    fin = N.norm_finalize(s, ss, n * P, gamma.detach(), beta.detach(), 1e-5, 0.1, rm0, rv0)
    assert torch.allclose(fin["running_mean"], rm, rtol=1e-12, atol=1e-14)
    assert torch.allclose(fin["running_var"], rv, rtol=1e-12, atol=1e-14)
    out, _ = N.norm_act_add(zc, fin["scale"], fin["shift"], N.ACT_LEAKY, slope)
    assert torch.allclose(out, a.detach().permute(0, 2, 1), rtol=1e-12, atol=1e-12)

    g = go.permute(0, 2, 1)
    chunks = N.stats_chunks(P, c)
    brow, _, sc_rows = N.norm_bwd_reduce_rows(g, zc, fin["scale"], fin["shift"], fin["mean"], fin["invstd"],
                                              N.ACT_LEAKY, slope, chunks)
    zeros = torch.zeros(c, dtype=D)
    fb = N.norm_bwd_finalize(brow.sum(0), n * P, zeros, zeros, torch.zeros(1, dtype=D), sc_rows)
    dz, _ = N.norm_bwd_apply(g, zc, fin["scale"], fin["shift"], fin["mean"], fin["invstd"], fb["c1"], fb["c2"],
                             N.ACT_LEAKY, slope)
    assert torch.allclose(dz, z.grad.permute(0, 2, 1), rtol=1e-10, atol=1e-12)
    assert torch.allclose(fb["dgamma"], gamma.grad, rtol=1e-10, atol=1e-12)
    assert torch.allclose(fb["dbeta"], beta.grad, rtol=1e-10, atol=1e-12)
    # PReLU's slope gradient: sum over pixels of g * y where y < 0
    assert torch.allclose(fb["dslope"], alpha.grad, rtol=1e-10, atol=1e-12)


def test_head_and_losses_match_autograd():
    g_ = _gen(2)
    n, P, c = 4, 6, 8
    a = torch.rand(n, P * c, generator=g_, dtype=D) * 2 - 1
    w = (torch.rand(P * c, generator=g_, dtype=D) - 0.5).requires_grad_(True)   # channels-last order
    b = torch.tensor([0.1], dtype=D, requires_grad=True)
    ar = a.clone().requires_grad_(True)
    logit = ar @ w + b
    prob = torch.sigmoid(logit)
    t = torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=D)
    loss = F.binary_cross_entropy(prob, t)
    loss.backward()
    mine_logit, _ = N.linear1_forward(a, w.detach())
    assert torch.allclose(mine_logit + 0.1, logit.detach(), rtol=1e-13)
    p = prob.detach()
    assert torch.allclose(N.bce_forward(p, t), loss.detach(), rtol=1e-13)
    dprob = N.bce_backward(p, t, 1.0)
    dlogit = N.sigmoid_backward(dprob, p)
    old_w, old_b = torch.zeros(P * c, dtype=D), torch.zeros(1, dtype=D)
    g_a, dw, _, db, _, _ = N.linear1_backward(a, w.detach(), dlogit, old_w, old_b, 1.0, P, c)
    assert torch.allclose(g_a, ar.grad, rtol=1e-10)
    perm = lambda v: v.reshape(P, c).t().reshape(-1)       # the torch (C-major) order the kernel writes
    assert torch.allclose(dw, perm(w.grad), rtol=1e-10)
    assert torch.allclose(db, b.grad, rtol=1e-10)
    # the -100 clamp of the log
    p1 = torch.tensor([0.0, 1.0], dtype=D)
    assert torch.allclose(N.bce_forward(p1, torch.tensor([1.0, 1.0], dtype=D)),
                          F.binary_cross_entropy(p1, torch.tensor([1.0, 1.0], dtype=D)))
    # L1
    x = torch.rand(50, generator=g_, dtype=D).requires_grad_(True)
    y = torch.rand(50, generator=g_, dtype=D)
    l = F.l1_loss(x, y)
    l.backward()
    v, gr = N.l1_loss(x.detach(), y)
    assert torch.allclose(v, l.detach()) and torch.allclose(gr, x.grad)
    # tanh backward
    u = torch.rand(20, generator=g_, dtype=D).requires_grad_(True)
    th = torch.tanh(u)
    go = torch.rand(20, generator=g_, dtype=D)
    th.backward(go)
    assert torch.allclose(N.tanh_backward(go, th.detach()), u.grad)


@pytest.mark.parametrize("steps", [1, 3])
def test_adam_matches_torch(steps):
    g_ = _gen(3)
    p0 = torch.rand(40, generator=g_, dtype=D)
    grads = [torch.rand(40, generator=g_, dtype=D) - 0.5 for _ in range(steps)]
    tp = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=2e-4, betas=(0.5, 0.999), eps=1e-8)
    p, m, v = p0.clone(), torch.zeros(40, dtype=D), torch.zeros(40, dtype=D)
    for k, g in enumerate(grads):
        tp.grad = g.clone()
        opt.step()
        p, m, v = N.adam_step(p, g, m, v, 2e-4, 0.5, 0.999, 1e-8, k + 1)
    assert torch.allclose(p, tp.detach(), rtol=1e-13, atol=1e-15)


def test_pack_and_epi_vectors():
    w = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4) + 1 / 3
    p0 = N.pack_weights_bf16(w, 0)
    assert p0.dtype == torch.bfloat16 and p0.float()[4 * 3 + 1].item() == w[1, 1, 0].to(torch.bfloat16).item()
    p1 = N.pack_weights_bf16(w, 1)
    assert p1.float()[(1 * 4 + 2) * 2 + 1].item() == w[1, 1, 2].to(torch.bfloat16).item()
    c = 6
    gamma, beta, rm, rv, bias = (torch.rand(c, generator=_gen(k)) for k in range(5))
    sc, sh, sl = N.epi_vectors(gamma, beta, rm, rv, bias, 0.3, 4, c, 1e-5)
    assert torch.allclose(sc[:4], gamma[:4].double() / torch.sqrt(rv[:4].double() + float(np.float32(1e-5))))
    assert sc[4:].eq(1).all() and sl[4:].eq(1).all() and torch.equal(sh[4:], bias[4:].double())
    assert torch.allclose(sl[:4], torch.full((4,), 0.3, dtype=D))


# ------------------------------------------------------------------ the kernels' fp32 order passes the bounds
def _offset_tensor(P, C, ratio, seed):
    """Channel-dependent offsets: |mean| / std = ratio, plus a near-constant channel (3.7 +- 0.001) and a constant
    non-dyadic one (0.1) in the last two channels."""
    g_ = _gen(seed)
    std = torch.rand(C, generator=g_, dtype=D) + 0.5
    mean = ratio * std * torch.where(torch.rand(C, generator=g_) < 0.5, -1.0, 1.0).double()
    z = mean + std * torch.randn(P, C, generator=g_, dtype=D)
    z[:, -2] = 3.7 + 0.001 * torch.randn(P, generator=g_, dtype=D)
    z[:, -1] = 0.1
    return z.float()


@pytest.mark.parametrize("ratio", [0.0, 1.0, 10.0, 100.0])
@pytest.mark.parametrize("C,vec", [(16, True), (16, False), (8, True), (128, True)])
def test_emulated_stats_pass_tier_r(ratio, C, vec):
    """channel_stats_kernel's fp32 order (rows) and the finalize's fp64 combine (wide form: >= 256 rows) pass
    every row bound and every finalize bound."""
    n, P = 2, 40000 if C <= 16 else 8000
    z = torch.stack([_offset_tensor(P, C, ratio, 10 + i) for i in range(n)])
    chunks = N.stats_chunks(P, C)
    L = N.chain_length("reduce", P=P, C=C, vec=vec)
    rows = np.concatenate([N.emulate_channel_stats(z[i].numpy(), vec) for i in range(n)])
    want, mag = N.channel_stats_rows(z.double(), chunks)
    ok, ratio_rows = N.check_sums(torch.from_numpy(rows).double(), want, mag, L + 1)
    assert ok, ratio_rows
    gamma, beta = torch.rand(C, generator=_gen(5), dtype=D) + 0.5, torch.rand(C, generator=_gen(6), dtype=D) - 0.5
    got = N.emulate_finalize(rows, n * P, gamma, beta, 1e-5)
    s, ss = want.sum(0)
    res = N.finalize_check(got, s, mag.sum(0)[0], ss, n * P, 1e-5, gamma.float().double(), beta.float().double(), L)
    assert _all_ok(res), res


@pytest.mark.parametrize("ratio", [1.0, 100.0])
def test_emulated_compact_fold_passes_tier_r(ratio):
    """The compact path: 18432 rows (> 16384) of fp32 tile sums, folded in partials_compact_kernel's order."""
    C, tile, nrows = 8, 16, 18432
    z = _offset_tensor(nrows * tile, C, ratio, 7).reshape(nrows, tile, C)
    rows32 = torch.stack([z.sum(1), (z * z).sum(1)], 1)                 # fp32 tile sums: self-consistent rows
    compact = N.emulate_compact(rows32.reshape(nrows, 2 * C).numpy())
    L = tile + N.chain_length("finalize", n=1, chunks=nrows)
    z64 = z.double().reshape(-1, C)
    s, ss, s_mag = z64.sum(0), (z64 * z64).sum(0), z64.abs().sum(0)
    gamma, beta = torch.ones(C, dtype=D), torch.zeros(C, dtype=D)
    got = N.emulate_finalize(compact.reshape(32, 2, C), nrows * tile, gamma, beta, 1e-5)
    res = N.finalize_check(got, s, s_mag, ss, nrows * tile, 1e-5, gamma, beta, L)
    assert _all_ok(res), res


def test_chain_lengths_follow_the_code():
    # C = 16, V = 4: R = 64, per = ceil(P / chunks); fold_rows with W = 32: G = 8 groups of 8 slots
    P = 128 ** 3
    ch = N.stats_chunks(P, 16)
    assert ch == 256 and N.chain_length("reduce", P=P, C=16) == -(-(-(-P // 256)) // 64) + 8 + 8
    # V = 1: R = 16 slots, G = 8 groups of 2
    assert N.chain_length("reduce", P=P, C=16, vec=False) == -(-(-(-P // 256)) // 16) + 2 + 8
    assert N.finalize_form(1, 16385)[0] == "compact" and N.finalize_form(1, 16384)[0] == "wide"
    assert N.finalize_form(1, 255)[0] == "narrow"
    assert N.chain_length("finalize", n=1, chunks=32768) == 256 + 3


# ------------------------------------------------------------------ planted faults fail a tier
def _stats_case(P=3000, C=8, ratio=10.0):
    z = _offset_tensor(P, C, ratio, 21).unsqueeze(0)
    chunks = N.stats_chunks(P, C)
    rows = torch.from_numpy(N.emulate_channel_stats(z[0].numpy(), True)).double()
    want, mag = N.channel_stats_rows(z.double(), chunks)
    return z, rows, want, mag, N.chain_length("reduce", P=P, C=C)


def test_fault_dropped_or_shifted_row_fails():
    z, rows, want, mag, L = _stats_case()
    assert N.check_sums(rows, want, mag, L + 1)[0]
    dropped = rows.clone()
    dropped[3] = 0
    assert not N.check_sums(dropped, want, mag, L + 1)[0]
    assert not N.check_sums(rows.roll(1, 0), want, mag, L + 1)[0]


def _fin_inputs(C=8, cnt=1000, ratio=1.0):
    z = _offset_tensor(cnt, C, ratio, 33).double()
    return z, z.sum(0), z.abs().sum(0), (z * z).sum(0)


def test_fault_cstride_ignored_fails():
    C, cnt = 8, 1000
    z, s, s_mag, ss = _fin_inputs(C, cnt)
    other = z + 50.0                                                    # the residual half: other values
    rows_w = torch.cat([torch.stack([z.sum(0), (z * z).sum(0)]), torch.stack([other.sum(0), (other * other).sum(0)])],
                       1).float()                                       # one row [2][cstride = 2C]
    flat = rows_w.reshape(-1)
    gamma, beta = torch.ones(C, dtype=D), torch.zeros(C, dtype=D)
    good = N.emulate_finalize(flat.reshape(2, 2 * C)[:, :C].reshape(1, 2, C), cnt, gamma, beta, 1e-5)
    bad = N.emulate_finalize(flat[:2 * C].reshape(1, 2, C), cnt, gamma, beta, 1e-5)   # rows read as [2][C]
    assert _all_ok(N.finalize_check(good, s, s_mag, ss, cnt, 1e-5, gamma, beta, 2))
    assert not _all_ok(N.finalize_check(bad, s, s_mag, ss, cnt, 1e-5, gamma, beta, 2))


def test_fault_biased_running_variance_fails():
    C, cnt = 8, 1000
    z, s, s_mag, ss = _fin_inputs(C, cnt)
    gamma, beta = torch.ones(C, dtype=D), torch.zeros(C, dtype=D)
    rm, rv = torch.zeros(C, dtype=D), torch.ones(C, dtype=D)
    ref = N.norm_finalize(s, ss, cnt, gamma, beta, float(np.float32(1e-5)), 0.1, rm, rv)
    got = {k: ref[k].float() for k in ("mean", "invstd", "scale", "shift", "running_mean", "running_var")}
    assert _all_ok(N.finalize_check(got, s, s_mag, ss, cnt, 1e-5, gamma, beta, 0, rm=rm, rv=rv))
    got["running_var"] = (0.9 * rv + 0.1 * ref["var"]).float()           # biased
    assert not _all_ok(N.finalize_check(got, s, s_mag, ss, cnt, 1e-5, gamma, beta, 0, rm=rm, rv=rv))


def test_fault_c1_c2_swapped_fails():
    g_ = _gen(8)
    sums = torch.rand(3, 8, generator=g_, dtype=D)
    mag = sums.abs() * 3
    fb = N.norm_bwd_finalize(sums, 500, None, None, None, None)
    assert N.check_sums(fb["c1"].float(), fb["c1"], mag[0] / 500, 0)[0]
    assert not N.check_sums(fb["c2"].float(), fb["c1"], mag[0] / 500, 0)[0]


def test_fault_pitch_off_by_one_fails():
    g_ = _gen(9)
    rows, c, ld = 64, 8, 12
    buf = torch.randint(-3, 4, (rows * ld + 8,), generator=g_).double()
    z = buf[:rows * ld].reshape(rows, ld)[:, :c]
    bad = buf[:rows * (ld - 1)].reshape(rows, ld - 1)[:, :c]
    sc, sh = torch.full((c,), 4.0, dtype=D), torch.full((c,), 0.5, dtype=D)
    want, _ = N.norm_act_add(z, sc, sh, N.ACT_LEAKY, 0.25)
    got, _ = N.norm_act_add(bad, sc, sh, N.ACT_LEAKY, 0.25)
    assert not torch.equal(got, want)


def test_fault_truncation_instead_of_rne_fails():
    from conv_ref import bf16_trunc
    v = torch.tensor([1.0 + 3 * 2 ** -9, -(2.0 + 2 ** -6 + 2 ** -8)], dtype=D)   # dyadic, not bf16-representable
    assert not torch.equal(bf16_trunc(v), N.bf16_rne(v))


def test_fault_beta_accumulation_dropped_fails():
    g_ = _gen(10)
    part = torch.randint(-3, 4, (40 * 16,), generator=g_).double()
    old = torch.randint(1, 4, (16,), generator=g_).double()
    want, mag = N.reduce_partials(old, 1.0, part, 40, 16, 16)
    dropped, _ = N.reduce_partials(old, 0.0, part, 40, 16, 16)
    assert N.check_sums(want, want, mag, 0, exact=True)[0]
    assert not N.check_sums(dropped, want, mag, 0, exact=True)[0]


def test_fault_compact_skips_last_group_fails():
    C, tile, nrows = 8, 16, 16400
    z = _offset_tensor(nrows * tile, C, 1.0, 44).reshape(nrows, tile, C)
    rows32 = torch.stack([z.sum(1), (z * z).sum(1)], 1).reshape(nrows, 2 * C).numpy()
    compact = N.emulate_compact(rows32)
    compact[-1] = 0                                                   # the last row group never written
    z64 = z.double().reshape(-1, C)
    gamma, beta = torch.ones(C, dtype=D), torch.zeros(C, dtype=D)
    got = N.emulate_finalize(compact.reshape(32, 2, C), nrows * tile, gamma, beta, 1e-5)
    L = tile + N.chain_length("finalize", n=1, chunks=nrows)
    res = N.finalize_check(got, z64.sum(0), z64.abs().sum(0), (z64 * z64).sum(0), nrows * tile, 1e-5, gamma, beta, L)
    assert not _all_ok(res)
    assert math.isfinite(max(r for _, r in res.values()))
