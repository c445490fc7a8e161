"""The optimiser extras' kernels (optim_ops.hip) at small, odd sizes: mpgan_adam_step_ex against
mpgan_adam_step bit for bit, the gradient norm and its clip coefficient against fp64, the clipped step and the weight
EMA against their fp64 restatements (tests/optim_ref.py), the buffer EMA with guard words, and the argument checks."""
import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

# 4096 * 256 + 259 exceeds one pass of a 4096-block grid of the element-wise form and of the norm's 1024 x 1024 sweep
SIZES = [1, 3, 4, 255, 256, 257, 1027, 4096 * 256 + 259]
# ... and this one a pass of the 16-byte form (4096 blocks x 256 lanes x 4 floats); used where no CPU sweep is needed
BIG_VEC = 4096 * 1024 + 1027
LR, B1, B2, EPS = 5e-4, 0.5, 0.999, 1e-8
GS = 1.0 / 3.0                      # a grad_scale that is no power of two: g * grad_scale rounds


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _dev(t, misaligned=False):
    """t on the GPU: a fresh (16-byte aligned) allocation, or a view one float into one."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()] if misaligned else buf[:t.numel()]
    v.copy_(t)
    return v


def _cases(operands):
    """(numel, misaligned operand or None): every size aligned, and at 1027 each operand in turn off by one float."""
    return [(n, None) for n in SIZES] + [(1027, name) for name in operands]


def _state(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = 0.01 * torch.randn(n, generator=gen)
    v = 1e-4 * torch.rand(n, generator=gen)
    return gen, p, m, v


def _norm(g, grad_scale, max_norm):
    from mpgan_amd import ops
    out2 = torch.full((2,), -7.0, device="cuda")
    ws = torch.empty(ops.grad_norm_workspace(g.numel()) // 8, dtype=torch.float64, device="cuda")
    ops.grad_norm(g, out2, ws, grad_scale, max_norm)
    return out2


# ---------------------------------------------------------------------------------------------------------------------
# exactness against mpgan_adam_step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "coef-one", "zero-grad"])
@pytest.mark.parametrize("n,mis", _cases("pgmv") + [(BIG_VEC, None)])
def test_adam_step_ex_equals_adam_step_bit_for_bit(n, mis, variant):
    from mpgan_amd import ops
    gen, p0, m0, v0 = _state(n, 11)
    ref = [_dev(t) for t in (p0, m0, v0)]
    got = [_dev(t, mis == name) for t, name in zip((p0, m0, v0), "pmv")]
    for step in range(1, 4):
        g_cpu = torch.zeros(n) if variant == "zero-grad" else 0.3 * torch.randn(n, generator=gen)
        g_ref, g = _dev(g_cpu), _dev(g_cpu, mis == "g")
        coef = None
        if variant != "plain":
            # a bound far above the norm (or a zero gradient): min(1, max_norm / (norm + 1e-6)) is exactly 1.0f
            out2 = _norm(g, GS, 1e30 if variant == "coef-one" else 1.0)
            coef = out2[1:2]
            assert float(coef) == 1.0
        ops.adam_step(ref[0], g_ref, ref[1], ref[2], LR, B1, B2, EPS, step, GS)
        ops.adam_step_ex(got[0], g, got[1], got[2], LR, B1, B2, EPS, step, GS, coef=coef)
        for name, a, b in zip("pmv", got, ref):
            assert torch.equal(_bits(a), _bits(b)), (name, step, int((_bits(a) != _bits(b)).sum()))
    assert not torch.equal(_bits(got[0]), _bits(_dev(p0)))       # the step did move the parameters


# ---------------------------------------------------------------------------------------------------------------------
# the norm
# ---------------------------------------------------------------------------------------------------------------------
def _check_norm(g_cpu, grad_scale, max_norm, mis=False):
    ref = R.grad_norm(g_cpu, grad_scale)
    ref32 = np.float32(ref)
    assert np.isfinite(ref32) and (ref32 == 0 or abs(ref32) >= np.finfo(np.float32).tiny)   # checked on the CPU first
    g = _dev(g_cpu, mis)
    out2 = _norm(g, grad_scale, max_norm).cpu().numpy()
    print(f"n={g_cpu.numel()} norm {out2[0]!r} ref {ref!r} coef {out2[1]!r}")
    assert abs(float(out2[0]) - float(ref32)) <= R.ulp32(ref32), (out2[0], ref)
    want_coef = R.clip_coef_f32(out2[0], max_norm)
    assert abs(float(out2[1]) - float(want_coef)) <= R.ulp32(want_coef), (out2[1], want_coef)
    again = _norm(g, grad_scale, max_norm).cpu()
    assert torch.equal(_bits(again), _bits(torch.from_numpy(out2)))           # two runs: the same bits
    return out2


@pytest.mark.parametrize("n,mis", _cases("g"))
def test_grad_norm_and_coefficient(n, mis):
    gen = torch.Generator().manual_seed(5 + n)
    g = 0.2 * torch.randn(n, generator=gen)
    ref = R.grad_norm(g, GS)
    clipped = _check_norm(g, GS, 0.1 * ref, mis is not None)
    assert 0.09 < clipped[1] < 0.11
    free = _check_norm(g, GS, 0.0, mis is not None)
    assert free[1] == 1.0 and free[0] == clipped[0]
    assert _check_norm(g, GS, 10.0 * ref + 1.0, mis is not None)[1] == 1.0


def test_grad_norm_where_fp32_squares_overflow_or_underflow():
    gen = torch.Generator().manual_seed(9)
    big = torch.randn(1027, generator=gen)
    big[torch.arange(8) * 128 + 3] = 3e19              # 9e38 > FLT_MAX: an fp32 sum of squares is inf
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float32(3e19) * np.float32(3e19))
    out = _check_norm(big, 1.0, 1.0)
    assert abs(out[0] / (3e19 * np.sqrt(8.0)) - 1) < 1e-6
    tiny = torch.full((1024,), 1e-30)                  # squares 1e-60 are 0 in fp32; the norm 3.2e-29 is an fp32 normal
    assert float(np.float32(1e-30) * np.float32(1e-30)) == 0.0
    out = _check_norm(tiny, 1.0, 1.0)
    assert abs(out[0] / 3.2e-29 - 1) < 1e-6 and out[1] == 1.0


def test_zero_gradient_norm_is_zero_and_never_clips():
    out = _check_norm(torch.zeros(257), GS, 1.0)
    assert out[0] == 0.0 and out[1] == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the clipped step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mis", _cases("pgmv"))
def test_clipped_adam_matches_fp64(n, mis):
    from mpgan_amd import ops
    gen, p0, m0, v0 = _state(n, 17)
    p, m, v = (_dev(t, mis == name) for t, name in zip((p0, m0, v0), "pmv"))
    p64, m64, v64 = p0.double(), m0.double(), v0.double()
    for step in range(1, 6):
        g_cpu = 0.3 * torch.randn(n, generator=gen)
        g = _dev(g_cpu, mis == "g")
        max_norm = 0.1 * float(_norm(g, GS, 0.0)[0])              # a tenth of this gradient's measured norm
        out2 = _norm(g, GS, max_norm)
        ops.adam_step_ex(p, g, m, v, LR, B1, B2, EPS, step, GS, coef=out2[1:2])
        norm64 = R.grad_norm(g_cpu, GS)
        coef64 = R.clip_coef(norm64, max_norm)
        assert 0.05 < coef64 < 0.2
        g64 = (g_cpu * torch.tensor(GS, dtype=torch.float32)).double()     # the fp32 product the kernels load
        p64, m64, v64 = R.adam_step_coef(p64, g64, m64, v64, LR, B1, B2, EPS, step, coef=coef64)
    err = (p.cpu().double() - p64).abs()
    print(f"n={n} mis={mis} max |err| {float(err.max()):.3e}")
    assert bool((err <= 1e-7 + 1e-6 * p64.abs()).all()), float(err.max())
    assert float((p.cpu().double() - p0.double()).abs().max()) > 1e-4           # five steps of about lr each


# ---------------------------------------------------------------------------------------------------------------------
# the weight EMA inside the step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.001, 0.1, 0.9])
@pytest.mark.parametrize("n,mis", _cases(["p", "g", "m", "v", "ema"]) + [(BIG_VEC, None)])
def test_ema_of_the_new_parameters(n, mis, w):
    from mpgan_amd import ops
    gen, p0, m0, v0 = _state(n, 23)
    e0 = torch.randn(n, generator=gen)
    e0[::7] = 1e-42                                                # denormal averages: the bound's floor
    g_cpu = 0.3 * torch.randn(n, generator=gen)
    p, m, v, e, g = (_dev(t, mis == name) for t, name in zip((p0, m0, v0, e0, g_cpu), ("p", "m", "v", "ema", "g")))
    p_plain, m_plain, v_plain = _dev(p0), _dev(m0), _dev(v0)
    ops.adam_step(p_plain, _dev(g_cpu), m_plain, v_plain, LR, B1, B2, EPS, 1, GS)
    ops.adam_step_ex(p, g, m, v, LR, B1, B2, EPS, 1, GS, ema=e, ema_weight=w)
    assert torch.equal(_bits(p), _bits(p_plain)) and torch.equal(_bits(m), _bits(m_plain))     # the EMA changes no step
    p_new = p.cpu()
    want = R.lerp(e0.double(), p_new.double(), float(np.float32(w)))
    err = (e.cpu().double() - want).abs()
    bound = R.ema_bound(e0, p_new)
    print(f"n={n} w={w} max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize("n,mis", [(257, None), (1027, "ema"), (1027, None)])
def test_ema_over_eight_chained_steps(n, mis):
    from mpgan_amd import ops
    w = 0.1
    gen, p0, m0, v0 = _state(n, 29)
    e0 = torch.randn(n, generator=gen)
    p, m, v, e = _dev(p0), _dev(m0), _dev(v0), _dev(e0, mis == "ema")
    e64, scale = e0.double(), e0.abs()
    coef = torch.ones(1, device="cuda")
    for step in range(1, 9):
        g = _dev(0.3 * torch.randn(n, generator=gen))
        ops.adam_step_ex(p, g, m, v, LR, B1, B2, EPS, step, GS, coef=coef, ema=e, ema_weight=w)
        p_new = p.cpu()
        e64 = R.lerp(e64, p_new.double(), float(np.float32(w)))
        scale = torch.maximum(scale, torch.maximum(p_new.abs(), e64.abs().float()))
    err = (e.cpu().double() - e64).abs()
    bound = R.ema_bound(scale, scale, steps=8)
    print(f"n={n} max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())


# ---------------------------------------------------------------------------------------------------------------------
# the buffer EMA
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.001, 0.1, 0.9])
def test_ema_buffers_table(w):
    from mpgan_amd import ops
    numels, guard = [1, 16, 17, 128], 3
    gen = torch.Generator().manual_seed(41)
    total = sum(numels) + guard * (len(numels) + 1)
    src_cpu, dst_cpu = torch.randn(total, generator=gen), torch.randn(total, generator=gen)
    src, dst = src_cpu.cuda(), dst_cpu.cuda()
    isrc = torch.tensor([-1, 12345678901, -1], dtype=torch.int64, device="cuda")
    idst = torch.tensor([-2, 7, -2], dtype=torch.int64, device="cuda")
    rows, spans, off = [], [], guard
    for n in numels:
        rows.append([src.data_ptr() + 4 * off, dst.data_ptr() + 4 * off, n, 0])
        spans.append((off, off + n))
        off += n + guard
    rows.append([isrc.data_ptr() + 8, idst.data_ptr() + 8, 1, 1])
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    ops.ema_buffers(table, len(rows), max(numels), w)
    got = dst.cpu()
    inside = torch.zeros(total, dtype=torch.bool)
    for a, b in spans:
        inside[a:b] = True
        want = R.lerp(dst_cpu[a:b].double(), src_cpu[a:b].double(), float(np.float32(w)))
        err = (got[a:b].double() - want).abs()
        assert bool((err <= R.ema_bound(dst_cpu[a:b], src_cpu[a:b])).all()), (a, b, float(err.max()))
        assert not torch.equal(got[a:b], dst_cpu[a:b])
    assert torch.equal(_bits(got[~inside]), _bits(dst_cpu[~inside]))           # guard words untouched
    assert torch.equal(src.cpu(), src_cpu)
    assert idst.tolist() == [-2, 12345678901, -2] and isrc.tolist() == [-1, 12345678901, -1]


def test_ema_buffers_without_entries_returns_zero():
    from mpgan_amd import _lib, ops
    assert _lib.lib().mpgan_ema_buffers(None, 0, 0, 0.1, None) == 0
    ops.ema_buffers(None, 0, 0, 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (on the host, before any launch)
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_name_their_function():
    from mpgan_amd import _lib
    lib = _lib.lib()
    buf = torch.zeros(64, device="cuda")
    ws = torch.zeros(8, dtype=torch.float64, device="cuda")
    before = buf.clone()
    P, W = buf.data_ptr(), ws.data_ptr()

    def refused(rc, name):
        assert rc == -1 and name in lib.mpgan_last_error(), (rc, lib.mpgan_last_error())

    assert lib.mpgan_grad_norm_workspace(1) == 8 and lib.mpgan_grad_norm_workspace(5000) == 40
    refused(lib.mpgan_grad_norm_workspace(0), b"mpgan_grad_norm_workspace")
    refused(lib.mpgan_grad_norm(None, 16, 1.0, 1.0, W, 64, P, None), b"mpgan_grad_norm")
    refused(lib.mpgan_grad_norm(P, 16, 1.0, 1.0, None, 64, P, None), b"mpgan_grad_norm")
    refused(lib.mpgan_grad_norm(P, 16, 1.0, 1.0, W, 64, None, None), b"mpgan_grad_norm")
    refused(lib.mpgan_grad_norm(P, 0, 1.0, 1.0, W, 64, P, None), b"mpgan_grad_norm")
    refused(lib.mpgan_grad_norm(P, 5000, 1.0, 1.0, W, 39, P + 64, None), b"mpgan_grad_norm")     # needs 5 doubles
    adam = (16, 1e-3, 0.5, 0.999, 1e-8, 1, 1.0, None, None, 0.0, None)
    for k in range(4):
        ptrs = [P, P + 64, P + 128, P + 192]
        ptrs[k] = None
        refused(lib.mpgan_adam_step_ex(*ptrs, *adam), b"mpgan_adam_step_ex")
    refused(lib.mpgan_adam_step_ex(P, P + 64, P + 128, P + 192, 0, *adam[1:]), b"mpgan_adam_step_ex")
    refused(lib.mpgan_adam_step_ex(P, P + 64, P + 128, P + 192, 16, 1e-3, 0.5, 0.999, 1e-8, 0, 1.0, None, None, 0.0, None),
            b"mpgan_adam_step_ex")
    refused(lib.mpgan_ema_buffers(None, 1, 16, 0.1, None), b"mpgan_ema_buffers")
    refused(lib.mpgan_ema_buffers(W, -1, 16, 0.1, None), b"mpgan_ema_buffers")
    refused(lib.mpgan_ema_buffers(W, 1, 0, 0.1, None), b"mpgan_ema_buffers")
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                           # nothing was launched


def test_wrappers_check_sizes_and_devices():
    from mpgan_amd import ops
    p, g, m, v = (torch.zeros(8, device="cuda") for _ in range(4))
    with pytest.raises(ValueError):
        ops.adam_step_ex(p, g[:7], m, v, LR, B1, B2, EPS, 1)
    with pytest.raises(ValueError):
        ops.adam_step_ex(p, g, m, v, LR, B1, B2, EPS, 1, ema=torch.zeros(9, device="cuda"))
    with pytest.raises(ValueError):
        ops.adam_step_ex(p, g, m, v.cpu(), LR, B1, B2, EPS, 1)
    with pytest.raises(ValueError):
        ops.adam_step_ex(p, g, m, v, LR, B1, B2, EPS, 1, coef=torch.ones(2, device="cuda"))
    with pytest.raises(ValueError):
        ops.grad_norm(g, torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.grad_norm(torch.zeros(5000, device="cuda"), torch.zeros(2, device="cuda"),
                      torch.zeros(2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.grad_norm(g[::2], torch.zeros(2, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.ema_buffers(torch.zeros(4, dtype=torch.int64), 1, 4, 0.1)
