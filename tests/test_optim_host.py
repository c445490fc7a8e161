"""The optimiser extras on the host: the fp64 restatements against torch's own clip_grad_norm_ ->
Adam.step -> lerp_, the EMA warm-up schedule, and the bindings of the three new entry points.  No GPU."""
import ctypes

import pytest
import torch

import optim_ref as R

LR, B1, B2, EPS = 5e-4, 0.5, 0.999, 1e-8
W = 0.1


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("case", ["below", "above", "zero"])
def test_reference_matches_torch_clip_adam_lerp(case):
    gen = torch.Generator().manual_seed(3)
    n, max_norm = 257, 1.0
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    amp = {"below": 0.01, "above": 5.0, "zero": 0.0}[case]
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([param], lr=LR, betas=(B1, B2), eps=EPS)
    ema_t = p0.clone()
    p, m, v, e = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), p0.clone()
    for step in range(1, 6):
        g = amp * torch.randn(n, generator=gen, dtype=torch.float64)
        param.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([param], max_norm)
        opt.step()
        with torch.no_grad():
            ema_t.lerp_(param.detach(), W)
        norm = R.grad_norm(g)
        coef = R.clip_coef(norm, max_norm)
        assert (coef < 1.0) == (case == "above")
        assert abs(norm - float(total)) <= 1e-12 * max(float(total), 1e-300)
        p, m, v = R.adam_step_coef(p, g, m, v, LR, B1, B2, EPS, step, coef=coef)
        e = R.lerp(e, p, W)
        assert _rel(p, param.detach()) <= 1e-12, (case, step)
        assert _rel(e, ema_t) <= 1e-12, (case, step)
        if case != "zero":
            assert _rel(g * coef, param.grad) <= 1e-12


def test_reference_norm_rounds_the_scaled_gradient_to_fp32_first():
    g = torch.tensor([1.0, 3.0, 1e-3], dtype=torch.float32)
    s = 1.0 / 3.0
    want = float(((g * torch.tensor(s, dtype=torch.float32)).double() ** 2).sum().sqrt())
    assert R.grad_norm(g, s) == want
    assert R.clip_coef(2.0, None) == 1.0 and R.clip_coef(2.0, 0.0) == 1.0
    assert float(R.clip_coef_f32(0.0, 1.0)) == 1.0


def test_reference_buffer_update():
    src = [torch.tensor([1.0, 2.0]), torch.tensor(7)]
    dst = [torch.tensor([3.0, 2.0]), torch.tensor(2)]
    out = R.ema_buffers(src, dst, 0.25)
    assert torch.equal(out[0], torch.tensor([2.5, 2.0], dtype=torch.float64)) and int(out[1]) == 7


def test_ema_decay_at():
    from mpgan_amd.gan import ema_decay_at
    assert ema_decay_at(1, 0.999, True) == pytest.approx(0.1, abs=1e-15)
    vals = [ema_decay_at(s, 0.999, True) for s in range(1, 20000)]
    assert all(b >= a for a, b in zip(vals, vals[1:]))
    for decay in (0.9, 0.99, 0.999):
        for step in range(1, 12000):
            t = step - 1
            ramp = (1.0 + t) / (10.0 + t)
            got = ema_decay_at(step, decay, True)
            assert got == (decay if ramp >= decay else ramp)
            assert got == R.ema_decay_at(step, decay, True)
        # (1 + t) / (10 + t) >= d  <=>  t >= (10 d - 1) / (1 - d)
        first = next(s for s in range(1, 12000) if ema_decay_at(s, decay, True) == decay)
        assert abs((first - 1) - (10 * decay - 1) / (1 - decay)) <= 1.0 + 1e-6
    assert {ema_decay_at(s, 0.97, False) for s in (1, 2, 10, 10 ** 6)} == {0.97}


def test_new_symbols_are_bound_with_the_declared_argument_counts():
    from mpgan_amd import _lib
    want = {"mpgan_grad_norm_workspace": (ctypes.c_int64, 1), "mpgan_grad_norm": (ctypes.c_int32, 8),
            "mpgan_adam_step_ex": (ctypes.c_int32, 15), "mpgan_ema_buffers": (ctypes.c_int32, 5)}
    for name, (res, nargs) in want.items():
        assert name in _lib.SIGNATURES, name
        got_res, args = _lib.SIGNATURES[name]
        assert got_res is res and len(args) == nargs, (name, got_res, len(args))
    # mpgan_adam_step's arguments up to grad_scale, then coef, ema, ema_weight, stream
    ex = _lib.SIGNATURES["mpgan_adam_step_ex"][1]
    assert ex[:11] == _lib.SIGNATURES["mpgan_adam_step"][1][:11]
    assert ex[11:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]


def test_gan_option_validation_needs_no_gpu():
    from mpgan_amd.gan import GAN
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(grad_clip=-1.0)):
        with pytest.raises(ValueError):
            GAN(1, 32, 32, dimensions=2, n_unet_blocks=1, device="cpu", **bad)
