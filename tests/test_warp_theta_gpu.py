"""The affine warp's gradient in theta (csrc/pair_augment.hip: mpgan_affine_warp_backward_theta) through
ops.affine_warp_backward_theta and augment.diff_affine_warp, against the float64 restatement of tests/warp_theta_ref.py
at the smallest shapes at which it can go wrong: odd extents, W % 4 != 0, tiles along every axis, in != out sizes, D = 1,
more than 256 tiles per sample, integer coordinates (every f == 0), a NaN theta.

Bound, per entry:  |got - ref| <= 1e-12 * sum_p |gy dy/dc_k P_j|
  both sides are fp64 sums of the same terms in another order: <= 7e4 terms of a few dozen roundings each, ~1e-14
  relative; the factor leaves room for an FMA-contracted coordinate, which moves f by < 1e-14.  A wrong cell, a skipped
  zero-weight corner or a missed dead voxel is an O(1) error."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import warp_theta_ref as T

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _theta(theta, n):
    return torch.as_tensor(np.asarray(theta), dtype=torch.float64).reshape(n, 12).cuda()


def _dev(a, two_d):
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = t[:, 0] if two_d else t
    return t.unsqueeze(1).cuda()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The case's device tensors (x0, x1, gy0, gy1, theta): made once, never modified."""
    n, in_size, out_size, theta = T.CASES[name]
    two_d = in_size[0] == 1
    return tuple(_dev(a, two_d) for a in T.make_case(name)) + (_theta(theta, n),)


@functools.lru_cache(maxsize=None)
def _ref(name, plane, fill):
    """(g_theta, scale) of one plane of a case by the restatement: computed once."""
    n, in_size, out_size, theta = T.CASES[name]
    x0, x1, g0, g1 = T.make_case(name)
    return T.affine_warp_theta_grad_ref(x1 if plane else x0, g1 if plane else g0, theta, fill)


def _grad(x0, x1, g0, g1, th, fill0=0.0, fill1=0.0):
    from mpgan_amd import ops
    return ops.affine_warp_backward_theta(x0, x1, g0, g1, th, ops.WARP_CONSTANT, fill0, fill1)


def _check(got, ref, scale, what):
    got = got.cpu().numpy()
    err, bound = np.abs(got - ref), 1e-12 * scale
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |got - ref| = {err.max():.3e}, max |ref| = {np.abs(ref).max():.3f}, worst err / bound = {worst:.4f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float(err.max()), worst)


# ---- 1. every case against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", T.FILLS)
@pytest.mark.parametrize("name", list(T.CASES))
def test_cases_against_fp64(name, fill):
    x0, x1, g0, g1, th = _inputs(name)
    got = _grad(x0, None, g0, None, th, fill)
    assert got.shape == (x0.shape[0], 12) and got.dtype == torch.float64
    ref, scale = _ref(name, 0, fill)
    _check(got, ref, scale, f"{name} fill {fill}")
    assert np.abs(ref).max() > 0.1
    if name == "integer":                              # the derivative is all in the corners the forward never reads
        assert (scale[:, [3, 7, 11]] > 1.0).all()


@pytest.mark.parametrize("name", ["rot3d", "rot2d", "crop", "wide", "integer"])
def test_two_planes_are_the_sum_of_the_planes(name):
    x0, x1, g0, g1, th = _inputs(name)
    both = _grad(x0, x1, g0, g1, th, -1.0, 0.5)
    (r0, s0), (r1, s1) = _ref(name, 0, -1.0), _ref(name, 1, 0.5)
    _check(both, r0 + r1, s0 + s1, f"{name} two planes")
    one, two = _grad(x0, None, g0, None, th, -1.0), _grad(x1, None, g1, None, th, 0.5)
    assert (np.abs((both - (one + two)).cpu().numpy()) <= 1e-12 * (s0 + s1)).all()


# ---- 2. exact zeros, reproducibility, batch independence ------------------------------------------------------------------
def test_nan_theta_kills_its_sample_alone():
    x0, x1, g0, g1, th = _inputs("nan")
    got = _grad(x0, x1, g0, g1, th, -1.0, -1.0)
    assert torch.equal(_bits(got[0]), torch.zeros(12, dtype=torch.int64))           # exactly +0.0
    alone = _grad(x0[1:].contiguous(), x1[1:].contiguous(), g0[1:].contiguous(), g1[1:].contiguous(), th[1:].contiguous(),
                  -1.0, -1.0)
    assert torch.equal(_bits(got[1]), _bits(alone[0])) and float(got[1].abs().max()) > 0.1


@pytest.mark.parametrize("name", ["rot3d", "many", "tiles3d"])
def test_two_runs_and_a_dirty_workspace_give_the_same_bits(name):
    from mpgan_amd import _lib, ops
    x0, x1, g0, g1, th = _inputs(name)
    n = x0.shape[0]
    first = _grad(x0, None, g0, None, th, -1.0)
    assert torch.equal(_bits(_grad(x0, None, g0, None, th, -1.0)), _bits(first))
    need = ops.affine_warp_theta_workspace(n, tuple(g0.shape[2:]))
    tiles = {"rot3d": 4, "many": 264, "tiles3d": 3 * 3 * 2}[name]
    assert need == n * tiles * 12 * 8
    ws = torch.full((need // 8,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((n, 12), 7.0, dtype=torch.float64, device="cuda")
    i3 = lambda t: ops._dhw(tuple(t.shape[2:]))
    rc = _lib.lib().mpgan_affine_warp_backward_theta(x0.data_ptr(), None, g0.data_ptr(), None, n, i3(x0), i3(g0),
                                                     th.data_ptr(), ops.WARP_CONSTANT, -1.0, -1.0, ws.data_ptr(), need,
                                                     out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(_bits(out), _bits(first))
    assert not bool(torch.isnan(ws).any())                      # every slot of the workspace is written


@pytest.mark.parametrize("name", ["rot3d", "many"])
def test_a_sample_does_not_depend_on_its_batch(name):
    x0, x1, g0, g1, th = _inputs(name)
    n = x0.shape[0]
    first = _grad(x0, x1, g0, g1, th, -1.0, 0.0)
    for s in range(n):
        alone = _grad(*(t[s:s + 1].contiguous() for t in (x0, x1, g0, g1, th)), -1.0, 0.0)
        assert torch.equal(_bits(alone[0]), _bits(first[s])), (name, s)
    order = list(range(n))[::-1]
    other = _grad(*(t[order].contiguous() for t in (x0, x1, g0, g1, th)), -1.0, 0.0)
    assert torch.equal(_bits(other), _bits(first[order]))


# ---- 3. autograd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rot3d", "rot2d", "crop"])
def test_diff_affine_warp_gives_theta_its_gradient(name, monkeypatch):
    from mpgan_amd import augment as A
    from mpgan_amd import ops
    n, in_size, out_size, _ = T.CASES[name]
    outs = tuple(out_size[1:] if in_size[0] == 1 else out_size)
    x0, x1, g0, g1, th = _inputs(name)
    want0, want1 = _grad(x0, None, g0, None, th, -1.0), _grad(x1, None, g1, None, th, 0.5)
    want_both = _grad(x0, x1, g0, g1, th, -1.0, 0.5)
    calls = []
    real = ops.affine_warp_backward_theta
    monkeypatch.setattr(ops, "affine_warp_backward_theta", lambda *a, **k: calls.append(a) or real(*a, **k))
    # one plane, x and theta both require grad: theta.grad has the ops call's bits, x.grad the bits it has without theta
    xa, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    ta = th.clone().requires_grad_(True)
    ya = A.diff_affine_warp(xa, ta, out_size=outs, fill=-1.0)
    yb = A.diff_affine_warp(xb, th, out_size=outs, fill=-1.0)
    assert torch.equal(_bits(ya), _bits(yb))
    ya.backward(g0)
    yb.backward(g0)
    assert len(calls) == 1 and ta.grad.shape == (n, 12) and ta.grad.dtype == torch.float64
    assert torch.equal(_bits(ta.grad), _bits(want0)) and torch.equal(_bits(xa.grad), _bits(xb.grad))
    # theta alone: nothing for x
    del calls[:]
    ta = th.clone().requires_grad_(True)
    A.diff_affine_warp(x0, ta, out_size=outs, fill=-1.0).backward(g0)
    assert len(calls) == 1 and torch.equal(_bits(ta.grad), _bits(want0))
    # two planes, both used
    del calls[:]
    ta = th.clone().requires_grad_(True)
    y0, y1 = A.diff_affine_warp(x0, ta, x1, out_size=outs, fill=(-1.0, 0.5))
    ((y0 * g0).sum() + (y1 * g1).sum()).backward()
    assert len(calls) == 1 and calls[0][1] is not None and torch.equal(_bits(ta.grad), _bits(want_both))
    # the second plane has no gradient: it is not passed
    del calls[:]
    ta = th.clone().requires_grad_(True)
    y0, y1 = A.diff_affine_warp(x0, ta, x1, out_size=outs, fill=(-1.0, 0.5))
    (y0 * g0).sum().backward()
    assert len(calls) == 1 and calls[0][1] is None and calls[0][3] is None and torch.equal(_bits(ta.grad), _bits(want0))
    # the first plane has none: the second goes in as plane 0 with its own fill
    del calls[:]
    ta = th.clone().requires_grad_(True)
    y0, y1 = A.diff_affine_warp(x0, ta, x1, out_size=outs, fill=(-1.0, 0.5))
    (y1 * g1).sum().backward()
    assert len(calls) == 1 and calls[0][1] is None and calls[0][6] == 0.5 and torch.equal(_bits(ta.grad), _bits(want1))
    # a theta that requires none: no call, and only theta is kept
    del calls[:]
    xa = x0.clone().requires_grad_(True)
    y = A.diff_affine_warp(xa, th, out_size=outs, fill=-1.0)
    assert len(y.grad_fn.saved_tensors) == 1
    y.backward(g0)
    assert not calls


def test_refusals_before_any_launch():
    from mpgan_amd import _lib, ops
    x0, x1, g0, g1, th = _inputs("rot3d")
    n = x0.shape[0]
    with pytest.raises(ValueError, match="CONSTANT"):
        ops.affine_warp_backward_theta(x0, None, g0, None, th, ops.WARP_BORDER, 0.0, 0.0)
    with pytest.raises(ValueError, match="go together"):
        ops.affine_warp_backward_theta(x0, x1, g0, None, th, ops.WARP_CONSTANT, 0.0, 0.0)
    with pytest.raises(ValueError, match="theta"):
        ops.affine_warp_backward_theta(x0, None, g0, None, th[:1].contiguous(), ops.WARP_CONSTANT, 0.0, 0.0)
    with pytest.raises(ValueError, match="theta"):
        ops.affine_warp_backward_theta(x0, None, g0, None, th.float(), ops.WARP_CONSTANT, 0.0, 0.0)
    with pytest.raises(ValueError, match="gtheta"):
        ops.affine_warp_backward_theta(x0, None, g0, None, th, ops.WARP_CONSTANT, 0.0, 0.0,
                                       gtheta=torch.empty(n, 11, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="gy0"):
        ops.affine_warp_backward_theta(x0, None, g0[:1].contiguous(), None, th, ops.WARP_CONSTANT, 0.0, 0.0)
    with pytest.raises(ValueError, match="second plane"):
        ops.affine_warp_backward_theta(x0, x1[..., :-1].contiguous(), g0, g1, th, ops.WARP_CONSTANT, 0.0, 0.0)
    # the library itself: BORDER and a short workspace leave gtheta and ws untouched
    need = ops.affine_warp_theta_workspace(n, tuple(g0.shape[2:]))
    ws = torch.full((need // 8,), 5.0, dtype=torch.float64, device="cuda")
    out = torch.full((n, 12), 3.0, dtype=torch.float64, device="cuda")
    i3 = ops._dhw(tuple(x0.shape[2:]))
    lib = _lib.lib()
    for mode, nbytes, word in ((ops.WARP_BORDER, need, b"border"), (ops.WARP_CONSTANT, need - 8, b"workspace")):
        assert lib.mpgan_affine_warp_backward_theta(x0.data_ptr(), None, g0.data_ptr(), None, n, i3, i3, th.data_ptr(), mode,
                                                    0.0, 0.0, ws.data_ptr(), nbytes, out.data_ptr(), None) == -1
        assert word in lib.mpgan_last_error()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((ws == 5.0).all())
