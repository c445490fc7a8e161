"""The affine warp's backward (csrc/pair_augment.hip: mpgan_affine_warp_backward) through ops.affine_warp_backward,
augment.diff_affine_warp and the DiffAugment policy word "affine", against the float64 restatement of
tests/warp_backward_ref.py at the smallest shapes at which it can go wrong: odd extents, W % 4 != 0, more than one
4 x 8 x 32 tile per sample, in != out sizes (a reach of 3.44 voxels one way, most voxels without a contributor the
other way), D = 1.

Bound, on every voxel:  |got - ref| <= 2^-24 |ref| + 5e-10
  2^-24 |ref|   the one fp32 rounding of an fp64 sum
  5e-10         ten times (2 * 3.44 + 1)^3 ~ 490 terms x 3 axes x 2.8e-14 (4 fp64 roundings of a coordinate of magnitude
                <= 2^6, which a tent weight of slope 1 passes on; |g_y| < 1) = 4.2e-11
Integer-valued maps (identity, flips, a quarter turn, an integer shift) are compared bit for bit with torch index ops."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import affine_ref as R
import warp_backward_ref as B

pytestmark = pytest.mark.gpu

EYE = np.eye(3, 4).reshape(12)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _theta(theta, n):
    return torch.as_tensor(np.asarray(theta), dtype=torch.float64).reshape(n, 12).cuda()


def _dev(a, two_d=False):
    """(n, D, H, W) numpy -> the (n, 1, D, H, W) (or (n, 1, H, W)) device tensor."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    t = t[:, 0] if two_d else t
    return t.unsqueeze(1).cuda()


def _backward(gy, theta, in_size):
    """ops.affine_warp_backward on a device g_y (n, 1, *out) -> g_x (n, 1, *in_size)."""
    from mpgan_amd import ops
    gx = torch.full((gy.shape[0], 1, *in_size), 7.0, dtype=torch.float32, device="cuda")      # overwritten everywhere
    return ops.affine_warp_backward(gy, _theta(theta, gy.shape[0]), ops.WARP_CONSTANT, gx)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(g_y fp32 numpy, the fp64 reference g_x): computed once, never modified."""
    n, in_size, out_size, theta = B.CASES[name]
    gy = B.make_grad(n, out_size)
    return gy, B.affine_warp_backward_ref(gy, theta, in_size)


def _check(got, ref, what):
    got = got.detach().cpu().double().numpy().reshape(ref.shape)
    err = np.abs(got - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 5e-10
    worst = float((err / bound).max())
    print(f"{what}: max |got - ref| = {err.max():.3e}, worst err / bound = {worst:.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float(err.max()), worst)


def _run_case(name):
    n, in_size, out_size, theta = B.CASES[name]
    two_d = in_size[0] == 1
    gy = _dev(_case(name)[0], two_d)
    return _backward(gy, theta, in_size[1:] if two_d else in_size)


# ---- 1. against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.CASES))
def test_cases_against_fp64(name):
    n, in_size, out_size, theta = B.CASES[name]
    gx = _run_case(name)
    assert gx.shape == (n, 1, *(in_size[1:] if in_size[0] == 1 else in_size))
    ref = _case(name)[1]
    _check(gx, ref, name)
    if name in ("mini", "crop", "wide"):                       # voxels without any contributor are exact zeros
        assert (ref == 0).sum() > ref.size // 8
        assert torch.equal(gx.cpu().reshape(ref.shape) == 0, torch.from_numpy(ref == 0))


# ---- 2. the adjoint identity on the device --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.CASES))
def test_adjoint_identity_on_the_device(name):
    """<W x, g> against <x, W^T g>, W x by affine_warp (constant, fill 0) and W^T g by the backward kernel, both products
    summed in fp64 on the host.  Each side carries one fp32 rounding per output element, so the two differ by at most
    2^-24 (sum |W x| |g| + sum |x| |W^T g|).  For positive data nothing cancels, that scale IS the product, and the
    relative gap |lhs - rhs| / max(|lhs|, |rhs|) is at most 2^-23 = 1.2e-7 < 1e-6.  The signed pair of the other tests
    is held to the same 1e-6 of the scale that bounds it, the sums of absolute terms."""
    from mpgan_amd import augment as A
    n, in_size, out_size, theta = B.CASES[name]
    two_d = in_size[0] == 1
    ins, outs = (in_size[1:], out_size[1:]) if two_d else (in_size, out_size)
    th = _theta(theta, n)
    for label, shift in (("positive", 1.5), ("signed", 0.0)):
        x, g = _dev(R.make_input(n, in_size, seed=5) + shift, two_d), _dev(R.make_input(n, out_size, seed=6) + shift, two_d)
        y = A.affine_warp(x, th, out_size=outs, mode="constant", fill=0.0)
        gx = _backward(g, theta, ins)
        lhs_terms, rhs_terms = (y.double() * g.double()).cpu(), (x.double() * gx.double()).cpu()
        lhs, rhs = float(lhs_terms.sum()), float(rhs_terms.sum())
        scale = max(abs(lhs), abs(rhs)) if shift else float(lhs_terms.abs().sum() + rhs_terms.abs().sum())
        print(f"{name} {label}: <Wx, g> = {lhs:.9e}, <x, W^T g> = {rhs:.9e}, gap / scale = {abs(lhs - rhs) / scale:.3e}")
        assert scale > 0 and abs(lhs - rhs) <= 1e-6 * scale, (name, label, lhs, rhs)


# ---- 3. integer-valued thetas: permuted copies ------------------------------------------------------------------------
def _shifted(gy, t):
    """g_x[q] = g_y[q - t] where q - t lies inside, else 0 (the adjoint of y[p] = x[p + t]), by slices."""
    gx = torch.zeros_like(gy)
    dst, src = [slice(None)] * 2, [slice(None)] * 2
    for k, tk in enumerate(t):
        S = gy.shape[2 + k]
        dst.append(slice(max(tk, 0), S + min(tk, 0)))
        src.append(slice(max(-tk, 0), S - max(tk, 0)))
    gx[tuple(dst)] = gy[tuple(src)]
    return gx


INTEGER_3D = {       # name -> (in size, out size, theta, the same map on g_y by torch index ops)
    "identity": ((3, 4, 5), (3, 4, 5), EYE, lambda g: g.clone()),
    "flip-d-w": ((3, 4, 5), (3, 4, 5), [-1, 0, 0, 2, 0, 1, 0, 0, 0, 0, -1, 4], lambda g: g.flip(2, 4)),
    "flip-h": ((3, 4, 5), (3, 4, 5), [1, 0, 0, 0, 0, -1, 0, 3, 0, 0, 1, 0], lambda g: g.flip(3)),
    # y[d, h', w'] = x[d, w', 4 - h']: out (3, 5, 4); y = x.transpose(3, 4).flip(3), so g_x = g_y.flip(3).transpose(3, 4)
    "quarter-turn": ((3, 4, 5), (3, 5, 4), [1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 4], lambda g: g.flip(3).transpose(3, 4)),
    "shift": ((3, 4, 5), (3, 4, 5), [1, 0, 0, 1, 0, 1, 0, -2, 0, 0, 1, 3], lambda g: _shifted(g, (1, -2, 3))),
    "shift-out": ((3, 4, 5), (3, 4, 5), [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 5], lambda g: torch.zeros_like(g)),
    "wide-flip": ((2, 9, 67), (2, 9, 67), [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 66], lambda g: g.flip(4)),      # 3 tiles along w
}
INTEGER_2D = {
    "identity": ((13, 10), (13, 10), EYE, lambda g: g.clone()),
    "flip-h-w": ((13, 10), (13, 10), [1, 0, 0, 0, 0, -1, 0, 12, 0, 0, -1, 9], lambda g: g.flip(2, 3)),
    "quarter-turn": ((13, 10), (10, 13), [1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 9], lambda g: g.flip(2).transpose(2, 3)),
    "shift": ((13, 10), (13, 10), [1, 0, 0, 0, 0, 1, 0, 4, 0, 0, 1, -3], lambda g: _shifted(g, (4, -3))),
}


@pytest.mark.parametrize("name,table", [(k, "3d") for k in INTEGER_3D] + [(k, "2d") for k in INTEGER_2D])
def test_integer_thetas_copy_bits(name, table):
    from mpgan_amd import augment as A
    in_size, out_size, theta, index_op = (INTEGER_3D if table == "3d" else INTEGER_2D)[name]
    n = 2
    gy = _dev(B.make_grad(n, out_size, seed=2), two_d=table == "2d")
    gx = _backward(gy, np.stack([np.asarray(theta, dtype=np.float64)] * n), in_size)
    want = index_op(gy)
    assert want.shape == gx.shape and torch.equal(_bits(gx), _bits(want.contiguous()))
    # and the forward under the same theta is the transposed index op: the pair is a permutation and its inverse
    x = _dev(R.make_input(n, in_size, seed=3), two_d=table == "2d")
    y = A.affine_warp(x, _theta(np.stack([np.asarray(theta, dtype=np.float64)] * n), n), out_size=out_size,
                      mode="constant", fill=0.0)
    lhs, rhs = (y.double() * gy.double()).sum(), (x.double() * want.double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * max(1.0, abs(float(lhs)))


# ---- 4. reproducibility ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rot3d", "rot2d", "wide"])
def test_two_runs_and_other_samples_leave_the_bits_alone(name):
    n, in_size, out_size, theta = B.CASES[name]
    two_d = in_size[0] == 1
    ins = in_size[1:] if two_d else in_size
    gy = _dev(_case(name)[0], two_d)
    first = _run_case(name)
    assert torch.equal(_bits(_run_case(name)), _bits(first))
    for s in range(n):                                         # alone, and in a batch with other neighbours, in another slot
        alone = _backward(gy[s:s + 1].contiguous(), theta[s:s + 1], ins)
        assert torch.equal(_bits(alone[0]), _bits(first[s])), (name, s)
    order = list(range(n))[::-1]
    other = _backward(gy[order].contiguous(), theta[order], ins)
    assert torch.equal(_bits(other), _bits(first[order]))


# ---- 5. degenerate thetas -------------------------------------------------------------------------------------------------
S345 = (3, 4, 5)
GOOD = R.theta_from_params((0.3, -0.2, 0.4), 1.1, (0.1, 0.2, -0.3), in_size=S345)
DEGENERATE = {
    "all-outside": (np.concatenate([np.eye(3), [[1000.0], [0.0], [0.0]]], axis=1).reshape(12), "zeros"),
    "zero-A": (np.zeros(12), "nan"),
    "reach-5": (np.concatenate([0.2 * np.eye(3), np.zeros((3, 1))], axis=1).reshape(12), "nan"),
    "nan-theta": (np.full(12, np.nan), "nan"),
}


@pytest.mark.parametrize("name", list(DEGENERATE))
@pytest.mark.parametrize("slot", [0, 1])
def test_degenerate_thetas(name, slot):
    bad, expect = DEGENERATE[name]
    theta = np.stack([bad, GOOD] if slot == 0 else [GOOD, bad])
    gy = B.make_grad(2, S345, seed=3)
    ref = B.affine_warp_backward_ref(gy, theta, S345)
    gx = _backward(_dev(gy), theta, S345).cpu()
    if expect == "zeros":
        assert B.supported(bad) and not ref[slot].any()
        assert torch.equal(_bits(gx[slot]), torch.zeros(1, *S345, dtype=torch.int32))
    else:
        assert not B.supported(bad) and np.isnan(ref[slot]).all()
        assert bool(torch.isnan(gx[slot]).all())
    _check(gx[1 - slot], ref[1 - slot], f"{name}: the supported sample beside it")        # finite and within the bound
    assert np.abs(ref[1 - slot]).max() > 0.1


# ---- 6. diff_affine_warp --------------------------------------------------------------------------------------------------
def _planes(n, size, two_d=False):
    return _dev(R.make_input(n, size, seed=0), two_d), _dev(R.make_input(n, size, seed=1), two_d)


@pytest.mark.parametrize("name", ["rot3d", "rot2d", "crop"])
def test_diff_affine_warp_is_affine_warp_under_no_grad(name):
    from mpgan_amd import augment as A
    n, in_size, out_size, theta = B.CASES[name]
    two_d = in_size[0] == 1
    outs = out_size[1:] if two_d else out_size
    x0, x1 = _planes(n, in_size, two_d)
    th = _theta(theta, n)
    with torch.no_grad():
        y = A.diff_affine_warp(x0, th, out_size=outs, fill=-1.0)
        z0, z1 = A.diff_affine_warp(x0, th, x1, out_size=outs, fill=(-1.0, 0.5))
    w0, w1 = A.affine_warp(x0, th, x1, out_size=outs, mode="constant", fill=(-1.0, 0.5))
    assert not y.requires_grad and y.shape == (n, 1, *outs)
    assert torch.equal(_bits(y), _bits(w0)) and torch.equal(_bits(z0), _bits(w0)) and torch.equal(_bits(z1), _bits(w1))
    # the default fill is 0, and the forward's bits do not depend on whether a graph is recorded
    y0 = A.diff_affine_warp(x0.clone().requires_grad_(True), th, out_size=outs)
    assert y0.requires_grad
    assert torch.equal(_bits(y0), _bits(A.affine_warp(x0, th, out_size=outs, mode="constant", fill=0.0)))


@pytest.mark.parametrize("name", ["rot3d", "rot2d", "zoom2"])
def test_diff_affine_warp_gradient_is_the_backward_kernel(name, monkeypatch):
    from mpgan_amd import augment as A
    from mpgan_amd import ops
    n, in_size, out_size, theta = B.CASES[name]
    two_d = in_size[0] == 1
    ins, outs = (in_size[1:], out_size[1:]) if two_d else (in_size, out_size)
    th = _theta(theta, n)
    g0, g1 = _dev(B.make_grad(n, out_size, seed=1), two_d), _dev(B.make_grad(n, out_size, seed=2), two_d)
    want0, want1 = _backward(g0, theta, ins), _backward(g1, theta, ins)
    calls = []
    real = ops.affine_warp_backward
    monkeypatch.setattr(ops, "affine_warp_backward", lambda *a: calls.append(1) or real(*a))
    # one plane
    x0, x1 = _planes(n, in_size, two_d)
    x0.requires_grad_(True)
    A.diff_affine_warp(x0, th, out_size=outs, fill=-1.0).backward(g0)
    assert len(calls) == 1 and torch.equal(_bits(x0.grad), _bits(want0))
    _check(x0.grad, B.affine_warp_backward_ref(g0.cpu().numpy().reshape(n, *out_size), theta, in_size), f"{name} autograd")
    # two planes: only the plane that requires grad gets a launch and a gradient
    for needs in ((True, False), (False, True), (True, True)):
        del calls[:]
        x0, x1 = (t.requires_grad_(r) for t, r in zip(_planes(n, in_size, two_d), needs))
        y0, y1 = A.diff_affine_warp(x0, th, x1, out_size=outs, fill=(-1.0, 0.5))
        ((y0 * g0).sum() + (y1 * g1).sum()).backward()
        assert len(calls) == sum(needs), (needs, calls)
        for x, need, want in ((x0, needs[0], want0), (x1, needs[1], want1)):
            assert (x.grad is None) == (not need)
            if need:
                assert torch.equal(_bits(x.grad), _bits(want))
    # both require grad, only the second output is used: one launch, no gradient for the first
    del calls[:]
    x0, x1 = (t.requires_grad_(True) for t in _planes(n, in_size, two_d))
    (A.diff_affine_warp(x0, th, x1, out_size=outs)[1] * g1).sum().backward()
    assert len(calls) == 1 and x0.grad is None and torch.equal(_bits(x1.grad), _bits(want1))


def test_border_is_refused():
    from mpgan_amd import augment as A
    from mpgan_amd import ops
    x = torch.zeros(2, 1, 3, 4, 5, device="cuda")
    th = _theta(np.stack([EYE, EYE]), 2)
    with pytest.raises(ValueError, match="constant"):
        A.diff_affine_warp(x, th, mode="border")
    gx = torch.full_like(x, 3.0)
    with pytest.raises(ValueError, match="CONSTANT"):
        ops.affine_warp_backward(x, th, ops.WARP_BORDER, gx)
    from mpgan_amd import _lib
    i3 = (ctypes.c_int32 * 3)(3, 4, 5)
    assert _lib.lib().mpgan_affine_warp_backward(x.data_ptr(), 2, i3, i3, th.data_ptr(), ops.WARP_BORDER, gx.data_ptr(),
                                                 None) == -1
    assert b"border" in _lib.lib().mpgan_last_error()
    torch.cuda.synchronize()
    assert bool((gx == 3.0).all())                             # nothing was launched
    with pytest.raises(ValueError):                            # affine_warp itself still refuses gradients
        A.affine_warp(x.clone().requires_grad_(True), th, mode="constant")


def test_unaligned_and_non_contiguous_views():
    from mpgan_amd import augment as A
    n, in_size, out_size, theta = B.CASES["rot3d"]
    th = _theta(theta, n)
    x = _dev(R.make_input(n, in_size, seed=0))
    g = _dev(B.make_grad(n, out_size, seed=1))
    ref = x.clone().requires_grad_(True)
    y_ref = A.diff_affine_warp(ref, th, fill=-1.0)
    y_ref.backward(g)
    # a 4-byte offset into a larger buffer: contiguous, aligned to 4 bytes only (input, and through gy.contiguous() the gradient)
    buf = torch.zeros(x.numel() + 1, device="cuda")
    buf[1:] = x.flatten()
    odd = buf[1:].view(x.shape).requires_grad_(True)
    gbuf = torch.zeros(g.numel() + 3, device="cuda")
    gbuf[3:] = g.flatten()
    assert odd.data_ptr() % 16 == 4 and gbuf[3:].data_ptr() % 16 == 12
    y = A.diff_affine_warp(odd, th, fill=-1.0)
    y.backward(gbuf[3:].view(g.shape))
    assert torch.equal(_bits(y), _bits(y_ref)) and torch.equal(_bits(odd.grad), _bits(ref.grad))
    # non-contiguous: every second w of a wider tensor, and a gradient that is a permuted view
    wide = torch.zeros(*x.shape[:-1], 2 * x.shape[-1], device="cuda")
    wide[..., ::2] = x
    view = wide[..., ::2].requires_grad_(True)
    gview = g.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
    assert not view.is_contiguous() and not gview.is_contiguous() and torch.equal(gview, g)
    y = A.diff_affine_warp(view, th, fill=-1.0)
    y.backward(gview)
    assert torch.equal(_bits(y), _bits(y_ref)) and torch.equal(_bits(view.grad), _bits(ref.grad))


# ---- 7. diff_augment with the word "affine" -------------------------------------------------------------------------------
POLICY = "color,affine,translation,cutout"


@pytest.mark.parametrize("shape", [(2, 1, 6, 10, 12), (3, 1, 13, 10)], ids=str)
def test_diff_augment_composes_the_two_steps(shape):
    from mpgan_amd import augment as A
    from mpgan_amd import ops
    n, spatial = shape[0], shape[2:]
    gen = torch.Generator().manual_seed(8)
    x = (torch.rand(*shape, generator=gen) * 2 - 1).cuda()
    cond = (torch.rand(*shape, generator=gen) * 2 - 1).cuda()
    g = (torch.rand(*shape, generator=gen) - 0.4).cuda()
    p = A.sample_params(n, spatial, POLICY, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    assert p.ops == 31 and p.theta.is_cuda and p.theta.shape == (n, 12)
    rest = p._replace(ops=p.ops & ~A.AFFINE, theta=None)
    # the output: the warp with `fill`, then the old kernel on the result
    xg = x.clone().requires_grad_(True)
    y = A.diff_augment(xg, p, fill=-1.0)
    warped = A.affine_warp(x, p.theta, mode="constant", fill=-1.0)
    assert torch.equal(_bits(y), _bits(A.diff_augment(warped, rest, fill=-1.0)))
    assert not torch.equal(_bits(warped), _bits(x))
    # the gradient: affine_warp_backward(diffaug_backward(g))
    y.backward(g)
    ws = torch.empty(ops.diffaug_workspace(n, spatial) // 8, dtype=torch.float64, device="cuda")
    inner = ops.diffaug_backward(g, rest.ops, p.color, p.geom, ws, torch.empty_like(g))
    want = ops.affine_warp_backward(inner, p.theta, ops.WARP_CONSTANT, torch.empty_like(g))
    assert torch.equal(_bits(xg.grad), _bits(want)) and float(want.abs().max()) > 0
    # the word alone returns the warp's output
    alone = p._replace(ops=A.AFFINE)
    assert torch.equal(_bits(A.diff_augment(x, alone, fill=-1.0)), _bits(warped))
    # a condition: the same theta, no colour
    c = A.diff_augment(cond, p, color=False, fill=-1.0)
    spatial_only = rest._replace(ops=rest.ops & ~(A.BRIGHTNESS | A.CONTRAST))
    c_warped = A.affine_warp(cond, p.theta, mode="constant", fill=-1.0)
    assert torch.equal(_bits(c), _bits(A.diff_augment(c_warped, spatial_only, fill=-1.0))) and not c.requires_grad
    # the module: one draw for both, replayed from the seed
    m = A.DiffAugment(POLICY, fill=-1.0, generator=torch.Generator(device="cuda").manual_seed(3))
    ym, cm = m(x, cond)
    assert torch.equal(m.last_params.theta, p.theta) and torch.equal(m.last_params.geom, p.geom)
    assert torch.equal(_bits(ym), _bits(y)) and torch.equal(_bits(cm), _bits(c))
