"""The differentiable-augmentation kernels (csrc/diffaug.hip) through ops.diffaug_* and augment.diff_augment against the
float64 restatement of tests/diffaug_ref.py, at the smallest shapes at which they can go wrong: odd extents, W % 4 != 0
(element-wise path; sample 1 off 16-byte alignment), W % 4 == 0 (16-byte path, shifts that are no multiple of 4), several
partial blocks per sample.

Bounds, eps = 2^-23:
  spatial ops alone   y and g_x are copies, zeros and `fill`: bit for bit
  with a colour op    |y - y64|   <= 4 eps (c |x - m| + (1 + c) |m| + |b|)   one rounded subtract, one multiply, two adds
                                                                             and the fp32 rounding of m
                      |g_x - g64| <= 4 eps (c |g_u| + |1 - c| |sum g_u| / N)
                      and where keep is false y is `fill` exactly
"""
import functools

import pytest
import torch

import diffaug_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
FILLS = (0.0, -1.5)


@functools.lru_cache(maxsize=None)
def _sets(shape):
    return R.param_sets(shape)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(x, g_y) fp32 on the CPU: computed once, never modified."""
    return R.make_input(shape), R.make_input(shape, seed=1, offset=-0.2)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ws(n, spatial, ops_mask):
    from mpgan_amd import ops
    if not ops_mask & R.CONTRAST:
        return None
    return torch.empty(ops.diffaug_workspace(n, spatial) // 8, dtype=torch.float64, device="cuda")


def _offset_view(t):
    """A contiguous copy of t that starts 4 bytes into its allocation."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _forward(x, ops_mask, color, geom, fill, views=False):
    from mpgan_amd import ops
    y = torch.empty_like(x)
    if views:
        x, y = _offset_view(x), _offset_view(y)
    return ops.diffaug_forward(x, ops_mask, color, geom, fill, _ws(x.shape[0], tuple(x.shape[2:]), ops_mask), y)


def _backward(gy, ops_mask, color, geom, views=False):
    from mpgan_amd import ops
    gx = torch.empty_like(gy)
    if views:
        gy, gx = _offset_view(gy), _offset_view(gx)
    return ops.diffaug_backward(gy, ops_mask, color, geom, _ws(gy.shape[0], tuple(gy.shape[2:]), ops_mask), gx)


def _check_forward(y, x, color, geom, ops_mask, fill, what):
    """Exact without a colour op, the derived bound with one."""
    want = R.forward(x, color, geom, ops_mask, fill)
    if not ops_mask & R.COLOR:
        assert torch.equal(_bits(y), _bits(want.float())), what
        return 0.0
    x64 = x.double()
    b, c, m = R.color_terms(x64, color, ops_mask)
    bound_u = 4 * EPS * (c * (x64 - m).abs() + (1 + c) * m.abs() + b.abs())
    bound = R.forward(bound_u, color, geom, ops_mask & ~R.COLOR, 0.0)       # the bound travels with its element; 0 = exact
    err = (y.detach().cpu().double() - want).abs()
    assert bool((err <= bound).all()), (what, float((err - bound).max()))
    return float((err / bound.clamp_min(1e-300)).max())


def _check_backward(gx, gy, color, geom, ops_mask, what):
    want, gu, total = R.backward(gy, color, geom, ops_mask)
    if not ops_mask & R.COLOR:
        assert torch.equal(_bits(gx), _bits(want.float())), what
        return 0.0
    _, c, _ = R.color_terms(gu, color, ops_mask)
    bound = 4 * EPS * (c * gu.abs() + (1 - c).abs() * total.abs() / gu[0].numel())
    err = (gx.detach().cpu().double() - want).abs()
    assert bool((err <= bound).all()), (what, float((err - bound).max()))
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_spatial_ops_are_bit_exact(shape):
    x, gy = _inputs(shape)
    xc, gc = x.cuda(), gy.cuda()
    for name, color, geom in _sets(shape):
        cc, gg = color.cuda(), geom.cuda()
        for ops_mask in R.OPS_SPATIAL:
            for fill in FILLS:
                _check_forward(_forward(xc, ops_mask, cc, gg, fill), x, color, geom, ops_mask, fill, (name, ops_mask, fill))
            _check_backward(_backward(gc, ops_mask, cc, gg), gy, color, geom, ops_mask, (name, ops_mask))
            # the tables of disabled ops are ignored: no colour table at all
            assert torch.equal(_bits(_forward(xc, ops_mask, None, gg, 0.0)), _bits(_forward(xc, ops_mask, cc, gg, 0.0)))
    # no op at all: a copy
    assert torch.equal(_bits(_forward(xc, 0, None, None, 3.0)), _bits(x))
    assert torch.equal(_bits(_backward(gc, 0, None, None)), _bits(gy))


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_colour_ops_meet_the_rounding_bounds(shape):
    x, gy = _inputs(shape)
    xc, gc = x.cuda(), gy.cuda()
    worst = [0.0, 0.0]
    for name, color, geom in _sets(shape):
        cc, gg = color.cuda(), geom.cuda()
        for ops_mask in R.OPS_COLOR:
            for fill in FILLS:
                worst[0] = max(worst[0], _check_forward(_forward(xc, ops_mask, cc, gg, fill), x, color, geom, ops_mask, fill,
                                                        (name, ops_mask, fill)))
            worst[1] = max(worst[1], _check_backward(_backward(gc, ops_mask, cc, gg), gy, color, geom, ops_mask,
                                                     (name, ops_mask)))
        # colour ops alone need no geometry table
        _check_forward(_forward(xc, R.COLOR, cc, None, 0.0), x, color, geom, R.COLOR, 0.0, (name, "no geom"))
    print(f"{shape}: worst error / bound forward {worst[0]:.3f}, backward {worst[1]:.3f}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_views_four_bytes_into_an_allocation(shape):
    """x / y (g_y / g_x) that start 4 bytes into their allocation: the element-wise path, the same bounds."""
    x, gy = _inputs(shape)
    xc, gc = x.cuda(), gy.cuda()
    for name, color, geom in _sets(shape)[1::2]:
        cc, gg = color.cuda(), geom.cuda()
        for ops_mask in (R.TRANSLATION | R.CUTOUT, R.ALL):
            y = _forward(xc, ops_mask, cc, gg, -1.5, views=True)
            _check_forward(y, x, color, geom, ops_mask, -1.5, (name, ops_mask, "views"))
            gx = _backward(gc, ops_mask, cc, gg, views=True)
            _check_backward(gx, gy, color, geom, ops_mask, (name, ops_mask, "views"))
            # only one side misaligned
            from mpgan_amd import ops
            y2 = ops.diffaug_forward(_offset_view(xc), ops_mask, cc, gg, -1.5, _ws(shape[0], shape[2:], ops_mask), torch.empty_like(xc))
            _check_forward(y2, x, color, geom, ops_mask, -1.5, (name, ops_mask, "x view"))
            if not ops_mask & R.COLOR:
                assert torch.equal(_bits(y2), _bits(y))


@pytest.mark.parametrize("shape", [R.SHAPES_2D[2], R.SHAPES_3D[2], R.SHAPES_3D[3]], ids=str)
def test_two_runs_give_the_same_bits(shape):
    x, gy = _inputs(shape)
    xc, gc = x.cuda(), gy.cuda()
    for name, color, geom in _sets(shape)[-2:]:
        cc, gg = color.cuda(), geom.cuda()
        y1, y2 = _forward(xc, R.ALL, cc, gg, 0.0), _forward(xc, R.ALL, cc, gg, 0.0)
        assert torch.equal(_bits(y1), _bits(y2))
        g1, g2 = _backward(gc, R.ALL, cc, gg), _backward(gc, R.ALL, cc, gg)
        assert torch.equal(_bits(g1), _bits(g2))


@pytest.mark.parametrize("shape", [R.SHAPES_2D[1], R.SHAPES_2D[2], R.SHAPES_3D[2], R.SHAPES_3D[3]], ids=str)
def test_diff_augment_autograd(shape):
    """augment.diff_augment: the forward kernel's bits, autograd's gradient = the backward kernel's bits, only the two
    parameter tables saved, and color=False = the spatial ops alone."""
    from mpgan_amd import augment as A
    x, gy = _inputs(shape)
    gc = gy.cuda()
    for name, color, geom in _sets(shape)[-3:]:
        p = A.DiffAugParams(color.cuda(), geom.cuda(), R.ALL)
        for use_color, mask in ((True, R.ALL), (False, R.TRANSLATION | R.CUTOUT)):
            xc = x.cuda().requires_grad_(True)
            y = A.diff_augment(xc, p, color=use_color, fill=0.5)
            assert y.shape == xc.shape and y.dtype == torch.float32 and y.requires_grad
            assert torch.equal(_bits(y), _bits(_forward(xc.detach(), mask, p.color, p.geom, 0.5)))
            _check_forward(y, x, color, geom, mask, 0.5, (name, use_color))
            saved = y.grad_fn.saved_tensors
            assert len(saved) == 2 and {t.data_ptr() for t in saved} == {p.color.data_ptr(), p.geom.data_ptr()}
            assert all(t.numel() <= 9 * shape[0] for t in saved)
            y.backward(gc)
            assert torch.equal(_bits(xc.grad), _bits(_backward(gc, mask, p.color, p.geom)))
            _check_backward(xc.grad, gy, color, geom, mask, (name, use_color))
        # an input that needs no gradient (the condition of a conditional discriminator) gives a plain tensor
        assert not A.diff_augment(x.cuda(), p, color=False).requires_grad
        # a non-contiguous input is made contiguous first
        wide = torch.zeros(*shape[:-1], shape[-1] + 3, device="cuda")
        wide[..., :shape[-1]] = x.cuda()
        assert torch.equal(_bits(A.diff_augment(wide[..., :shape[-1]], p)), _bits(A.diff_augment(x.cuda(), p)))


def test_module_draws_fresh_parameters_on_the_device():
    from mpgan_amd import augment as A
    gen = torch.Generator(device="cuda").manual_seed(3)
    aug = A.DiffAugment("color,translation,cutout", fill=-1.0, generator=gen)
    assert not list(aug.parameters()) and not list(aug.buffers()) and not aug.state_dict()
    x, _ = _inputs(R.SHAPES_3D[2])
    xc = x.cuda()
    y1 = aug(xc)
    p1 = aug.last_params
    assert p1.color.is_cuda and p1.geom.is_cuda and p1.ops == R.ALL
    y2, c2 = aug(xc, xc)
    p2 = aug.last_params
    assert not torch.equal(p1.color, p2.color)
    replay = torch.Generator(device="cuda").manual_seed(3)
    for y, p in ((y1, p1), (y2, p2)):
        q = A.sample_params(xc.shape[0], xc.shape[2:], "color,translation,cutout", generator=replay, device="cuda")
        assert torch.equal(q.color, p.color) and torch.equal(q.geom, p.geom)
        assert torch.equal(_bits(y), _bits(A.diff_augment(xc, q, fill=-1.0)))
        _check_forward(y, x, p.color.cpu(), p.geom.cpu(), R.ALL, -1.0, "module")
    assert torch.equal(_bits(c2), _bits(A.diff_augment(xc, p2, color=False, fill=-1.0)))
    _check_forward(c2, x, p2.color.cpu(), p2.geom.cpu(), R.TRANSLATION | R.CUTOUT, -1.0, "module, condition")


def test_ops_refuse_bad_tensors():
    from mpgan_amd import ops
    x = torch.zeros(2, 1, 8, 8, device="cuda")
    color, geom = torch.zeros(2, 2, device="cuda"), torch.zeros(2, 9, dtype=torch.int32, device="cuda")
    ws = torch.empty(2, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    ops.diffaug_forward(x, 15, color, geom, 0.0, ws, y)
    bad = [dict(x=x.double()), dict(x=x.cpu()), dict(x=x[:, :, :, ::2]), dict(x=x.view(2, 8, 8)), dict(x=x.expand(2, 2, 8, 8)),
           dict(y=torch.empty(2, 1, 8, 4, device="cuda")), dict(color=color.double()), dict(color=color[:1]), dict(color=None),
           dict(geom=geom.long()), dict(geom=geom[:, :8].contiguous()), dict(geom=None), dict(geom=geom.cpu()),
           dict(ws=None), dict(ws=ws[:1]), dict(ws=ws.float()), dict(mask=16)]
    for kw in bad:
        a = dict(x=x, mask=15, color=color, geom=geom, ws=ws, y=y)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.diffaug_forward(a["x"], a["mask"], a["color"], a["geom"], 0.0, a["ws"], a["y"])
        if "y" not in kw:
            with pytest.raises(ValueError):
                ops.diffaug_backward(a["x"], a["mask"], a["color"], a["geom"], a["ws"], a["y"])
