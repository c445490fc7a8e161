"""Every refusal of the Python layers around the trilinear-warp family (ops.affine_warp, ops.affine_warp_backward,
ops.affine_warp_backward_theta, ops.deform_warp; augment.affine_warp, augment.diff_affine_warp, augment.deform_warp):
one table per wrapper, each row a bad argument and the word (the argument's name or the rule) its ValueError must
contain.  Every call raises before the library is reached: ops.lib is replaced by a function that fails the test, and the
outputs, pre-filled with a sentinel, are compared once at the end.  No kernel runs, so the two shapes are tiny:
(2, 1, 3, 4, 5) and (2, 1, 6, 7).  The rows marked HOST fire before the device check and also run without a GPU."""
import pytest
import torch

S3, S2 = (2, 1, 3, 4, 5), (2, 1, 6, 7)
SENTINEL = -7.0
HOST = True


# ---- bad values derived from a good one --------------------------------------------------------------------------------
def _batch(t):
    return torch.full((t.shape[0] + 1, *t.shape[1:]), SENTINEL, dtype=t.dtype, device=t.device)


def _wider(t):
    return torch.zeros((*t.shape[:-1], t.shape[-1] + 1), dtype=t.dtype, device=t.device)


def _rank(t):
    """The image of the other rank: (B, 1, D, H, W) -> (B, 1, H, W) and back."""
    return t[:, :, 0].contiguous() if t.dim() == 5 else t.unsqueeze(2).contiguous()


def _strided(t):
    """The same shape and values, not contiguous."""
    return _wider(t)[..., :-1]


def _grad(t):
    return t.clone().requires_grad_(True)


def _lattice(t, axis, extent):
    shape = list(t.shape)
    shape[axis] = extent
    return torch.zeros(shape, dtype=t.dtype, device=t.device)


def _theta(dev):
    return torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).repeat(2, 1).to(dev)


THETA_ROWS = [("theta float32", lambda g: dict(theta=g["theta"].float()), "theta"),
              ("theta of one row", lambda g: dict(theta=g["theta"][:1].contiguous()), "theta"),
              ("theta strided", lambda g: dict(theta=_strided(g["theta"])), "theta"),
              ("theta None", lambda g: dict(theta=None), "theta")]


def _image_rows(first, last):
    """What _diffaug_geometry refuses on the first image and where the last tensor lives."""
    return [(f"{first} of rank 3", lambda g: {first: g[first][:, :, 0, 0]}, "B, 1, H, W", HOST),
            (f"{first} with two channels", lambda g: {first: torch.cat([g[first]] * 2, 1)}, "B, 1, H, W", HOST),
            (f"{first} float64", lambda g: {first: g[first].double()}, "float32", HOST),
            (f"{first} strided", lambda g: {first: _strided(g[first])}, "contiguous", HOST),
            (f"{first} on the CPU", lambda g: {first: g[first].cpu()}, "GPU", HOST),
            (f"{last} on the CPU", lambda g: {last: g[last].cpu()}, "GPU")]


# ---- ops.affine_warp and ops.deform_warp: positional, so the tables are keyed by the parameter names ---------------------
OPS_WARP_KEYS = ("x0", "x1", "theta", "mode", "fill0", "fill1", "noise0", "noise1", "sigma", "y0", "y1")
OPS_DEFORM_KEYS = ("x0", "x1", "theta", "ctrl", "gain", "gain_planes", "gamma", "lo", "hi", "mode", "fill0", "fill1",
                   "noise0", "noise1", "sigma", "y0", "y1")


def _ops_warp_good(shape, dev):
    z = lambda: torch.zeros(shape, device=dev)
    s = lambda: torch.full(shape, SENTINEL, device=dev)
    return dict(x0=z(), x1=z(), theta=_theta(dev), mode=0, fill0=0.0, fill1=0.0, noise0=z(), noise1=z(),
                sigma=torch.zeros((2, 2), device=dev), y0=s(), y1=s())


def _ops_deform_good(shape, dev):
    grid = (4, 4, 4) if len(shape) == 5 else (1, 4, 4)
    return dict(_ops_warp_good(shape, dev), ctrl=torch.zeros((2, 3, *grid), dtype=torch.float64, device=dev),
                gain=torch.zeros((2, *grid), dtype=torch.float64, device=dev), gain_planes=1,
                gamma=torch.ones((2, 2), dtype=torch.float64, device=dev), lo=-1.0, hi=1.0)


ONE_PLANE = dict(x1=None, y1=None, noise1=None)
OPS_WARP_ROWS = _image_rows("x0", "y1") + THETA_ROWS + [
    ("y0 with another batch", lambda g: dict(y0=_batch(g["y0"])), "y0"),
    ("y0 of the other rank", lambda g: dict(y0=_rank(g["y0"])), "y0"),
    ("y0 float64", lambda g: dict(y0=g["y0"].double()), "float32"),
    ("x1 of another shape", lambda g: dict(x1=_wider(g["x1"])), "second plane"),
    ("y1 of another shape", lambda g: dict(y1=_wider(g["y1"])), "second plane"),
    ("x1 without y1", lambda g: dict(y1=None), "go together"),
    ("y1 without x1", lambda g: dict(x1=None, noise1=None), "go together"),
    ("unknown mode", lambda g: dict(mode=2), "mode"),
    ("noise1 without a second plane", lambda g: dict(x1=None, y1=None), "noise1"),
    ("sigma without noise", lambda g: dict(noise0=None, noise1=None), "sigma"),
    ("noise without sigma", lambda g: dict(sigma=None), "sigma"),
    ("sigma float64", lambda g: dict(sigma=g["sigma"].double()), "sigma"),
    ("sigma of three columns", lambda g: dict(sigma=_wider(g["sigma"])), "sigma"),
    ("noise0 of another shape", lambda g: dict(noise0=_wider(g["noise0"])), "noise0"),
    ("noise1 float64", lambda g: dict(noise1=g["noise1"].double()), "noise1"),
    ("noise0 strided", lambda g: dict(noise0=_strided(g["noise0"])), "noise0")]

OPS_DEFORM_ROWS = OPS_WARP_ROWS + [
    ("ctrl is no tensor", lambda g: dict(ctrl=g["ctrl"].tolist()), "ctrl"),
    ("ctrl float32", lambda g: dict(ctrl=g["ctrl"].float()), "ctrl"),
    ("ctrl with two channels", lambda g: dict(ctrl=g["ctrl"][:, :2].contiguous()), "ctrl"),
    ("ctrl strided", lambda g: dict(ctrl=_strided(g["ctrl"])), "ctrl"),
    ("gain of the ctrl's rank", lambda g: dict(gain=g["ctrl"]), "gain"),
    ("ctrl lattice of extent 3", lambda g: dict(ctrl=_lattice(g["ctrl"], -1, 3)), "lattice"),
    ("gain lattice of extent 65", lambda g: dict(gain=_lattice(g["gain"], -2, 65)), "lattice"),
    ("ctrl lattice of extent 1 on a long axis", lambda g: dict(ctrl=_lattice(g["ctrl"], -1, 1)), "lattice"),
    ("gain_planes 0 with a gain", lambda g: dict(gain_planes=0), "gain_planes"),
    ("gain_planes 4", lambda g: dict(gain_planes=4), "gain_planes"),
    ("gain_planes 2 without a second plane", lambda g: dict(ONE_PLANE, gain_planes=2), "gain_planes"),
    ("hi == lo", lambda g: dict(hi=-1.0), "hi > lo"),
    ("hi < lo with gamma alone", lambda g: dict(gain=None, hi=-2.0), "hi > lo"),
    ("gamma float32", lambda g: dict(gamma=g["gamma"].float()), "gamma"),
    ("gamma of one row", lambda g: dict(gamma=g["gamma"][:1].contiguous()), "gamma")]
# an axis of extent 1 takes the lattice extent 1 alone: the d axis of the 2-D shape
OPS_DEFORM_ROWS_2D = [("ctrl lattice of extent 4 on the d axis", lambda g: dict(ctrl=_lattice(g["ctrl"], 2, 4)), "lattice"),
                      ("gain lattice of extent 4 on the d axis", lambda g: dict(gain=_lattice(g["gain"], 1, 4)), "lattice")]


# ---- ops.affine_warp_backward(gy, theta, mode, gx) ------------------------------------------------------------------------
OPS_BACKWARD_KEYS = ("gy", "theta", "mode", "gx")


def _ops_backward_good(shape, dev):
    return dict(gy=torch.zeros(shape, device=dev), theta=_theta(dev), mode=0, gx=torch.full(shape, SENTINEL, device=dev))


OPS_BACKWARD_ROWS = _image_rows("gy", "gx") + THETA_ROWS + [
    ("theta is no tensor", lambda g: dict(theta=g["theta"].tolist()), "theta"),
    ("gx with another batch", lambda g: dict(gx=_batch(g["gx"])), "gx"),
    ("gx of the other rank", lambda g: dict(gx=_rank(g["gx"])), "gx"),
    ("gx float64", lambda g: dict(gx=g["gx"].double()), "float32"),
    ("the border mode", lambda g: dict(mode=1), "CONSTANT"),
    ("unknown mode", lambda g: dict(mode=2), "mode")]


# ---- ops.affine_warp_backward_theta(x0, x1, gy0, gy1, theta, mode, fill0, fill1, gtheta) ---------------------------------
OPS_THETA_KEYS = ("x0", "x1", "gy0", "gy1", "theta", "mode", "fill0", "fill1", "gtheta")


def _ops_theta_good(shape, dev):
    z = lambda: torch.zeros(shape, device=dev)
    return dict(x0=z(), x1=z(), gy0=z(), gy1=z(), theta=_theta(dev), mode=0, fill0=0.0, fill1=0.0,
                gtheta=torch.full((2, 12), SENTINEL, dtype=torch.float64, device=dev))


OPS_THETA_ROWS = _image_rows("x0", "gy1") + THETA_ROWS + [
    ("theta is no tensor", lambda g: dict(theta=g["theta"].tolist()), "theta"),
    ("gy0 with another batch", lambda g: dict(gy0=_batch(g["gy0"])), "gy0"),
    ("gy0 of the other rank", lambda g: dict(gy0=_rank(g["gy0"])), "gy0"),
    ("x1 of another shape", lambda g: dict(x1=_wider(g["x1"])), "second plane"),
    ("gy1 of another shape", lambda g: dict(gy1=_wider(g["gy1"])), "second plane"),
    ("x1 without gy1", lambda g: dict(gy1=None), "go together"),
    ("gy1 without x1", lambda g: dict(x1=None), "go together"),
    ("the border mode", lambda g: dict(mode=1), "CONSTANT"),
    ("unknown mode", lambda g: dict(mode=2), "mode"),
    ("gtheta of eleven columns", lambda g: dict(gtheta=g["gtheta"][:, :11].contiguous()), "gtheta"),
    ("gtheta float32", lambda g: dict(gtheta=g["gtheta"].float()), "gtheta"),
    ("gtheta strided", lambda g: dict(gtheta=_strided(g["gtheta"])), "gtheta")]


# ---- augment.affine_warp and augment.deform_warp (x, theta, x1, *, ...) --------------------------------------------------
def _aug_good(shape, dev):
    return dict(x=torch.zeros(shape, device=dev), theta=_theta(dev), x1=torch.zeros(shape, device=dev))


def _aug_deform_good(shape, dev):
    grid, ndim = (4,) * (len(shape) - 2), len(shape) - 2
    return dict(_aug_good(shape, dev), ctrl=torch.zeros((2, ndim, *grid), dtype=torch.float64, device=dev),
                gain=torch.zeros((2, *grid), dtype=torch.float64, device=dev),
                gamma=torch.ones((2, 2), dtype=torch.float64, device=dev))


def _field(g):
    return torch.zeros_like(g["x"])


AUG_SHARED_ROWS = [
    ("x on the CPU", lambda g: dict(x=g["x"].cpu()), "GPU", HOST),
    ("x1 on the CPU", lambda g: dict(x1=g["x1"].cpu()), "GPU", HOST),
    ("x is no tensor", lambda g: dict(x=g["x"].tolist()), "GPU", HOST),
    ("fill of three numbers", lambda g: dict(fill=(0.0, 1.0, 2.0)), "fill"),
    ("out_size of the wrong rank", lambda g: dict(out_size=(4,) * (5 - g["x"].dim() + 2)), "out_size"),
    ("x1 of another shape", lambda g: dict(x1=_wider(g["x1"])), "second plane")] + THETA_ROWS

AUG_WARP_ROWS = AUG_SHARED_ROWS + [
    ("x requires grad", lambda g: dict(x=_grad(g["x"])), "differentiable"),
    ("x1 requires grad", lambda g: dict(x1=_grad(g["x1"])), "differentiable"),
    ("unknown mode", lambda g: dict(mode="nearest"), "mode"),
    ("noise of three fields", lambda g: dict(noise=(None, None, None)), "noise"),
    ("noise without sigma", lambda g: dict(noise=_field(g)), "sigma"),
    ("sigma without noise", lambda g: dict(sigma=torch.zeros((2, 2), device=g["x"].device)), "sigma"),
    ("noise for plane 1 without a second plane",
     lambda g: dict(x1=None, noise=(None, _field(g)), sigma=torch.zeros((2, 2), device=g["x"].device)), "noise1"),
    ("x float64", lambda g: dict(x=g["x"].double()), "float32")]

AUG_DEFORM_ROWS = AUG_WARP_ROWS + [
    ("ctrl is no tensor", lambda g: dict(ctrl=g["ctrl"].tolist()), "ctrl"),
    ("ctrl float32", lambda g: dict(ctrl=g["ctrl"].float()), "ctrl"),
    ("ctrl with one channel too many", lambda g: dict(ctrl=torch.cat([g["ctrl"], g["ctrl"][:, :1]], 1)), "ctrl"),
    ("gain of the ctrl's rank", lambda g: dict(gain=g["ctrl"]), "gain"),
    ("ctrl lattice of extent 3", lambda g: dict(ctrl=_lattice(g["ctrl"], -1, 3)), "lattice"),
    ("gain lattice of extent 65", lambda g: dict(gain=_lattice(g["gain"], -2, 65)), "lattice"),
    ("gain_planes names a third plane", lambda g: dict(gain_planes=(2,)), "gain_planes"),
    ("no gain plane with a gain", lambda g: dict(gain_planes=()), "gain_planes"),
    ("gain on plane 1 without a second plane", lambda g: dict(x1=None, gain_planes=(1,)), "gain_planes"),
    ("hi <= lo", lambda g: dict(value_range=(1.0, -1.0)), "hi > lo"),
    ("gamma float32", lambda g: dict(gamma=g["gamma"].float()), "gamma")]

AUG_DIFF_ROWS = AUG_SHARED_ROWS[:5] + THETA_ROWS + [
    ("the border mode", lambda g: dict(mode="border"), "constant", HOST),
    ("x float64", lambda g: dict(x=g["x"].double()), "float32"),
    ("x1 float64", lambda g: dict(x1=g["x1"].double()), "float32"),
    ("x1 of another shape", lambda g: dict(x1=_wider(g["x1"])), "one shape"),
    ("x of rank 3", lambda g: dict(x=g["x"][:, :, 0, 0], x1=None), "(B, 1, *S)")]


def _positional(fn, keys):
    return lambda **kw: fn(*(kw[k] for k in keys))


def _tables():
    from mpgan_amd import augment, ops
    return {"ops.affine_warp": (_positional(ops.affine_warp, OPS_WARP_KEYS), _ops_warp_good, OPS_WARP_ROWS, []),
            "ops.affine_warp_backward": (_positional(ops.affine_warp_backward, OPS_BACKWARD_KEYS), _ops_backward_good,
                                         OPS_BACKWARD_ROWS, []),
            "ops.affine_warp_backward_theta": (_positional(ops.affine_warp_backward_theta, OPS_THETA_KEYS),
                                               _ops_theta_good, OPS_THETA_ROWS, []),
            "ops.deform_warp": (_positional(ops.deform_warp, OPS_DEFORM_KEYS), _ops_deform_good, OPS_DEFORM_ROWS,
                                OPS_DEFORM_ROWS_2D),
            "augment.affine_warp": (augment.affine_warp, _aug_good, AUG_WARP_ROWS, []),
            "augment.diff_affine_warp": (augment.diff_affine_warp, _aug_good, AUG_DIFF_ROWS, []),
            "augment.deform_warp": (augment.deform_warp, _aug_deform_good, AUG_DEFORM_ROWS, [])}


WRAPPERS = ("ops.affine_warp", "ops.affine_warp_backward", "ops.affine_warp_backward_theta", "ops.deform_warp",
            "augment.affine_warp", "augment.diff_affine_warp", "augment.deform_warp")


def _run(wrapper, dev, monkeypatch, host_only):
    """Every row of one table at both shapes; returns the good arguments' tensors (the outputs hold the sentinel), each
    with a copy taken before the rows ran."""
    from mpgan_amd import ops

    def reached(*a, **k):
        raise AssertionError(f"{wrapper}: the library was reached")

    monkeypatch.setattr(ops, "lib", reached)
    call, good, rows, rows_2d = _tables()[wrapper]
    kept, count = [], 0
    for shape in (S3, S2):
        g = good(shape, dev)
        kept += [(t, t.clone()) for t in g.values() if isinstance(t, torch.Tensor)]
        for label, change, word, *host in rows + (rows_2d if shape is S2 else []):
            if host_only and not host:
                continue
            with pytest.raises(ValueError) as e:
                call(**dict(g, **change(g)))
            assert word in str(e.value), (wrapper, shape, label, word, str(e.value))
            count += 1
    assert count >= (4 if host_only else 16), (wrapper, count)
    return kept


@pytest.mark.gpu
@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_every_row_raises_before_any_launch(wrapper, monkeypatch):
    kept = _run(wrapper, "cuda", monkeypatch, host_only=False)
    torch.cuda.synchronize()                              # once: whatever a row had launched would have landed by now
    for t, was in kept:
        assert torch.equal(t, was), wrapper


@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_host_rows_without_a_device(wrapper, monkeypatch):
    """The rows that fire before the device check, and the device check itself, on CPU tensors."""
    _run(wrapper, "cpu", monkeypatch, host_only=True)
    call, good, _, _ = _tables()[wrapper]
    with pytest.raises(ValueError, match="GPU"):
        call(**good(S2, "cpu"))
