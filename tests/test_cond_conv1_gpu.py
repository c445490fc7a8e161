"""The conditional discriminator's first conv at kernel level (mpgan_conv2p_*): Conv(2, 64, 3) over two
separate 1-channel planes, through ops, against tests/cond_disc_ref.py in float64.  The planes differ from each other
and so do the two planes of the weight, so a swapped plane or pack order shows.  Shapes: the smallest at which the row
walker takes each of its paths -- 4 output columns (one exact group), 5 and 7 (a last group re-anchored over 3 and 1
counted pixels), three output rows for a block's four waves, two samples, and 3-D.

Bounds.  An output is 54 products and 54 additions and a bias: 55 fp32 roundings of at most 2^-24 = 6e-8 of the running
magnitude each, so |y - y64| <= 55 * 6e-8 * (|w| * |x| + |b|) < 1e-5 * (|w| * |x| + |b|); a bf16 result adds half a bf16
ulp, 2^-8 |y64|.  Sums over pixels (statistics, weight gradient, bias gradient) are held to 1e-5 of the sum of the
magnitudes of their terms."""
import functools

import pytest
import torch

import cond_disc_ref as R
from gpu_helpers import assert_close, from_cl, to_cl

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

CASES = {  # id: (n, spatial)
    "2d-w6": (1, (6, 6)), "2d-w7": (1, (6, 7)), "2d-w9": (1, (6, 9)), "2d-h5": (1, (5, 8)), "2d-n2": (2, (7, 10)),
    "3d": (1, (5, 6, 8)),
}


def _geom(n, spatial, cin=2):
    from mpgan_amd.ops import ConvGeom
    d = len(spatial)
    pad3 = lambda v, fill: (fill,) * (3 - d) + (v,) * d
    return ConvGeom(n, (1,) * (3 - d) + tuple(spatial), cin, 64, pad3(3, 1), (1, 1, 1), (0, 0, 0))


@functools.lru_cache(maxsize=None)
def _case(cid):
    """Inputs (fp32 values held in float64) and the float64 reference of one case, computed once."""
    n, spatial = CASES[cid]
    dims = len(spatial)
    gen = torch.Generator().manual_seed(1000 + sorted(CASES).index(cid))
    r = lambda *s: torch.rand(*s, generator=gen)
    img, cond = r(n, 1, *spatial) * 2 - 1, r(n, 1, *spatial) * 3 - 1
    w = (r(64, 2, *([3] * dims)) - 0.5) * torch.tensor([0.5, 1.5]).view(1, 2, *([1] * dims))
    b = r(64) - 0.5
    c = dict(n=n, spatial=spatial, dims=dims, img=img, cond=cond, w=w, b=b)
    d = lambda t: t.double()
    c["y"] = R.conv1(d(img), d(cond), d(w), d(b))
    c["yscale"] = R.conv1_scale(d(img), d(cond), d(w), d(b))
    c["yscale_nobias"] = R.conv1_scale(d(img), d(cond), d(w), torch.zeros(64, dtype=torch.float64))
    c["epi"] = (r(64) + 0.5, r(64) - 0.5, torch.where(r(64) > 0.3, torch.full((64,), 0.2), torch.ones(64)))
    for name, dy in (("f32", r(*c["y"].shape) - 0.5), ("bf16", (r(*c["y"].shape) - 0.5).to(BF).float())):
        dx, dw, db = R.conv1_grads(d(img), d(cond), d(w), d(dy))
        c["bwd_" + name] = dict(dy=dy, dx=dx, dw=dw, db=db, dwscale=R.conv1_wgrad_scale(d(img), d(cond), d(dy)),
                                dbscale=d(dy).abs().transpose(0, 1).reshape(64, -1).sum(1))
    c["dw0"], c["db0"] = r(*w.shape) - 0.5, r(64) - 0.5
    return c


def _within(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    over = err - bound
    print(f"{what}: max err {err.max().item():.3e}, max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (over <= 0).all(), (what, err.max().item(), over.max().item())


@pytest.mark.parametrize("out", ["f32", "bf16"])
@pytest.mark.parametrize("cid", list(CASES))
def test_forward_and_statistics(cid, out):
    from mpgan_amd import ops
    c = _case(cid)
    g = _geom(c["n"], c["spatial"])
    bf = out == "bf16"
    T = 3 ** c["dims"]
    assert ops.conv2p_kernel_name(g, bf) == f"thin_cin2_rows_kernel<{T}, {'true' if bf else 'false'}>"
    rows = ops.conv2p_stats_rows(g, bf)
    M = c["y"].numel() // 64
    assert rows == ((M + 255) // 256 if bf else 0)            # where the one-plane conv1 leaves them: bf16 out only
    y = torch.empty(c["n"], *g.out_dhw, 64, device="cuda", dtype=BF if bf else torch.float32)
    part = torch.full((max(rows, 1) * 128,), float("nan"), device="cuda") if bf else None
    ops.conv2p_forward(g, c["img"].cuda(), c["cond"].cuda(), ops.pack_weight(c["w"].cuda()), c["b"].cuda(), y,
                       stats_partials=part)
    bound = 1e-5 * c["yscale"] + (2.0 ** -8 * c["y"].abs() if bf else 0)
    _within(from_cl(y.float(), c["dims"]), c["y"], bound, "y")
    if bf:
        st = part.view(rows, 2, 64).double().sum(0).cpu()
        per_c = lambda t: t.transpose(0, 1).reshape(64, -1).sum(1)
        _within(st[0], per_c(c["y"]), 1e-5 * per_c(c["y"].abs()), "sum y")
        _within(st[1], per_c(c["y"] ** 2), 1e-5 * per_c(c["y"] ** 2), "sum y^2")


@pytest.mark.parametrize("out", ["f32", "bf16"])
@pytest.mark.parametrize("cid", list(CASES))
def test_forward_with_the_eval_epilogue(cid, out):
    """y = lrelu(conv * scale + shift, slope): the conv's error times |scale|, plus the affine's own two roundings."""
    from mpgan_amd import ops
    c = _case(cid)
    g = _geom(c["n"], c["spatial"])
    bf = out == "bf16"
    sc, sh, sl = c["epi"]
    shp = [1, 64] + [1] * c["dims"]
    conv = c["y"] - c["b"].double().view(shp)                 # the entry takes no bias: it is folded into shift
    lin = conv * sc.double().view(shp) + sh.double().view(shp)
    want = torch.where(lin > 0, lin, lin * sl.double().view(shp))
    y = torch.empty(c["n"], *g.out_dhw, 64, device="cuda", dtype=BF if bf else torch.float32)
    ops.conv2p_forward_act(g, c["img"].cuda(), c["cond"].cuda(), ops.pack_weight(c["w"].cuda()), sc.cuda(), sh.cuda(),
                           sl.cuda(), y)
    bound = 1e-5 * (c["yscale_nobias"] * sc.double().view(shp) + sh.double().abs().view(shp))
    _within(from_cl(y.float(), c["dims"]), want, bound + (2.0 ** -8 * want.abs() if bf else 0), "activated y")


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("dy_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cid", list(CASES))
def test_weight_and_bias_gradient(cid, dy_dtype, beta):
    from mpgan_amd import ops
    c = _case(cid)
    g = _geom(c["n"], c["spatial"])
    ref = c["bwd_" + dy_dtype]
    bf = dy_dtype == "bf16"
    T = 3 ** c["dims"]
    assert ops.conv2p_wgrad_kernel_name(g, bf) == f"wgrad_thin2_rows_kernel<{T}, {'true' if bf else 'false'}>"
    dy = to_cl(ref["dy"]).to(BF) if bf else to_cl(ref["dy"])
    dw, db = c["dw0"].cuda().contiguous(), c["db0"].cuda().contiguous()
    ws = torch.empty(max(ops.conv2p_wgrad_workspace(g) // 4, 4), device="cuda")
    ops.conv2p_backward_weight(g, c["img"].cuda(), c["cond"].cuda(), dy, dw, ws, beta=beta, dbias=db)
    assert dw.shape == (64, 2, *([3] * c["dims"]))
    _within(dw, ref["dw"] + beta * c["dw0"].double(), 1e-5 * (ref["dwscale"] + beta * c["dw0"].double().abs()), "dW")
    _within(db, ref["db"] + beta * c["db0"].double(), 1e-5 * (ref["dbscale"] + beta * c["db0"].double().abs()), "dbias")


@pytest.mark.parametrize("dy_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cid", list(CASES))
def test_image_plane_backward_data(cid, dy_dtype):
    """dL/d img = channel 0 of the input gradient: the existing C -> 1 gather forms over the layout-3 pack."""
    import dataclasses
    from mpgan_amd import ops
    c = _case(cid)
    g1 = dataclasses.replace(_geom(c["n"], c["spatial"]), cin=1)
    ref = c["bwd_" + dy_dtype]
    wp = ops.pack_weight_plane0_bwd(c["w"].cuda())
    assert wp.numel() == 64 * 3 ** c["dims"]
    dx = torch.full((c["n"], *g1.in_dhw, 1), float("nan"), device="cuda")
    if dy_dtype == "bf16":
        ops.conv_backward_data_bf16_to_f32(g1, to_cl(ref["dy"]).to(BF), wp, dx)
    else:
        ops.conv_backward_data(g1, to_cl(ref["dy"]), wp, dx)
    assert_close(from_cl(dx, c["dims"]), ref["dx"], what="dL/d img")


def test_refusals_name_the_condition():
    """Geometries outside the row walker's conditions are refused with a message, before any launch."""
    from mpgan_amd import ops
    g = _geom(1, (6, 5))                                      # 3 output columns
    with pytest.raises(RuntimeError, match="at least 4 output columns"):
        ops.conv2p_kernel_name(g, False)
    assert ops.conv2p_stats_rows(g, True) == 0 and ops.conv2p_wgrad_workspace(g) == -1
    y = torch.empty(1, *g.out_dhw, 64, device="cuda")
    x = torch.zeros(1, 1, 6, 5, device="cuda")
    with pytest.raises(RuntimeError, match="at least 4 output columns"):
        ops.conv2p_forward(g, x, x, torch.zeros(64 * 18, device="cuda"), torch.zeros(64, device="cuda"), y)
    g = _geom(1, (6, 8))
    y = torch.empty(1, *g.out_dhw, 64, device="cuda")
    x = torch.zeros(1, 1, 6, 8, device="cuda")
    with pytest.raises(RuntimeError, match="no fused statistics"):   # fp32 out: as the one-plane conv1
        ops.conv2p_forward(g, x, x, torch.zeros(64 * 18, device="cuda"), torch.zeros(64, device="cuda"), y,
                           stats_partials=torch.zeros(256, device="cuda"))
