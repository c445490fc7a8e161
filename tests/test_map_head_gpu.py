"""The Markovian head's kernels (csrc/map_head.hip) through `ops`, at the smallest shapes at which each thing can go
wrong, against the float64 restatement of tests/map_head_ref.py.  Tolerance: gpu_helpers.assert_close at its defaults
with outliers=0, as test_linear1_head_forward_backward holds the Linear head (g_a and dw pass no activation kink)."""
import functools

import pytest
import torch

import map_head_ref as M
from gpu_helpers import assert_close, from_cl, t3, to_cl

pytestmark = pytest.mark.gpu

#        id                 n  c    in          prologue
CASES = {
    "2d_baseline":         (3, 64,  (9, 7),     "bn"),      # map 6x4
    "2d_map_1x1":          (2, 256, (4, 4),     "bn"),      # the head degenerates to Flatten + Linear
    "2d_few_quads":        (1, 8,   (4, 11),    "bn"),      # 2 channel quads on 64 lanes; map 1x8, input rows 8 + 3
    "3d_no_prologue":      (2, 256, (4, 5, 6),  None),      # 64 taps, map 1x2x3
    "3d_per_sample":       (2, 64,  (6, 6, 6),  "sample"),  # n_stride = c; map 3^3
    # beyond the issue's table: the kernels walk strips of 8 pixels along x and cap their grids at 2048 blocks of 4 waves
    "2d_two_strips":       (1, 16,  (5, 14),    "bn"),      # map 2x11: a full strip and a ragged one per row
    "2d_grid_stride":      (1, 4,   (1033, 67), "bn"),      # 8240 forward and 9297 backward strips > 8192 waves
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs (float32, CPU) and the float64 reference of one case, computed once and shared."""
    n, c, sp, pro = CASES[name]
    dims = len(sp)
    gen = torch.Generator().manual_seed(sorted(CASES).index(name) + 40)
    z = torch.rand(n, c, *sp, generator=gen) - 0.5
    sv = {"bn": (c,), "sample": (n, c), None: None}[pro]
    sc = sh = None
    if sv is not None:
        sc, sh = torch.rand(*sv, generator=gen) + 0.5, torch.rand(*sv, generator=gen) - 0.5
    w = (torch.rand(1, c, *(4,) * dims, generator=gen) - 0.5) / 8
    b = torch.rand(1, generator=gen) - 0.5
    out = tuple(s - 3 for s in sp)
    dl = torch.rand(n, 1, *out, generator=gen) - 0.5
    old_w, old_b = torch.rand(w.shape, generator=gen) - 0.5, torch.rand(1, generator=gen) - 0.5
    a64 = z.double() if sc is None else M.activate(z.double(), sc.double(), sh.double())
    logit, prob = M.head_forward(a64, w.double(), b.double())
    g_a, dw, db = M.head_backward(a64, w.double(), dl.double())
    return dict(n=n, c=c, sp=sp, dims=dims, out=out, z=z, sc=sc, sh=sh, w=w, b=b, dl=dl, old_w=old_w, old_b=old_b,
                a64=a64, logit=logit, prob=prob, g_a=g_a, dw=dw, db=db)


def _device(case):
    """The case on the device as the kernels take it: channels-last z, prologue, packed weight, k."""
    from mpgan_amd import ops
    pro = None
    if case["sc"] is not None:
        per_sample = case["sc"].dim() == 2
        pro = ops.Prologue(case["sc"].reshape(-1).cuda(), case["sh"].reshape(-1).cuda(), case["c"] if per_sample else 0,
                           ops.ACT_LEAKY, 0.2)
    return (to_cl(case["z"]), pro, t3(4, case["dims"], 1), ops.pack_weight(case["w"].cuda()), case["b"].cuda(),
            case["dl"].reshape(-1).cuda())


def _forward(case):
    from mpgan_amd import ops
    z, pro, k, wp, b, _ = _device(case)
    logit = torch.full((case["logit"].numel(),), float("nan"), device="cuda")
    prob = torch.full_like(logit, float("nan"))
    ops.maphead_forward(z, pro, k, wp, b, logit, prob)
    return logit, prob


def _backward(case, *, g_a=True, dw=True, db=True, beta=0.0, fill=float("nan")):
    from mpgan_amd import ops
    z, pro, k, wp, _, dl = _device(case)
    ws = torch.empty(ops.maphead_workspace(case["n"], z.shape[1:4], case["c"], k) // 4, device="cuda")
    G = torch.full_like(z, fill) if g_a else None
    W = (case["old_w"].cuda().clone() if beta else torch.full(case["w"].shape, fill, device="cuda")) if dw else None
    B = (case["old_b"].cuda().clone() if beta else torch.full((1,), fill, device="cuda")) if db else None
    ops.maphead_backward(z, pro, k, wp, dl, G, W, B, beta=beta, workspace=ws if dw else None)
    return G, W, B


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_match_the_float64_restatement(name):
    case = _case(name)
    logit, prob = _forward(case)
    assert_close(logit.cpu(), case["logit"].reshape(-1), what="logit")
    assert_close(prob.cpu(), case["prob"].reshape(-1), what="prob")
    g_a, dw, db = _backward(case)
    assert_close(from_cl(g_a, case["dims"]), case["g_a"], what="g_a")
    assert_close(dw.cpu(), case["dw"], what="dw (torch order)")
    assert_close(db.cpu(), case["db"], what="dbias")


def test_map_1x1_is_the_linear_head():
    """On a 4x4 feature map the head is Flatten + Linear(F, 1): the Linear head's kernel on the same packed data."""
    from mpgan_amd import ops
    case = _case("2d_map_1x1")
    z, pro, k, wp, b, _ = _device(case)
    n = case["n"]
    logit_lin = torch.empty(n, device="cuda")
    ops.linear1_forward(z, pro, wp, b, torch.empty(ops.linear1_partials(n), device="cuda"), logit_lin)
    logit, _ = _forward(case)
    assert_close(logit_lin.cpu(), case["logit"].reshape(-1), what="linear1 logit")
    assert_close(logit.cpu(), logit_lin.cpu(), what="maphead vs linear1 logit")


def test_3d_corner_pixels_get_exactly_one_contribution():
    """Input pixel (0,0,0) is seen by map pixel (0,0,0) through tap 0 only, the last input pixel by the last map pixel
    through the last tap only: one product, no sum, so the bits are those of a single fp32 multiply."""
    case = _case("3d_no_prologue")
    g_a, _, _ = _backward(case)
    _, _, _, wp, _, dl = _device(case)
    wp = wp.view(64, case["c"])
    dl = dl.view(case["n"], -1)
    for s in range(case["n"]):
        assert torch.equal(g_a[s, 0, 0, 0], dl[s, 0] * wp[0])
        assert torch.equal(g_a[s, -1, -1, -1], dl[s, -1] * wp[63])


@pytest.mark.parametrize("name", ["2d_baseline", "3d_per_sample"])
def test_beta_one_accumulates(name):
    case = _case(name)
    _, dw, db = _backward(case, g_a=False, beta=1.0)
    assert_close(dw.cpu(), case["old_w"].double() + case["dw"], what="dw, beta = 1")
    assert_close(db.cpu(), case["old_b"].double() + case["db"], what="dbias, beta = 1")
    # ... and it is old + exactly what beta = 0 writes
    _, dw0, db0 = _backward(case, g_a=False)
    assert torch.equal(dw, case["old_w"].cuda() + dw0) and torch.equal(db, case["old_b"].cuda() + db0)


@pytest.mark.parametrize("name", ["2d_baseline", "3d_no_prologue"])
def test_each_output_is_nullable_and_the_others_keep_their_bits(name):
    from mpgan_amd import ops
    case = _case(name)
    full = _backward(case)
    for absent in range(3):
        want = [i != absent for i in range(3)]
        got = _backward(case, g_a=want[0], dw=want[1], db=want[2])
        for i in range(3):
            if want[i]:
                assert torch.equal(got[i], full[i]), (absent, i)
            else:
                assert got[i] is None
    logit, prob = _forward(case)
    z, pro, k, wp, b, _ = _device(case)
    only = torch.empty_like(logit)
    ops.maphead_forward(z, pro, k, wp, b, only, None)                  # prob is nullable
    assert torch.equal(only, logit)
    no_bias = torch.empty_like(logit)
    ops.maphead_forward(z, pro, k, wp, None, no_bias, None)
    assert_close(no_bias.cpu(), case["logit"].reshape(-1) - case["b"].double(), what="logit without bias")


@pytest.mark.parametrize("name", list(CASES))
def test_two_runs_give_the_same_bits(name):
    case = _case(name)
    (l1, p1), (l2, p2) = _forward(case), _forward(case)
    assert torch.equal(l1, l2) and torch.equal(p1, p2)
    a, b = _backward(case), _backward(case)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
