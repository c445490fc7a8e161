"""The epilogues of the discriminator's dense fp32 launches at the smallest geometries that select their kernels:
mpgan_conv_backward_data_stats on both LDS-DMA forms (gather_conv_dma_kernel<128, 2, 2, 2, 2> and <64, 1, 2, 1, 2>)
and mpgan_conv_forward with fused statistics on the mask-free pipelined form, against fp64 references.

Bounds are those of test_conv_gpu.py and test_step_launches_gpu.py: with integer operands (exact in fp32 in any order)
outputs and sums equal the reference bit for bit; with random operands outputs sit within rtol 2e-4 (atol 2e-5 max|ref|)
and a fused sum within (L + 1) 2^-24 sum|terms|, L the longest addition chain of a partial row (conv_ref.check_sums).

The backward-data launch runs twice on the same data: with 16-byte aligned pitched views (the transposed, 16-byte
store path of the epilogue) and with views whose byte offset mod 16 is 4 (the element-wise walk).  Both add a channel's
elements in the same order, so their outputs and partial rows must be the same bits.  Every output is a channel slice
of a wider NaN-filled buffer and every partial-row buffer has a NaN tail: nothing may be written outside.

Which of the two epilogue paths a launch took leaves no trace in its results (that is the point of it), so these tests
pin what either path must compute; that aligned operands do take the 16-byte store path is shown by timing the product
library against the `make DEV=1 WALK=1` build (profiles/r13_dense_epilogue.txt)."""
import pytest
import torch

import conv_ref as R
from gpu_helpers import assert_close

pytestmark = pytest.mark.gpu

DMA128 = "gather_conv_dma_kernel<128, 2, 2, 2, 2>"
DMA64 = "gather_conv_dma_kernel<64, 1, 2, 1, 2>"
FAST = "gather_conv_pipe_kernel<128, 2, 2, 2, 1, 3, true, 1, false>"
TAIL = 64       # NaN floats behind the partial rows


def _geom(n, cin, cout, k, s, spatial):
    from mpgan_amd.ops import ConvGeom
    return ConvGeom(n, (1, *spatial), cin, cout, (1, k, k), (1, s, s), (0, 0, 0), min_blocks=1)


def _ints(shape, density, gen, lim=3):
    v = torch.randint(-lim, lim + 1, shape, generator=gen, device="cuda").float()
    return v * (torch.rand(shape, generator=gen, device="cuda") < density)


def _u(shape, gen):
    return torch.rand(shape, generator=gen, device="cuda") * 2 - 1


def _view(shape, lead, width, fill=float("nan")):
    """A (..., C) channel slice starting at channel `lead` of a NaN-filled buffer of `width` channels."""
    base = torch.full((*shape[:-1], width), fill, device="cuda")
    return base, base[..., lead:lead + shape[-1]]


def _guard_ok(base, view):
    mask = torch.ones_like(base, dtype=torch.bool)
    mask[..., view.storage_offset() % base.shape[-1]:view.storage_offset() % base.shape[-1] + view.shape[-1]] = False
    return bool(torch.isnan(base[mask]).all())


# (cin, cout, k, stride, spatial, n, kernel).  The launch's output is dx: `cin` channels.  A 128-row tile count of
# 256 (128 for two column tiles) is the least at which the library picks the wide forms (select_variant).
#   64 <- 128, 3x3: the 64-wide DMA form, from 385 tiles on (below that the in-block split-K form serves it);
#       M = 3*131*127 = 389*128 + 119 rows: the last tile ragged
#   128 <- 256, 4x4 stride 2, input 129 x 125 (odd): phases of 65x63, 65x62, 64x63, 64x62 pixels -- the tiles walk the
#       largest phase's extent, so the smaller phases have rows without an output pixel, and 2*65*63 = 63*128 + 126
#   256 <- 256, the same with one sample: two 128-wide column tiles per row tile
#   192 <- 64 and 96 <- 64, 3x3: channel counts that are no multiple of the 128-wide tile (the library picks it from 65
#       channels on) -- the last column tile has 64 / 96 live columns, so no tile of it is "interior": the per-element
#       walk of the 16-byte store path with its column tests, and z loads that must not run past the last channel
BWD_CASES = [
    (64, 128, 3, 1, (131, 127), 3, DMA64),
    (128, 256, 4, 2, (129, 125), 2, DMA128),
    (256, 256, 4, 2, (129, 125), 1, DMA128),
    (192, 64, 3, 1, (129, 127), 1, DMA128),
    (96, 64, 3, 1, (129, 127), 2, DMA128),
]


@pytest.mark.parametrize("tier", ["ints", "random"])
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "{}from{}_k{}s{}_{}x{}".format(*c[:4], *c[4]))
def test_backward_data_stats_epilogue(case, tier):
    from mpgan_amd import engine, ops
    cin, cout, k, s, spatial, n, kernel = case
    g = _geom(n, cin, cout, k, s, spatial)
    assert engine.gather_kernel_name(g, True, False) == kernel
    rows = ops.conv_bwd_stats_rows(g)
    assert rows > 0
    exact = tier == "ints"
    gen = torch.Generator(device="cuda").manual_seed(77 + cin + 3 * cout + spatial[0])
    T = k * k
    M_in = n * g.in_dhw[1] * g.in_dhw[2]
    if exact:      # as tier Xs of test_step_launches_gpu.py: scales +-4, shift 0, slope 0.25 (integers on both sides of the
        # kink), dy thin enough that the sums' magnitudes (2 fractional bits) stay below 2^24
        dy = _ints((n, *g.out_dhw, cout), min(4.0, 2.0 ** 20 / (M_in * 12.0)) / (cout * T), gen)
        w = _ints((cout, cin, k, k), 1.0, gen)
        zval = _ints((n, *g.in_dhw, cin), 0.5, gen)
        scale = 4.0 * (torch.randint(0, 2, (cin,), generator=gen, device="cuda").float() * 2 - 1)
        shift, mean, invstd = torch.zeros(cin, device="cuda"), torch.zeros(cin, device="cuda"), torch.ones(cin, device="cuda")
        slope = 0.25
    else:
        dy = _u((n, *g.out_dhw, cout), gen)
        w = _u((cout, cin, k, k), gen) / (cin * T) ** 0.5
        zval = _u((n, *g.in_dhw, cin), gen)
        scale, shift = _u((cin,), gen) * 0.5 + 1.0, _u((cin,), gen) * 0.3
        mean, invstd = _u((cin,), gen) * 0.2, _u((cin,), gen) * 0.3 + 1.0
        slope = 0.2
    wpb = ops.pack_weight(w, for_dgrad=True)
    ref = R.conv_backward_data(dy.double(), w.double().reshape(cout, cin, 1, k, k), (1, k, k), (1, s, s), (0, 0, 0), g.in_dhw)

    results = []
    for lead, width in ((4, cin + 8), (1, cin + 4)):        # byte offset mod 16: 0 (16-byte stores), 4 (element-wise walk)
        dx_base, dx = _view((n, *g.in_dhw, cin), lead, width)
        z_base, z = _view((n, *g.in_dhw, cin), lead, width, 7.0)
        z.copy_(zval)
        assert (dx.data_ptr() % 16 == 0) == (lead == 4) and (z.data_ptr() % 16 == 0) == (lead == 4)
        part = torch.full((rows * 3 * cin + TAIL,), float("nan"), device="cuda")
        assert ops.conv_backward_data_stats(g, dy, wpb, dx, z, scale, shift, mean, invstd, ops.ACT_LEAKY, slope, part) == rows
        torch.cuda.synchronize()
        assert _guard_ok(dx_base, dx), "dx: written outside its channel slice"
        assert bool(torch.isnan(part[rows * 3 * cin:]).all()), "partial rows: written past the last row"
        got = dx.clone()
        sums = part[:rows * 3 * cin].view(rows, 3, cin)
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(sums).all())
        want, mag = R.norm_bwd_sums(got.double(), zval.double(), scale.double(), shift.double(), mean.double(),
                                    invstd.double(), slope)
        if exact:
            ok, msg = R.check_exact(got, ref)
            assert ok, msg
            assert R.exact_sums_ok(mag, 2), f"operands too dense for exact sums: {mag.max().item()}"
            ok, ratio = R.check_sums(sums.double().sum(0), want, mag, 0, exact=True)
        else:
            assert_close(got, ref, what="dx")
            # a row adds at most row_chain terms; each term costs up to three roundings (zhat, gy * zhat)
            ok, ratio = R.check_sums(sums.double().sum(0), want, mag, R.row_chain(M_in, rows) + 4)
        print(f"{kernel} lead {lead}: norm-backward sums ratio {ratio:.3g}")
        assert ok, ratio
        results.append((got, sums.clone()))
    assert torch.equal(results[0][0], results[1][0]), "dx differs between the 16-byte store path and the walk"
    assert torch.equal(results[0][1], results[1][1]), "partial rows differ between the 16-byte store path and the walk"
    # ... and the plain launch leaves the same dx
    dx0 = torch.empty(n, *g.in_dhw, cin, device="cuda")
    ops.conv_backward_data(g, dy, wpb, dx0)
    assert torch.equal(dx0, results[0][0])


# (cin, cout, k, stride, spatial, n): the mask-free pipelined form needs a pad-free conv with cout % 128 == 0 and the
# same tile counts.
#   128 <- 64, 3x3, 131 x 129: M = 2*129*127 = 255*128 + 126 rows: the last tile ragged (its clamped rows are cleared
#       before the statistics)
#   256 <- 128, 4x4 stride 2, 184 x 182: M = 2*91*90 = 127*128 + 124, two column tiles
FWD_CASES = [
    (64, 128, 3, 1, (131, 129), 2),
    (128, 256, 4, 2, (184, 182), 2),
]


@pytest.mark.parametrize("tier", ["ints", "random"])
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "{}to{}_k{}s{}".format(*c[:4]))
def test_forward_statistics_epilogue(case, tier):
    from mpgan_amd import engine, ops
    cin, cout, k, s, spatial, n = case
    g = _geom(n, cin, cout, k, s, spatial)
    assert engine.gather_kernel_name(g, False, True, False, True) == FAST
    rows = ops.conv_stats_rows(g, 3)
    assert rows > 0
    exact = tier == "ints"
    gen = torch.Generator(device="cuda").manual_seed(177 + cin + 3 * cout)
    T = k * k
    if exact:      # one non-zero product per output on average: sum y^2 over the launch's 16K-32K pixels stays below 2^24
        x = _ints((n, *g.in_dhw, cin), 1.0 / (cin * T), gen)
        w = _ints((cout, cin, k, k), 1.0, gen)
        scale = 4.0 * (torch.randint(0, 2, (cin,), generator=gen, device="cuda").float() * 2 - 1)
        shift, bias, slope = torch.zeros(cin, device="cuda"), torch.zeros(cout, device="cuda"), 0.25
    else:
        x = _u((n, *g.in_dhw, cin), gen)
        w = _u((cout, cin, k, k), gen) / (cin * T) ** 0.5
        scale, shift, bias, slope = _u((cin,), gen) * 0.5 + 1.0, _u((cin,), gen) * 0.3, _u((cout,), gen) * 0.5, 0.2
    pro = ops.Prologue(scale, shift, 0, ops.ACT_LEAKY, slope)
    a = R.prologue(x.double(), scale.double(), shift.double(), 0, R.ACT_LEAKY, slope)
    aab = R.prologue(x.double(), scale.double(), shift.double(), 0, R.ACT_LEAKY, slope, absolute=True)
    w5 = w.double().reshape(cout, cin, 1, k, k)
    ref = R.conv_forward(a, w5, (1, k, k), (1, s, s), (0, 0, 0), g.out_dhw) + bias.double()
    absr = R.conv_forward(aab, w5.abs(), (1, k, k), (1, s, s), (0, 0, 0), g.out_dhw) + bias.double().abs()
    y_base, y = _view((n, *g.out_dhw, cout), 4, cout + 8)
    part = torch.full((rows * 2 * cout + TAIL,), float("nan"), device="cuda")
    ops.conv_forward(g, x, ops.pack_weight(w), bias, y, pro=pro, stats_partials=part)
    torch.cuda.synchronize()
    assert _guard_ok(y_base, y), "y: written outside its channel slice"
    assert bool(torch.isnan(part[rows * 2 * cout:]).all()), "statistics rows: written past the last row"
    got = y.clone()
    sums = part[:rows * 2 * cout].view(rows, 2, cout).double().sum(0)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(sums).all())
    M_out = n * g.out_dhw[1] * g.out_dhw[2]
    L = cin * T + 2 + 2
    want, mag, extra = R.stats_terms(ref, absr, 0 if exact else L)
    if exact:
        ok, msg = R.check_exact(got, ref)
        assert ok, msg
        assert R.exact_sums_ok(mag), f"operands too dense for exact statistics: {mag.max().item()}"
    else:
        assert_close(got, ref, what="y")
    ok, ratio = R.stats_check(sums, want, mag, extra, M_out, rows, exact)
    print(f"{FAST}: statistics ratio {ratio:.3g}")
    assert ok, ratio
