"""The fp32 peer-tap path of the three norm-backward launches (the `peer` argument of mpgan_norm_bwd_reduce and
mpgan_norm_bwd_apply, variant B's perceptual taps) against the fp64 formula, at the smallest shapes where the row and
column indexing can go wrong.

    y = z*scale + shift, a = LeakyReLU(y), zhat = (z - mean)*invstd, and likewise y', a' of the peer pass's z'
    g_a = g - ca*sign(a' - a),  gy = g_a*act'(y) - cy*sign(y' - y)
    dbeta = sum gy, dgamma = sum gy*zhat, c1 = dbeta / count, c2 = dgamma / count
    dz = scale*(gy - c1 - zhat*c2) - cz*sign(z' - z)

The inputs are exact in fp32 (z, z', g on multiples of 1/8, scales from {1/2, 1, 2}, shifts on multiples of 1/4, slope
1/4), so y, y', a and a' are exact and sign() sees the same zeros in fp32 and fp64.  mean and invstd are inputs of
the launches: arbitrary vectors with positive invstd.  Tolerance: that of test_norm_prelu_forward_backward for the same
three launches (assert_close, rtol = 1e-3)."""
import pytest
import torch

from gpu_helpers import assert_close, from_cl, to_cl

SLOPE = 0.25
COEF = (0.375, 0.25, 0.5)            # (cz, cy, ca): non-zero, distinct
# (n, c, spatial)
SHAPES = [(2, 16, (1, 5, 7)),        # vec4, fewer rows than a pass
          (2, 6, (1, 9, 11)),        # scalar path, CG = 6 does not divide 256
          (1, 128, (1, 9, 7)),       # R = 8
          (3, 4, (1, 40, 36))]       # several chunks, with a partly filled last one


def _inputs(n, c, sp):
    gen = torch.Generator().manual_seed(100 * c + n)
    grid = lambda: torch.randint(-24, 25, (n, c, *sp), generator=gen).float() / 8
    z, zp, g = grid(), grid(), grid()
    pick = lambda: torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c,), generator=gen)]
    quarter = lambda: torch.randint(-4, 5, (c,), generator=gen).float() / 4
    scale, shift, pscale, pshift = pick(), quarter(), pick(), quarter()
    mean, invstd = torch.rand(c, generator=gen) - 0.5, torch.rand(c, generator=gen) + 0.5
    return z, zp, g, scale, shift, mean, invstd, pscale, pshift


def _reference(z, zp, g, scale, shift, mean, invstd, pscale, pshift, coef):
    """fp64; returns dz, dgamma, dbeta and the three sign fields."""
    cz, cy, ca = coef
    v = lambda t: t.double().view(1, -1, 1, 1, 1)
    z, zp, g = z.double(), zp.double(), g.double()
    y, yp = z * v(scale) + v(shift), zp * v(pscale) + v(pshift)
    a, ap = torch.where(y < 0, y * SLOPE, y), torch.where(yp < 0, yp * SLOPE, yp)
    signs = (torch.sign(zp - z), torch.sign(yp - y), torch.sign(ap - a))
    ga = g - ca * signs[2]
    gy = torch.where(y < 0, ga * SLOPE, ga) - cy * signs[1]
    zhat = (z - v(mean)) * v(invstd)
    red = [0, 2, 3, 4]
    s1, s2 = gy.sum(red), (gy * zhat).sum(red)
    cnt = z.numel() // z.shape[1]
    dz = v(scale) * (gy - v(s1 / cnt) - zhat * v(s2 / cnt)) - cz * signs[0]
    return dz, s2, s1, signs


def _beyond_tolerance(got, want, rtol=1e-3):
    """The elements assert_close(got, want, rtol=rtol) would object to."""
    atol = 2e-5 * want.abs().max()
    return (got - want).abs() > atol + rtol * want.abs()


def _check_reference_can_fail(inp):
    """Every sign term is live on at least a quarter of the elements, and zeroing any one coefficient moves dz beyond the
    tolerance on at least a quarter of them: a kernel that dropped a term could not pass."""
    dz, _, _, signs = _reference(*inp, COEF)
    for name, s in zip(("z", "y", "a"), signs):
        assert (s != 0).double().mean() >= 0.25, name
    for k in range(3):
        coef = tuple(0.0 if j == k else COEF[j] for j in range(3))
        moved = _beyond_tolerance(_reference(*inp, coef)[0], dz)
        assert moved.double().mean() >= 0.25, (k, moved.double().mean().item())


@pytest.mark.parametrize("n,c,sp", SHAPES)
def test_reference_can_fail(n, c, sp):
    _check_reference_can_fail(_inputs(n, c, sp))


def _gpu(inp, coef):
    """reduce -> finalize -> apply; coef None: without a peer.  Returns dz (NCDHW, cpu), dgamma, dbeta, and the raw
    partials and dz for bit comparisons."""
    from mpgan_amd import ops
    z, zp, g, scale, shift, mean, invstd, pscale, pshift = inp
    n, c = z.shape[:2]
    P = z[0, 0].numel()
    z_cl, g_cl = to_cl(z), to_cl(g)
    pro = ops.Prologue(scale.cuda(), shift.cuda(), 0, ops.ACT_LEAKY, SLOPE)
    peer = None
    if coef is not None:
        peer = ops.PeerTaps(to_cl(zp), pscale.cuda(), pshift.cuda(), torch.tensor(coef, device="cuda"))
    mean_d, invstd_d = mean.cuda(), invstd.cuda()
    chunks = ops.stats_chunks(P, c)
    partials = torch.zeros(n * chunks * (3 * c + 1), device="cuda")
    ops.norm_bwd_reduce(g_cl, z_cl, pro, mean_d, invstd_d, partials, peer)
    dgamma, dbeta = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
    c1, c2 = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    ops.norm_bwd_finalize(partials, n, chunks, c, P, False, dgamma, dbeta, None, c1, c2)
    dz = torch.zeros_like(z_cl)
    ops.norm_bwd_apply(g_cl, z_cl, pro, mean_d, invstd_d, c1, c2, dz, peer)
    return from_cl(dz, 3), dgamma.cpu(), dbeta.cpu(), partials, dz


@pytest.mark.gpu
@pytest.mark.parametrize("n,c,sp", SHAPES)
def test_norm_backward_fp32_peer_taps(n, c, sp):
    inp = _inputs(n, c, sp)
    _check_reference_can_fail(inp)
    dz_ref, dgamma_ref, dbeta_ref, _ = _reference(*inp, COEF)
    dz, dgamma, dbeta, _, _ = _gpu(inp, COEF)
    assert_close(dz, dz_ref, rtol=1e-3, what="dz")
    assert_close(dgamma, dgamma_ref, rtol=1e-3, what="dgamma")
    assert_close(dbeta, dbeta_ref, rtol=1e-3, what="dbeta")
    # all coefficients zero: the peer call leaves the bits of the call without a peer
    zero, plain = _gpu(inp, (0.0, 0.0, 0.0)), _gpu(inp, None)
    assert torch.equal(zero[3], plain[3]), "partials"
    assert torch.equal(zero[4], plain[4]), "dz"
    # ... which is the formula without the peer terms
    dz0_ref, dgamma0_ref, dbeta0_ref, _ = _reference(*inp, (0.0, 0.0, 0.0))
    assert_close(plain[0], dz0_ref, rtol=1e-3, what="dz (no peer)")
    assert_close(plain[1], dgamma0_ref, rtol=1e-3, what="dgamma (no peer)")
    assert_close(plain[2], dbeta0_ref, rtol=1e-3, what="dbeta (no peer)")
