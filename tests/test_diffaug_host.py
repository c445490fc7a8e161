"""Differentiable augmentation, everything that needs no GPU: the float64 restatement against autograd and against the
paper's own pad / clamp / gather / mask arithmetic, the sampler on the CPU, the trainer option's defaults, and the
library's host-side refusals."""
import ctypes
import os

import pytest
import torch

import diffaug_ref as R


# ---- the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES[:2] + R.SHAPES_3D[:2], ids=str)
def test_closed_form_backward_equals_autograd(shape):
    gen = torch.Generator().manual_seed(3)
    for name, color, geom in R.param_sets(shape):
        for ops in (R.ALL, R.COLOR | R.TRANSLATION, R.CONTRAST | R.CUTOUT, R.TRANSLATION | R.CUTOUT, R.BRIGHTNESS):
            x = R.make_input(shape).double().requires_grad_(True)
            y = R.forward(x, color, geom, ops, fill=0.25)
            gy = torch.rand(*shape, generator=gen, dtype=torch.float64) - 0.4
            y.backward(gy)
            gx, _, _ = R.backward(gy, color, geom, ops)
            assert (gx - x.grad).abs().max().item() <= 1e-12, (name, ops)


def test_hand_rows_cover_the_edge_cases():
    for shape in R.SHAPES:
        S = R.dhw(shape)
        x = torch.ones(shape, dtype=torch.float64)
        kept = {}
        for name, color, geom in R.param_sets(shape):
            y = R.forward(x, color, geom, R.TRANSLATION | R.CUTOUT, fill=-7.0)
            for s in range(shape[0]):
                kept[tuple(geom[s].tolist())] = int((y[s] == 1).sum())
        n = S[0] * S[1] * S[2]
        assert 0 in kept.values() and n in kept.values() and any(0 < v < n for v in kept.values()), shape


@pytest.mark.parametrize("shape", R.SHAPES_2D + [(4, 1, 16, 12)], ids=str)
def test_2d_restatement_equals_the_papers_arithmetic(shape):
    """fill = 0, float64: translation and cutout of the restatement against the paper's pad-clamp-gather and its clamped
    mask grid, on the colour stage's output, compared with torch.equal (the paper multiplies by a zero mask, so a cut
    negative value is -0.0 there and +0.0 here: equal as values, the one bit pattern that may differ).  Also: for
    sampled parameters the paper's clamped cutout grid is the clipped box, because the box always meets the image."""
    from mpgan_amd.augment import sample_params
    B, _, H, W = shape
    gen = torch.Generator().manual_seed(21)
    for trial in range(20):
        p = sample_params(B, (H, W), "color,translation,cutout", generator=gen)
        x = R.make_input(shape, seed=trial).double()
        u = R.forward(x, p.color, p.geom, R.COLOR)
        want = R.paper_translation(u, p.geom[:, 1].long(), p.geom[:, 2].long())
        size = (int(p.geom[0, 7]), int(p.geom[0, 8]))
        assert size == (int(H * 0.5 + 0.5), int(W * 0.5 + 0.5))
        offset = (p.geom[:, 4].long() + size[0] // 2, p.geom[:, 5].long() + size[1] // 2)   # the paper's draw: lo = o - size//2
        for k, s in ((0, H), (1, W)):       # the box meets the image on each axis
            lo = offset[k] - size[k] // 2
            assert bool(((lo < s) & (lo + size[k] > 0)).all())
        want = R.paper_cutout(want, offset[0], offset[1], size)
        got = R.forward(x, p.color, p.geom, R.ALL, fill=0.0)
        assert torch.equal(got, want), trial
        # each stage alone
        assert torch.equal(R.forward(x, p.color, p.geom, R.TRANSLATION),
                           R.paper_translation(x, p.geom[:, 1].long(), p.geom[:, 2].long()))
        assert torch.equal(R.forward(x, p.color, p.geom, R.CUTOUT), R.paper_cutout(x, offset[0], offset[1], size))


# ---- the sampler ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial", [(33, 65), (8, 8), (5, 7), (20, 33, 35), (4, 5, 6), (128, 128, 128)], ids=str)
def test_sample_params_on_the_cpu(spatial):
    from mpgan_amd import augment as A
    n = 512
    gen = torch.Generator().manual_seed(9)
    p = A.sample_params(n, spatial, "color,translation,cutout", generator=gen)
    assert p.ops == 15
    assert p.color.dtype == torch.float32 and p.color.shape == (n, 2) and p.color.is_contiguous()
    assert p.geom.dtype == torch.int32 and p.geom.shape == (n, 9) and p.geom.is_contiguous()
    b, c = p.color[:, 0], p.color[:, 1]
    assert float(b.min()) >= -0.5 and float(b.max()) < 0.5 and float(c.min()) >= 0.5 and float(c.max()) < 1.5
    assert float(b.max() - b.min()) > 0.8 and float(c.max() - c.min()) > 0.8
    first = 3 - len(spatial)
    if first:
        assert p.geom[:, [0, 3, 6]].tolist() == [[0, 0, 1]] * n
    for k, s in enumerate(spatial, first):
        r, size = int(s / 8 + 0.5), int(s / 2 + 0.5)
        t, lo, sz = p.geom[:, k], p.geom[:, 3 + k], p.geom[:, 6 + k]
        assert int(t.min()) >= -r and int(t.max()) <= r
        assert set(t.tolist()) == set(range(-r, r + 1)) or n < 40 * (2 * r + 1)
        assert bool((sz == size).all())
        o = lo + size // 2
        assert int(o.min()) >= 0 and int(o.max()) <= s - 1 + (1 - size % 2)
        assert bool(((lo < s) & (lo + size > 0)).all())            # the box always meets the image
    again = A.sample_params(n, spatial, "color,translation,cutout", generator=torch.Generator().manual_seed(9))
    assert torch.equal(again.color, p.color) and torch.equal(again.geom, p.geom)
    other = A.sample_params(n, spatial, "color,translation,cutout", generator=gen)      # the generator has moved on
    assert not torch.equal(other.color, p.color)


def test_sample_params_policies():
    from mpgan_amd import augment as A
    gen = torch.Generator().manual_seed(1)
    p = A.sample_params(6, (16, 16), "translation", generator=gen)
    assert p.ops == A.TRANSLATION and p.color.tolist() == [[0.0, 1.0]] * 6 and p.geom[:, 3:].tolist() == [[0, 0, 0, 1, 0, 0]] * 6
    p = A.sample_params(6, (8, 16, 16), " cutout , color ", generator=gen)
    assert p.ops == A.CUTOUT | A.BRIGHTNESS | A.CONTRAST and p.geom[:, :3].tolist() == [[0, 0, 0]] * 6
    assert p.geom[:, 6:].tolist() == [[4, 8, 8]] * 6
    assert A.sample_params(2, (8, 8), "", generator=gen).ops == 0
    # the draw order that replays rely on: color, then translation, then cutout
    g1, g2 = torch.Generator().manual_seed(4), torch.Generator().manual_seed(4)
    full = A.sample_params(5, (16, 24), "cutout,translation,color", generator=g1)
    assert torch.equal(A.sample_params(5, (16, 24), "color", generator=g2).color, full.color)
    assert torch.equal(A.sample_params(5, (16, 24), "translation", generator=g2).geom[:, :3], full.geom[:, :3])
    assert torch.equal(A.sample_params(5, (16, 24), "cutout", generator=g2).geom[:, 3:], full.geom[:, 3:])
    for bad in ("colour", "color,flip", "translation cutout"):
        with pytest.raises(ValueError, match="policy"):
            A.sample_params(2, (8, 8), bad)
    with pytest.raises(ValueError):
        A.sample_params(2, (8,), "color")
    assert A.parse_policy("color,translation,cutout") == 15 and A.parse_policy("") == 0


# ---- the trainer option ---------------------------------------------------------------------------------------------
def test_trainer_defaults_and_hparams():
    from mpgan_amd.augment import DiffAugment
    from mpgan_amd.gan import GAN
    g = GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu")
    assert g.hparams.diff_augment == "" and g.hparams.diff_augment_fill == 0.0
    assert "diff_augment" not in vars(g.hparams) and "diff_augment_fill" not in vars(g.hparams)
    assert g.augment is None and g.aug_generator is None
    assert not any(isinstance(m, DiffAugment) for m in g.modules())
    keys = list(g.state_dict())
    a = GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu", diff_augment="color,cutout", diff_augment_fill=-1.0)
    assert vars(a.hparams)["diff_augment"] == "color,cutout" and vars(a.hparams)["diff_augment_fill"] == -1.0
    assert isinstance(a.augment, DiffAugment) and a.augment.ops == 11 and a.augment.fill == -1.0
    assert list(a.state_dict()) == keys                              # no parameter, no buffer
    assert a.aug_generator is None
    for bad in ("colour", "color,rotation"):
        with pytest.raises(ValueError, match="policy"):
            GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu", diff_augment=bad)


def test_there_is_no_cpu_path():
    from mpgan_amd import augment as A
    p = A.sample_params(2, (8, 8), "translation")
    with pytest.raises(ValueError, match="GPU"):
        A.diff_augment(torch.zeros(2, 1, 8, 8), p)


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def _lib():
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_host_side_refusals_happen_before_any_launch():
    """As test_capi_symbols.py::test_error_reporting_without_gpu: the pointers are never dereferenced on these paths."""
    lib = _lib()
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)
    p = 4096                                                           # any 16-byte aligned non-null address
    ok = i3(1, 8, 8)
    need = lib.mpgan_diffaug_workspace(2, ok)
    assert need == 2 * 8                                               # one block per 64-element sample
    assert lib.mpgan_diffaug_workspace(4, i3(128, 128, 128)) == 4 * 512 * 8
    assert lib.mpgan_diffaug_workspace(16, i3(1, 256, 256)) == 16 * 64 * 8

    def fwd(x=p, n=2, dhw=ok, ops=15, color=p, geom=p, ws=p, ws_bytes=need, y=p):
        return lib.mpgan_diffaug_forward(x, n, dhw, ops, color, geom, 0.0, ws, ws_bytes, y, None)

    def bwd(gy=p, n=2, dhw=ok, ops=15, color=p, geom=p, ws=p, ws_bytes=need, gx=p):
        return lib.mpgan_diffaug_backward(gy, n, dhw, ops, color, geom, ws, ws_bytes, gx, None)

    for call, name in ((fwd, b"mpgan_diffaug_forward"), (bwd, b"mpgan_diffaug_backward")):
        first, last = ("x", "y") if call is fwd else ("gy", "gx")
        cases = [({first: None}, b"null"), ({last: None}, b"null"), ({"dhw": None}, b"null"),
                 ({"color": None}, b"null"), ({"geom": None}, b"null"), ({"ws": None}, b"null"),
                 ({"n": 0}, b"n = 0"), ({"n": -3}, b"n = -3"),
                 ({"dhw": i3(0, 8, 8)}, b"extent"), ({"dhw": i3(1, 8, -1)}, b"extent"),
                 ({"ops": 16}, b"ops"), ({"ops": 15 | 64}, b"ops"), ({"ops": -1}, b"ops"),
                 ({"ws_bytes": need - 1}, b"workspace"), ({"ws": p + 4}, b"aligned"),
                 ({"n": 1024, "dhw": i3(128, 128, 128), "ws_bytes": 1 << 40}, b"32-bit"),
                 ({"n": 1, "dhw": i3(2048, 1024, 1024), "ws_bytes": 1 << 40}, b"32-bit")]
        for kw, word in cases:
            assert call(**kw) == -1, kw
            msg = lib.mpgan_last_error()
            assert name in msg and word in msg, (kw, msg)
    assert lib.mpgan_diffaug_workspace(0, ok) == -1 and b"diffaug_workspace" in lib.mpgan_last_error()
    assert lib.mpgan_diffaug_workspace(2, i3(1, 0, 8)) == -1 and b"extent" in lib.mpgan_last_error()
    assert lib.mpgan_diffaug_workspace(2, None) == -1
    assert lib.mpgan_diffaug_workspace(2048, i3(128, 128, 128)) == -1 and b"32-bit" in lib.mpgan_last_error()
    assert lib.mpgan_abi_version() == 2
