"""Variant A's Markovian (PatchGAN) head, everything that needs no GPU: the module's constructor and state_dict, the
trainer option, the flat store, the restatement's closed forms against autograd, and the library's host-side refusals."""
import ctypes
import os

import pytest
import torch

import map_head_ref as M


def _disc(*a, **k):
    from mpgan_amd.networks import Discriminator
    return Discriminator(*a, **k)


def _count(m):
    return sum(p.numel() for p in m.parameters())


def test_constructor_state_dict_and_parameter_counts():
    d3 = _disc((1, 128, 128, 128), dimensions=3, head="markovian")
    assert _count(d3) == 6_532_865 == 6_516_480 + 16_385
    d2 = _disc((1, 256, 256), dimensions=2, head="markovian")
    assert _count(d2) == 1_653_377 == 1_649_280 + 4_097
    for d, dims in ((d3, 3), (d2, 2)):
        assert d.head == "markovian" and not hasattr(d, "model_linear")
        conv, sig = d.model_head
        assert isinstance(conv, {2: torch.nn.Conv2d, 3: torch.nn.Conv3d}[dims]) and isinstance(sig, torch.nn.Sigmoid)
        assert (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding) == \
            (256, 1, (4,) * dims, (1,) * dims, (0,) * dims) and conv.bias is not None
        keys = set(d.state_dict())
        assert {"model_head.0.weight", "model_head.0.bias"} <= keys
        assert not any(k.startswith("model_linear") for k in keys)
        # the restatement carries the same keys and shapes: state_dicts load both ways
        ref = M.MarkovianDiscriminator(dims)
        assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == \
            {k: tuple(v.shape) for k, v in d.state_dict().items()}
        d.load_state_dict(ref.state_dict())


def test_disc_map_size():
    from mpgan_amd.networks import disc_feature_sizes, disc_map_size
    assert disc_map_size((128, 128, 128)) == (26, 26, 26)
    assert disc_map_size((256, 256)) == (58, 58)
    assert disc_map_size((26, 34)) == (1, 3) and disc_feature_sizes((26, 34))[-1] == (4, 6)
    assert disc_map_size((26, 26, 30)) == (1, 1, 2)
    d = _disc((1, 26, 34), dimensions=2, head="markovian")
    assert d.validity_shape(2, (26, 34)) == (2, 1, 1, 3)
    assert _disc((1, 32, 32), dimensions=2).validity_shape(5, (32, 32)) == (5, 1)


def test_value_errors():
    with pytest.raises(ValueError, match="head"):
        _disc((1, 64, 64), dimensions=2, head="patch")
    with pytest.raises(ValueError, match="26"):
        _disc((1, 25, 64), dimensions=2, head="markovian")            # last feature map 3 x ...
    with pytest.raises(ValueError):
        _disc((1, 64, 64, 24), dimensions=3, head="markovian")
    _disc((1, 26, 26), dimensions=2, head="markovian")                 # the smallest input side
    _disc((1, 25, 64), dimensions=2)                                   # the Linear head keeps its own, lower limit


def test_defaults_are_unchanged():
    from mpgan_amd.gan import GAN
    from oracle import refmodel as R
    d = _disc((1, 32, 40), dimensions=2)
    assert d.head == "linear" and not hasattr(d, "model_head")
    ref = R.Discriminator((1, 32, 40), dimensions=2)
    assert list(d.state_dict()) == list(ref.state_dict())
    assert {k: tuple(v.shape) for k, v in d.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert _count(_disc((1, 128, 128, 128), dimensions=3)) == 12_760_065
    g = GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu")
    rg = R.GAN((1, 32, 40), dimensions=2, n_unet_blocks=1)
    assert list(g.state_dict()) == list(rg.state_dict())
    hp = vars(g.hparams)
    assert hp == dict(latent_dim=100, g_lr=0.0005, d_lr=0.0005, b1=0.5, b2=0.999, batch_size=64,
                      one_sided_label_value=0.9, d_head="linear")
    m = GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu", d_head="markovian")
    assert m.hparams.d_head == "markovian" and m.discriminator.head == "markovian"
    assert "discriminator.model_head.0.weight" in m.state_dict()
    with pytest.raises(ValueError):
        GAN(1, 32, 40, dimensions=2, n_unet_blocks=1, device="cpu", d_head="nope")


def test_variant_b_does_not_take_the_option():
    from mpgan_amd.networks import PatchDiscriminator
    with pytest.raises(TypeError):
        PatchDiscriminator((1, 16, 16), dimensions=2, head="markovian")


@pytest.mark.parametrize("dims", [2, 3])
def test_flat_store_registers_the_head(dims):
    from mpgan_amd.engine import ParamStore
    d = _disc((1,) + (26,) * dims, dimensions=dims, head="markovian")
    store = ParamStore(d)
    d._register_extra(store)
    names = {id(p): n for n, p in d.named_parameters()}
    recs = {names[id(r.mod.weight)]: r for r in store.convs}
    assert set(recs) == {f"model_conv.{i}.weight" for i in (0, 3, 6, 9)} | {"model_head.0.weight"}
    r = recs["model_head.0.weight"]
    assert (r.cout, r.cin, r.taps, r.transposed) == (1, 256, 4 ** dims, False)
    w = d.model_head[0].weight
    o = store.offset(w)
    assert o % 4 == 0 and r.fwd_off % 4 == 0
    assert w.data_ptr() == store.flat.data_ptr() + 4 * o               # a view of the flat buffer
    assert w.grad.data_ptr() == store.flat_grad.data_ptr() + 4 * o    # ... and of the flat gradient (Adam, all-reduce)


@pytest.mark.parametrize("dims,shape,per_sample", [(2, (3, 8, 9, 7), False), (3, (2, 8, 4, 5, 6), False),
                                                   (3, (2, 4, 6, 6, 6), True)])
def test_closed_forms_equal_autograd(dims, shape, per_sample):
    gen = torch.Generator().manual_seed(11)
    n, c = shape[:2]
    z = torch.rand(*shape, generator=gen, dtype=torch.float64) - 0.5
    sv = (n, c) if per_sample else (c,)
    sc, sh = torch.rand(*sv, generator=gen, dtype=torch.float64) + 0.5, torch.rand(*sv, generator=gen, dtype=torch.float64) - 0.5
    a = M.activate(z, sc, sh).requires_grad_(True)
    w = (torch.rand(1, c, *(4,) * dims, generator=gen, dtype=torch.float64) - 0.5).requires_grad_(True)
    b = torch.rand(1, generator=gen, dtype=torch.float64).requires_grad_(True)
    logit, prob = M.head_forward(a, w, b)
    assert logit.shape == (n, 1) + tuple(s - 3 for s in shape[2:])
    dl = torch.rand(*logit.shape, generator=gen, dtype=torch.float64) - 0.5
    logit.backward(dl)
    g_a, dw, db = M.head_backward(a.detach(), w.detach(), dl)
    for got, want in ((g_a, a.grad), (dw, w.grad), (db, b.grad)):
        assert (got - want).abs().max().item() <= 1e-12
    assert (prob - 1 / (1 + torch.exp(-logit))).abs().max().item() <= 1e-15


def _lib():
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.lib()


def test_host_side_refusals_happen_before_any_launch():
    """As test_error_reporting_without_gpu: the pointers are never dereferenced on these paths."""
    lib = _lib()
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)
    p = 4096                                                           # any 16-byte aligned non-null address
    ok_in, k = i3(1, 9, 7), i3(1, 4, 4)
    # c % 4 != 0
    assert lib.mpgan_maphead_forward(p, None, 2, ok_in, 6, k, p, p, p, None, None) < 0
    assert b"maphead" in lib.mpgan_last_error()
    assert lib.mpgan_maphead_backward(p, None, 2, ok_in, 6, k, p, p, p, None, None, 0.0, None, 0, None) < 0
    assert b"maphead" in lib.mpgan_last_error()
    assert lib.mpgan_maphead_workspace(2, ok_in, 6, k) < 0 and b"maphead" in lib.mpgan_last_error()
    # in < k
    assert lib.mpgan_maphead_forward(p, None, 2, i3(1, 3, 8), 64, k, p, p, p, None, None) < 0
    assert b"maphead" in lib.mpgan_last_error() and b"smaller" in lib.mpgan_last_error()
    assert lib.mpgan_maphead_backward(p, None, 2, i3(1, 9, 3), 64, k, p, p, p, None, None, 0.0, None, 0, None) < 0
    assert b"maphead" in lib.mpgan_last_error()
    # a workspace that is too small (needed for dw only)
    need = lib.mpgan_maphead_workspace(2, ok_in, 64, k)
    assert need >= 16 * 64 * 4
    assert lib.mpgan_maphead_backward(p, None, 2, ok_in, 64, k, p, p, None, p, None, 0.0, p, need - 4, None) < 0
    assert b"maphead" in lib.mpgan_last_error() and b"workspace" in lib.mpgan_last_error()
    assert lib.mpgan_maphead_backward(p, None, 2, ok_in, 64, k, p, p, None, p, None, 0.0, None, 0, None) < 0
    # misalignment, and taps*c beyond the LDS budget of the weights
    assert lib.mpgan_maphead_forward(p + 4, None, 2, ok_in, 64, k, p, p, p, None, None) < 0
    assert b"maphead" in lib.mpgan_last_error() and b"align" in lib.mpgan_last_error()
    assert lib.mpgan_maphead_forward(p, None, 2, i3(4, 9, 7), 512, i3(4, 4, 4), p, p, p, None, None) < 0
    assert b"maphead" in lib.mpgan_last_error() and b"LDS" in lib.mpgan_last_error()
    assert lib.mpgan_abi_version() == 2
