"""Eval-mode discriminators, the part that needs no GPU: the reference fixture (tests/golden/disc_eval.npz, written by
tools/make_eval_golden.py from the REFERENCE'S OWN Discriminator classes) against the oracle restatement, the new C
entries' host-side argument checks, and the bf16 emulation of the fused eval contract against its fp32 oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import refmodel as R
from oracle.make_golden import summarize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mpgan_conv_forward_act_bf16", "mpgan_conv_forward_act_f32_to_bf16")


@pytest.fixture
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "disc_eval.npz"))


@pytest.fixture
def eight_threads():
    """The recipe's thread count (tools/make_eval_golden.py), so that the bit-for-bit comparisons see its summation order."""
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _draw(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


def oracle_b_after_train_pass(fx):
    d = R.PatchDiscriminator((1, 16, 16, 16))
    R.closed_form_fill_(d)
    d.train()
    with torch.no_grad():
        d(torch.from_numpy(fx["b_x_train"]))
    return d.eval()


def test_fixture_inputs_follow_the_recipe(fx):
    g = torch.Generator().manual_seed(int(fx["b_seed"]))
    assert torch.equal(_draw(g, 4, 1, 16, 16, 16), torch.from_numpy(fx["b_x_train"]))
    assert torch.equal(_draw(g, 3, 1, 16, 16, 16), torch.from_numpy(fx["b_x_eval"]))
    assert int(fx["a_seed"]) == 22 and fx["a_validity"].shape == (1, 1)
    assert all(v.dtype.kind in "fiu" for v in fx.values())        # arrays of numbers only


def test_variant_b_oracle_reproduces_the_reference_fixture_bit_for_bit(fx, eight_threads):
    """Train pass + eval pass of oracle.refmodel.PatchDiscriminator: buffers, validity, logit and all 16 eval taps with
    max abs difference 0.0 against the reference's class, and the eval pass leaves every buffer unchanged."""
    d = oracle_b_after_train_pass(fx)
    for n, b in d.named_buffers():
        assert np.array_equal(b.numpy(), fx["b_buf__" + n]), n
    before = {n: b.clone() for n, b in d.named_buffers()}
    with torch.no_grad():
        val, taps = d(torch.from_numpy(fx["b_x_eval"]))
    assert all(torch.equal(before[n], b) for n, b in d.named_buffers())
    assert not d.training
    assert np.abs(val.numpy() - fx["b_validity"]).max() == 0.0
    assert np.abs(taps[14].double().numpy() - fx["b_logit"]).max() == 0.0
    assert sorted(taps) == list(range(16))
    for k, t in taps.items():
        assert tuple(t.shape) == tuple(fx[f"b_tap{k}_shape"]), k
        assert np.abs(summarize(t) - fx[f"b_tap{k}"]).max() == 0.0, k
    # nowhere near saturation: the comparisons of the GPU tests are meaningful
    assert 0.50 < fx["b_validity"].min() and fx["b_validity"].max() < 0.51


@pytest.mark.slow
def test_variant_a_oracle_reproduces_the_reference_fixture_bit_for_bit(fx, eight_threads):
    d = R.Discriminator((1, 128, 128, 128))
    R.closed_form_fill_(d)
    g = torch.Generator().manual_seed(int(fx["a_seed"]))
    x_train, x_eval = _draw(g, 1, 1, 128, 128, 128), _draw(g, 1, 1, 128, 128, 128)
    d.train()
    with torch.no_grad():
        v_train = d(x_train)
    assert np.abs(v_train.numpy() - fx["a_validity_train"]).max() == 0.0
    for n, b in d.named_buffers():
        assert np.array_equal(b.numpy(), fx["a_buf__" + n]), n
    d.eval()
    before = {n: b.clone() for n, b in d.named_buffers()}
    with torch.no_grad():
        v = d(x_eval)
    assert all(torch.equal(before[n], b) for n, b in d.named_buffers())
    assert np.abs(v.numpy() - fx["a_validity"]).max() == 0.0
    v64 = v.double()
    assert np.abs(torch.log(v64 / (1 - v64)).numpy() - fx["a_logit"]).max() == 0.0
    assert abs(fx["a_validity"].item() - 0.5223) < 1e-4 and abs(fx["a_validity_train"].item() - 0.5461) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# the new C entries
# ---------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_and_bound():
    from mpgan_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpgan_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES, name
    # one argument type per parameter of the header's declaration
    for name in NEW_ENTRIES:
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


def _geom(cin, cout):
    from mpgan_amd import _lib
    g = _lib.ConvGeomC()
    g.n, g.cin, g.cout = 1, cin, cout
    for d in range(3):
        g.in_dhw[d], g.out_dhw[d], g.k[d], g.stride[d], g.pad[d] = 10, 8, 3, 1, 0
    return g


def test_new_entries_are_exported_and_check_their_arguments_on_the_host():
    """Null pointers, bad pitches, misaligned vectors and a statistics request (fused statistics describe the raw conv
    output, which these launches never form) are rejected with -1 and a message naming the entry, before any launch
    (no GPU here)."""
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmpgan_hip.so not built (run __graft_entry__.build())")
    handle = C.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert hasattr(handle, name), name
    lib = _lib.lib()
    assert lib.mpgan_abi_version() == 2
    A = 4096                                      # a 16-byte aligned stand-in address: nothing is dereferenced on these paths
    g = _geom(64, 128)
    f = lib.mpgan_conv_forward_act_bf16
    short = b"conv_forward_act_bf16"
    #               x  ldx w  scale shift slope stats y  ldy  f32
    ok = [C.byref(g), A, 64, A, A, A, A, None, A, 128, 0, None]

    def call(fn, args, **change):
        a = list(args)
        for i, v in change.items():
            a[int(i[1:])] = v
        rc = fn(*a)
        return rc, lib.mpgan_last_error()

    for change in ({"_1": None}, {"_3": None}, {"_4": None}, {"_5": None}, {"_6": None}, {"_8": None}):
        rc, msg = call(f, ok, **change)
        assert rc == -1 and short in msg and b"null" in msg, (change, rc, msg)
    for change in ({"_2": 63}, {"_9": 127}):
        rc, msg = call(f, ok, **change)
        assert rc == -1 and short in msg and b"pitch" in msg, (change, rc, msg)
    for i in ("_4", "_5", "_6"):
        rc, msg = call(f, ok, **{i: A + 4})
        assert rc == -1 and short in msg and b"aligned" in msg, (i, rc, msg)
    rc, msg = call(f, ok, _7=A)
    assert rc == -1 and short in msg and b"statistics" in msg, (rc, msg)

    g1 = _geom(1, 64)
    f1 = lib.mpgan_conv_forward_act_f32_to_bf16
    short1 = b"conv_forward_act_f32_to_bf16"
    #                x  ldx w  scale shift slope stats y  ldy
    ok1 = [C.byref(g1), A, 1, A, A, A, A, None, A, 64, None]
    for change in ({"_1": None}, {"_3": None}, {"_4": None}, {"_5": None}, {"_6": None}, {"_8": None}):
        rc, msg = call(f1, ok1, **change)
        assert rc == -1 and short1 in msg and b"null" in msg, (change, rc, msg)
    for change in ({"_2": 0}, {"_9": 63}):
        rc, msg = call(f1, ok1, **change)
        assert rc == -1 and short1 in msg and b"pitch" in msg, (change, rc, msg)
    for i in ("_4", "_5", "_6"):
        rc, msg = call(f1, ok1, **{i: A + 8})
        assert rc == -1 and short1 in msg and b"aligned" in msg, (i, rc, msg)
    rc, msg = call(f1, ok1, _7=A)
    assert rc == -1 and short1 in msg and b"statistics" in msg, (rc, msg)
    g2 = _geom(64, 64)                             # more than one input channel: not this entry's layer
    rc, msg = call(f1, [C.byref(g2)] + ok1[1:], _2=64)
    assert rc == -2 and short1 in msg, (rc, msg)


# ---------------------------------------------------------------------------------------------------------------------
# the fused bf16 contract, emulated, against its fp32 oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_emulated_bf16_eval_stays_within_the_bf16_bound_of_the_oracle_variant_b(fx):
    """tests/disc_eval_ref.py on the fixture's variant-B inputs: validity within the train-mode bf16 bound (2e-2) of the
    fp32 oracle and of the reference fixture, for the fused and for the tap-keeping program; the two programs differ
    (one rounding per layer against two) and the eval pass writes nothing."""
    from disc_eval_ref import disc_eval_bf16
    d = oracle_b_after_train_pass(fx)
    x = torch.from_numpy(fx["b_x_eval"])
    before = {n: b.clone() for n, b in d.named_buffers()}
    with torch.no_grad():
        want, taps = d(x)
    out = {}
    for fused in (True, False):
        got = disc_eval_bf16(d, x, fused=fused)
        out[fused] = got
        dv = (got["validity"] - want).abs().max().item()
        dl = (got["logit"] - taps[14]).abs().max().item()
        print(f"emulated bf16 eval (fused={fused}): |validity - fp32| {dv:.3e}  |logit - fp32| {dl:.3e}")
        np.testing.assert_allclose(got["validity"].numpy(), want.numpy(), rtol=0, atol=2e-2)
        np.testing.assert_allclose(got["validity"].numpy(), fx["b_validity"], rtol=0, atol=2e-2)
        assert [tuple(a.shape) for a in got["acts"]] == [tuple(taps[3 * i + 2].shape) for i in range(4)]
        for a in got["acts"][:3]:
            assert torch.equal(a, a.to(torch.bfloat16).float())           # stored as bf16
    assert not torch.equal(out[True]["acts"][1], out[False]["acts"][1])
    assert all(torch.equal(before[n], b) for n, b in d.named_buffers())


@pytest.mark.slow
def test_emulated_bf16_eval_stays_within_the_bf16_bound_of_the_oracle_variant_a(fx):
    from disc_eval_ref import disc_eval_bf16
    d = R.Discriminator((1, 128, 128, 128))
    R.closed_form_fill_(d)
    sd = d.state_dict()
    for n in list(sd):
        if "a_buf__" + n in fx:
            sd[n] = torch.from_numpy(fx["a_buf__" + n])
    d.load_state_dict(sd)
    d.eval()
    g = torch.Generator().manual_seed(int(fx["a_seed"]))
    _draw(g, 1, 1, 128, 128, 128)
    x = _draw(g, 1, 1, 128, 128, 128)
    got = disc_eval_bf16(d, x, fused=True)
    print("emulated bf16 eval, A at 128^3: validity", got["validity"].item(), "fixture", fx["a_validity"].item())
    np.testing.assert_allclose(got["validity"].numpy(), fx["a_validity"], rtol=0, atol=2e-2)
