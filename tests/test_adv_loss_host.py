"""The logit-space adversarial objectives without a GPU: the float64 restatement of tests/adv_loss_ref.py against torch's
autograd, the fact that motivates them, the binding and host-side validation of mpgan_adv_loss, and the
Discriminator(output=...) constructor."""
import ctypes
import os
import re

import pytest
import torch

import adv_loss_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("n", [1, 3, 65, 1797])
def test_restatement_equals_torch_autograd(kind, n):
    z32, t32 = A.inputs(n)
    z, t = z32.double().requires_grad_(True), t32.double()
    want = A.torch_objective(kind, z, t)
    want.backward()
    want = want.detach()
    loss, grad = A.objective(kind, z.detach(), t)
    assert abs(float(loss) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert (grad - z.grad).abs().max().item() <= 1e-12
    assert torch.isfinite(grad).all()


def test_the_probability_chain_dies_where_the_logit_form_does_not():
    """Logit -90, target 1, one element: the Sigmoid underflows in float32, today's loss is pinned at the log clamp and
    its gradient is exactly zero; the logit form gives loss 90 and the full gradient -1/n."""
    z, t = torch.tensor([-90.0]), torch.tensor([1.0])
    loss, dlogit = A.prob_chain_f32(z, t)
    assert loss.dtype == torch.float32 and float(loss) == 100.0
    assert float(dlogit[0]) == 0.0
    loss, grad = A.objective("bce_logits", z.double(), t.double())
    assert float(loss) == 90.0
    assert float(grad[0]) == -1.0 / z.numel()
    # ... and above the underflow the two are the same loss (logit -20: p = 2.1e-9)
    z = torch.tensor([-20.0, 3.0, 0.5])
    t = torch.tensor([1.0, 0.9, 0.0])
    chain, _ = A.prob_chain_f32(z, t)
    stable, _ = A.objective("bce_logits", z.double(), t.double())
    assert abs(float(chain) - float(stable)) <= 1e-6 * float(stable)


def test_header_declares_and_binding_covers_the_new_symbols():
    from mpgan_amd import _lib
    text = open(os.path.join(ROOT, "include", "mpgan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("mpgan_adv_loss_partials", "mpgan_adv_loss"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"MPGAN_ADV_BCE_LOGITS\s*=\s*0\s*,\s*MPGAN_ADV_LSGAN\s*=\s*1", code)
    assert len(_lib.SIGNATURES["mpgan_adv_loss"][1]) == 8
    from mpgan_amd import ops
    assert ops.ADV_KINDS == {"bce_logits": 0, "lsgan": 1}


def test_adv_loss_refuses_bad_arguments_on_the_host():
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()
    assert lib.mpgan_abi_version() == 2
    buf = (ctypes.c_double * 8)()                     # a host address: every call below must return before any launch
    p = ctypes.addressof(buf)
    good = dict(logit=p, target=p, n=4, kind=0, partials=p, loss=p, grad=None)

    def call(**kw):
        a = dict(good, **kw)
        lib.mpgan_zero_bytes(None, 0, None)           # leaves another function's name in the error text
        assert b"adv_loss" not in lib.mpgan_last_error()
        return lib.mpgan_adv_loss(a["logit"], a["target"], a["n"], a["kind"], a["partials"], a["loss"], a["grad"], None)

    for bad in (dict(n=0), dict(n=-5), dict(kind=2), dict(kind=-1), dict(logit=None), dict(target=None),
                dict(partials=None), dict(loss=None)):
        assert call(**bad) == -1, bad
        assert b"mpgan_adv_loss" in lib.mpgan_last_error(), (bad, lib.mpgan_last_error())
    assert lib.mpgan_adv_loss_partials(1) == 1
    assert lib.mpgan_adv_loss_partials(1024) == 1 and lib.mpgan_adv_loss_partials(1025) == 2
    assert lib.mpgan_adv_loss_partials(70304) == 69
    assert lib.mpgan_adv_loss_partials(2 ** 31 - 1) == 1024          # the grid is capped: the blocks sweep again
    assert lib.mpgan_adv_loss_partials(0) == -1 and b"mpgan_adv_loss_partials" in lib.mpgan_last_error()


def test_discriminator_output_option_on_the_cpu():
    """Fails on a tree without the option: the constructor takes no `output`."""
    from mpgan_amd.networks import Discriminator
    for head, shape in (("linear", (1, 32, 32)), ("markovian", (1, 26, 34))):
        default = Discriminator(shape, dimensions=2, head=head)
        logit = Discriminator(shape, dimensions=2, head=head, output="logit")
        assert default.output == "prob" and logit.output == "logit"
        assert list(logit.state_dict()) == list(default.state_dict())
        assert [type(m).__name__ for m in logit.modules()] == [type(m).__name__ for m in default.modules()]
        assert not next(logit.parameters()).is_cuda
    with pytest.raises(ValueError, match="output"):
        Discriminator((1, 32, 32), dimensions=2, output="bogus")


def test_adversarial_loss_kind_is_validated():
    from mpgan_amd.gan import ADV_LOSSES, adversarial_loss
    assert ADV_LOSSES == ("bce", "bce_logits", "lsgan")
    with pytest.raises(ValueError, match="kind"):
        adversarial_loss(torch.zeros(2, 1), torch.zeros(2, 1), kind="hinge")


def test_ops_adv_loss_hands_no_host_tensor_to_a_kernel():
    from mpgan_amd import ops
    z, t = torch.zeros(4), torch.zeros(4)
    with pytest.raises(ValueError, match="GPU"):
        ops.adv_loss(z, t, "lsgan", torch.zeros(1, dtype=torch.float64), torch.zeros(()))
    with pytest.raises(ValueError, match="kind"):
        ops.adv_loss(z, t, "hinge", torch.zeros(1, dtype=torch.float64), torch.zeros(()))
