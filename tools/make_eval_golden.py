"""Generate tests/golden/disc_eval.npz: the REFERENCE'S OWN discriminators (variants A and B) in eval mode, on the CPU.

Run where oracle/make_golden.py runs (it needs the reference checkout that script names; the GPU box never sees it):
    python tools/make_eval_golden.py

Both reference `Discriminator` classes are pure torch and execute under the stubs of oracle/make_golden.py.  Each gets
closed-form weights (oracle.refmodel.closed_form_fill_), ONE train-mode pass (so that the running statistics are not the
trivial (0, 1)), then `.eval()` and a pass on fresh input.  The fixture holds arrays only:
  B (16^3 patches): both inputs, every buffer after the train pass in full, the eval validity, the 16 eval taps as
     (summary, shape) and the logit (tap 14) in full;
  A (128^3): the seed of its inputs, every buffer after the train pass in full (so a GPU test needs no CPU pass at
     128^3), the eval validity and its logit log(v / (1 - v)) in float64.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import OUT, REF, _install_stubs, _load, summarize  # noqa: E402
from oracle.refmodel import closed_form_fill_  # noqa: E402

SEED_B, SEED_A = 21, 22


def draw(gen, *shape):
    return torch.rand(*shape, generator=gen) * 2 - 1


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    _install_stubs()
    ref_a = _load(os.path.join(REF, "code/GAN/GAN_final.py"), "ref_gan_final")
    ref_b = _load(os.path.join(REF, "test_runs/GAN.py"), "ref_gan_b")
    fx = {}

    # ---- variant B: train pass on (4,1,16^3), eval pass on the next (3,1,16^3) of the same stream ----
    dB = ref_b.Discriminator((1, 16, 16, 16))
    closed_form_fill_(dB)
    g = torch.Generator().manual_seed(SEED_B)
    x_train, x_eval = draw(g, 4, 1, 16, 16, 16), draw(g, 3, 1, 16, 16, 16)
    dB.train()
    with torch.no_grad():
        dB(x_train)
    dB.eval()
    before = {n: b.clone() for n, b in dB.named_buffers()}
    with torch.no_grad():
        val, taps = dB(x_eval)
    assert all(torch.equal(before[n], b) for n, b in dB.named_buffers()), "the eval pass wrote a buffer"
    fx.update(b_seed=np.array(SEED_B), b_x_train=x_train.numpy(), b_x_eval=x_eval.numpy(), b_validity=val.numpy())
    for n, b in dB.named_buffers():
        fx["b_buf__" + n] = b.numpy()
    for k, t in taps.items():
        fx[f"b_tap{k}"] = summarize(t)
        fx[f"b_tap{k}_shape"] = np.array(t.shape)
    fx["b_logit"] = taps[14].double().numpy()

    # ---- variant A at 128^3: train pass on the seed's first draw, eval pass on the next ----
    dA = ref_a.Discriminator((1, 128, 128, 128))
    closed_form_fill_(dA)
    g = torch.Generator().manual_seed(SEED_A)
    xa_train, xa_eval = draw(g, 1, 1, 128, 128, 128), draw(g, 1, 1, 128, 128, 128)
    dA.train()
    with torch.no_grad():
        v_train = dA(xa_train)
    dA.eval()
    with torch.no_grad():
        vA = dA(xa_eval)
        logit = dA.model_linear[1](dA.model_linear[0](dA.model_conv(xa_eval))).double()
    v64 = vA.double()
    fx.update(a_seed=np.array(SEED_A), a_validity_train=v_train.numpy(), a_validity=vA.numpy(),
              a_logit=torch.log(v64 / (1 - v64)).numpy(), a_logit_linear=logit.numpy())
    for n, b in dA.named_buffers():
        fx["a_buf__" + n] = b.numpy()

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "disc_eval.npz")
    np.savez_compressed(path, **fx)
    print("B eval validity", val.flatten().tolist(), "logit", taps[14].flatten().tolist())
    print("A train validity", v_train.item(), "eval validity", vA.item())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
