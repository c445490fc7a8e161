"""mpgan_amd.inference on the MI355X: the HIP gather / count / blend / finalize kernels against the CPU
restatement of MONAI 0.4.0 sliding_window_inference (sliding_window_ref.py), bit for bit.  Every predictor call's
input and output is recorded; the restatement is replayed on the recorded outputs."""
import pytest
import torch

import sliding_window_ref as ref
from mpgan_amd import inference as inf
from sw_helpers import Recorder, noisy as _noisy

pytestmark = pytest.mark.gpu


def _check(x, roi, sw, overlap, mode, cout=1, cval=0.0, seed=0):
    rec = Recorder(_noisy(cout, seed))
    got = inf.sliding_window_inference(x, roi, sw, rec, overlap=overlap, mode=mode, cval=cval)
    torch.cuda.synchronize()
    want, batches = ref.sliding_window(x.cpu(), roi, sw, rec.replay(), overlap=overlap, mode=mode, cval=cval)
    assert len(batches) == len(rec.inputs)
    for i, (a, b) in enumerate(zip(rec.inputs, batches)):
        assert a.shape == b.shape and torch.equal(a, b), f"window batch {i} differs from the padded slices"
    assert got.shape == want.shape
    assert torch.equal(got.cpu(), want), f"max |diff| {(got.cpu() - want).abs().max().item():.3e}"
    return got


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("overlap", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("sw", [1, 3, 8])
def test_bit_exact_3d_noncubic(sw, overlap, mode):
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(1, 1, 150, 200, 130, generator=g) * 2 - 1).cuda()
    _check(x, (64, 64, 64), sw, overlap, mode, seed=sw)


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_bit_exact_batch2_two_output_channels(mode):
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(2, 1, 96, 80, 72, generator=g) * 2 - 1).cuda()
    _check(x, (48, 48, 48), 5, 0.25, mode, cout=2)         # calls straddle the two images


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_bit_exact_2d(mode):
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(2, 1, 300, 260, generator=g) * 2 - 1).cuda()
    _check(x, (128, 128), 4, 0.25, mode)


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_bit_exact_image_smaller_than_roi(mode):
    g = torch.Generator().manual_seed(10)
    x = (torch.rand(1, 1, 50, 80, 70, generator=g) * 2 - 1).cuda()    # D < roi: padded with cval; W start 6
    _check(x, (64, 64, 64), 2, 0.25, mode, cval=-0.75)


def test_two_runs_identical():
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(1, 1, 150, 200, 130, generator=g) * 2 - 1).cuda()
    a = inf.sliding_window_inference(x, (64, 64, 64), 3, _noisy(1, 3), overlap=0.5, mode="gaussian")
    b = inf.sliding_window_inference(x, (64, 64, 64), 3, _noisy(1, 3), overlap=0.5, mode="gaussian")
    assert torch.equal(a, b)


def test_image_equal_to_roi_returns_predictor_output():
    g = torch.Generator().manual_seed(12)
    x = (torch.rand(2, 1, 64, 64, 64, generator=g) * 2 - 1).cuda()
    rec = Recorder(_noisy(2, 4))
    y = inf.SlidingWindowInferer((64, 64, 64), sw_batch_size=2)(x, rec)
    assert len(rec.outputs) == 1 and torch.equal(y.cpu(), rec.outputs[0])


def test_device_importance_map_is_the_restated_one():
    m = inf._device_importance((64, 64, 64), "gaussian", 0.125, torch.device("cuda", torch.cuda.current_device()))
    assert torch.equal(m.cpu(), ref.compute_importance_map((64, 64, 64), "gaussian", 0.125))


def test_predictor_output_is_validated():
    x = torch.rand(1, 1, 40, 40, 40, device="cuda")
    with pytest.raises(ValueError, match="predictor"):
        inf.sliding_window_inference(x, (32, 32, 32), 2, lambda w: w[:, :, :16])            # spatial shape
    with pytest.raises(ValueError, match="predictor"):
        inf.sliding_window_inference(x, (32, 32, 32), 2, lambda w: torch.cat([w, w]))       # batch
    with pytest.raises(ValueError, match="predictor"):
        inf.sliding_window_inference(x, (32, 32, 32), 2, lambda w: w.double())              # dtype
    with pytest.raises(ValueError, match="predictor"):
        inf.sliding_window_inference(x, (32, 32, 32), 2, lambda w: w.cpu())                 # device
    with pytest.raises(ValueError, match="device"):
        inf.sliding_window_inference(x, (32, 32, 32), 2, lambda w: w, device="cpu")
    y = inf.sliding_window_inference(x, (32, 32, 32), 2, lambda w: w, device="cuda", sw_device=x.device)
    torch.testing.assert_close(y, x, rtol=0, atol=1e-6)     # identity predictor, constant weights: the input back


def _generator():
    from mpgan_amd.networks import CasNetGenerator
    torch.manual_seed(0)
    gen = CasNetGenerator((1, 128, 128, 128), 6, dimensions=3, device="cuda")
    g = torch.Generator().manual_seed(13)
    warm = (torch.rand(1, 1, 128, 128, 128, generator=g) * 2 - 1).cuda()
    gen.train()
    with torch.no_grad():
        gen(warm)                       # running statistics away from their initial values
    gen.eval()
    return gen


def test_generator_bit_exact_against_restatement():
    gen = _generator()
    g = torch.Generator().manual_seed(14)
    x = (torch.rand(1, 1, 160, 160, 144, generator=g) * 2 - 1).cuda()
    for mode in ("constant", "gaussian"):
        rec = Recorder(gen)
        with torch.no_grad():
            got = inf.sliding_window_inference(x, (128, 128, 128), 4, rec, overlap=0.25, mode=mode)
        torch.cuda.synchronize()
        want, batches = ref.sliding_window(x.cpu(), (128, 128, 128), 4, rec.replay(), overlap=0.25, mode=mode)
        assert len(rec.outputs) == 2 and all(torch.equal(a, b) for a, b in zip(rec.inputs, batches))
        assert torch.equal(got.cpu(), want), mode


def test_generator_single_window_equals_direct_call():
    gen = _generator()
    g = torch.Generator().manual_seed(15)
    x = (torch.rand(1, 1, 128, 128, 128, generator=g) * 2 - 1).cuda()
    with torch.no_grad():
        direct = gen(x).clone()
        sw = inf.sliding_window_inference(x, (128, 128, 128), 12, gen)
    assert torch.equal(sw, direct)
