"""Host half of mpgan_amd.inference (no GPU): window enumeration, padding, the Gaussian importance map and the
argument checks, against hand-computed cases and the CPU restatement in sliding_window_ref.py."""
import random

import pytest
import torch

import sliding_window_ref as ref
from mpgan_amd import inference as inf


def _ref_starts(image_size, roi, overlap):
    roi = ref.fall_back_tuple(roi, image_size)
    padded = tuple(max(s, r) for s, r in zip(image_size, roi))
    interval = ref.get_scan_interval(padded, roi, len(image_size), overlap)
    return [tuple(s.start for s in w) for w in ref.dense_patch_slices(padded, roi, interval)]


@pytest.mark.parametrize("size,roi,overlap,starts", [
    ((256,), (128,), 0.25, [(0, 96, 128)]),
    ((128,), (128,), 0.25, [(0,)]),
    ((128,), (128,), 0.9, [(0,)]),
    ((256,), (128,), 0.0, [(0, 128)]),
    ((256,), (128,), 0.5, [(0, 64, 128)]),
    ((256,), (128,), 0.75, [(0, 32, 64, 96, 128)]),
    ((150, 200, 130), (64, 64, 64), 0.25, [(0, 48, 86), (0, 48, 96, 136), (0, 48, 66)]),
])
def test_hand_computed_starts(size, roi, overlap, starts):
    plan = inf.plan_windows(size, roi, overlap)
    assert list(plan.starts) == [tuple(s) for s in starts]
    assert plan.pad_lo == (0,) * len(size) and plan.padded == tuple(size)


def test_image_smaller_than_roi_pads_and_takes_one_window():
    plan = inf.plan_windows((100, 128, 131), (128, 128, 128), 0.25)
    assert plan.pad_lo == (14, 0, 0)            # diff 28 -> 14 before, 14 after; W=131 is not padded
    assert plan.padded == (128, 128, 131)
    assert plan.starts == ((0,), (0,), (0, 3))
    plan = inf.plan_windows((99,), (128,), 0.5)
    assert plan.pad_lo == (14,) and plan.padded == (128,) and plan.starts == ((0,),)   # 29 = 14 + 15


def test_roi_fallback_and_window_order():
    plan = inf.plan_windows((40, 50), (0, None), 0.25)
    assert plan.roi == (40, 50) and plan.windows() == [(0, 0)]
    plan = inf.plan_windows((256, 256, 256), 128, 0.25)
    w = plan.windows()
    assert len(w) == plan.num_windows == 27
    assert w[:4] == [(0, 0, 0), (0, 0, 96), (0, 0, 128), (0, 96, 0)]      # first spatial dim slowest


def test_enumeration_matches_restatement_sweep():
    rng = random.Random(1234)
    cases = 0
    while cases < 400:
        nsd = rng.choice((2, 3))
        size = tuple(rng.randint(1, 300) for _ in range(nsd))
        roi = tuple(rng.choice((rng.randint(1, 160), 0, -1, None, 64, 128)) for _ in range(nsd))
        overlap = rng.choice((0.0, 0.25, 0.5, 0.75, 0.9, 0.99, rng.random() * 0.999))
        plan = inf.plan_windows(size, roi, overlap)
        if plan.num_windows > 20000:          # (interval 1 over a large image: millions of windows, slow to list)
            continue
        cases += 1
        assert plan.windows() == _ref_starts(size, roi, overlap), (size, roi, overlap)
        r = ref.fall_back_tuple(roi, size)
        assert plan.roi == r
        assert plan.pad_lo == tuple(max(a - s, 0) // 2 for a, s in zip(r, size))


@pytest.mark.parametrize("roi,sigma_scale", [((64, 64, 64), 0.125), ((128, 128, 128), 0.125), ((32, 48, 20), 0.125),
                                             ((40, 24), 0.3), ((128, 128), 0.125), ((30, 9, 64), 0.05)])
def test_gaussian_map_matches_restatement(roi, sigma_scale):
    got = inf.importance_map(roi, "gaussian", sigma_scale)
    want = ref.compute_importance_map(roi, "gaussian", sigma_scale)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want)
    assert (got > 0).all() and got.max().item() == 1.0


def test_gaussian_vectors_match_gaussian_1d():
    for r, s in ((64, 0.125), (128, 0.125), (20, 0.3), (30, 0.05)):
        (v,) = inf.gaussian_vectors((r,), s)
        k = ref.gaussian_1d(r * s)
        tail = (k.numel() - 1) // 2
        c = r // 2
        for p in range(r):
            want = k[p - c + tail].item() if abs(p - c) <= tail else 0.0
            assert v[p].item() == want, (r, s, p)


def test_constant_map_is_ones():
    assert torch.equal(inf.importance_map((5, 6, 7), "constant"), torch.ones(5, 6, 7))


def _pred(x):
    return x


def test_argument_validation():
    x = torch.zeros(1, 1, 32, 32, 32)
    with pytest.raises(ValueError, match="overlap"):
        inf.sliding_window_inference(x, (16, 16, 16), 1, _pred, overlap=1.0)
    with pytest.raises(ValueError, match="overlap"):
        inf.sliding_window_inference(x, (16, 16, 16), 1, _pred, overlap=-0.1)
    with pytest.raises(ValueError, match="roi_size"):
        inf.sliding_window_inference(x, (16, 16), 1, _pred)
    with pytest.raises(ValueError, match="mode"):
        inf.sliding_window_inference(x, (16, 16, 16), 1, _pred, mode="linear")
    with pytest.raises(NotImplementedError, match="padding_mode"):
        inf.sliding_window_inference(x, (16, 16, 16), 1, _pred, padding_mode="reflect")
    with pytest.raises(NotImplementedError, match="padding_mode"):
        inf.sliding_window_inference(x, (16, 16, 16), 1, _pred, padding_mode="replicate")
    with pytest.raises(ValueError, match="sw_batch_size"):
        inf.sliding_window_inference(x, (16, 16, 16), 0, _pred)
    with pytest.raises(ValueError, match="CUDA"):                # a valid call on a CPU tensor
        inf.sliding_window_inference(x, (16, 16, 16), 1, _pred)
    with pytest.raises(ValueError, match="CUDA"):
        inf.sliding_window_inference(x.double(), (16, 16, 16), 1, _pred)
    with pytest.raises(ValueError, match="spatial dims"):
        inf.sliding_window_inference(torch.zeros(1, 32, 32), (16, 16), 1, _pred)
    with pytest.raises(ValueError, match="mode"):
        inf.SlidingWindowInferer((16, 16, 16), mode="nearest")
    with pytest.raises(ValueError, match="CUDA"):
        inf.SlidingWindowInferer((16, 16, 16), sw_batch_size=2)(x, _pred)


def test_library_validates_geometry_without_gpu():
    """The C entries check the geometry and the host start table before any launch."""
    import ctypes as C
    import os

    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    L = _lib.lib()
    starts = (C.c_int32 * 5)(0, 0, 0, 32, 40)          # z: 0; y: 0; x: 0, 32, 40 (40 > 64 - 32 is out of range)
    g = _lib.SwGeomC()
    g.batch = 1
    for d, (s, r, n) in enumerate(((1, 1, 1), (32, 32, 1), (64, 32, 3))):
        g.dhw[d], g.padded[d], g.roi[d], g.num[d] = s, s, r, n
    g.starts_dev = 16                                    # never dereferenced: validation fails first
    g.starts_host = C.cast(starts, C.POINTER(C.c_int32))
    assert L.mpgan_sw_count(C.byref(g), None, 16, None) == -1
    assert b"window start 40" in L.mpgan_last_error()
    starts[4] = 32
    g.roi[2] = 80                                        # roi larger than the padded extent
    assert L.mpgan_sw_gather(C.byref(g), 16, 1, 0, 1, 0.0, 16, None) == -1
    assert b"padded extent" in L.mpgan_last_error()
    g.roi[2] = 32
    assert L.mpgan_sw_blend(C.byref(g), 16, 1, 2, 2, None, 16, None) == -1     # windows [2, 4) of 3
    assert b"windows" in L.mpgan_last_error()
    assert L.mpgan_sw_finalize(None, 16, 1, 16, 16, None) == -1
