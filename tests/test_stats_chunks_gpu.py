"""The streaming histograms' shared planner (stream_chunks) and wave peel (hist_submit) at the chunk boundaries, through
the public functions and exact against numpy: metrics.joint_histogram at 23 bins (one band, every a-row in LDS) and at
200 bins (banded), without a mask and with an explicit one, and preprocess.foreground_count, whose Otsu threshold comes
from the 2-round peel and whose count runs on the planner's chunks.  The lengths straddle the planners' minimum chunks
(4096 and 16384 values) and the four-value groups; the constant pair makes every lane of a wave crowd one counter."""
import numpy as np
import pytest
import torch

import foreground_ref as FR
import mi_ref

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4095, 4096, 4097, 16383, 16384, 16385)
VOLUME = (37, 41, 43)                                   # 65231 voxels: several chunks of either planner, an odd tail
ITEMS = (3, 4097)                                       # items 1 and 2 start off the 16-byte grid
RANGE = (0.0, 256.0)


def _pair(shape, kind):
    """fp32 (a, b, mask): "noise" spreads integer levels 0..255 over every bin with a tenth of the values outside the
    range; "const" is one level per image."""
    n = int(np.prod(shape))
    rng = np.random.RandomState(17 + n)
    if kind == "const":
        a, b = np.full(n, 100.0, np.float32), np.full(n, 7.0, np.float32)
    else:
        a = np.round(rng.rand(n) * 280 - 12).astype(np.float32)
        b = np.round(np.clip(0.7 * a + 20 * rng.randn(n), -5, 260)).astype(np.float32)
    mask = (rng.rand(n) < 0.7).astype(np.uint8)
    return a.reshape(shape), b.reshape(shape), mask.reshape(shape)


CASES = [((n,), kind) for n in LENGTHS for kind in ("noise", "const")] + [(VOLUME, "noise"), (VOLUME, "const")]


@pytest.mark.parametrize("bins", (23, 200))
@pytest.mark.parametrize("shape,kind", CASES)
def test_joint_histogram_of_one_item_is_exact(shape, kind, bins):
    from mpgan_amd import metrics
    a, b, mask = _pair(shape, kind)
    da, db, dm = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(mask).cuda()
    for m, dmask in ((None, None), (mask, dm)):
        got = metrics.joint_histogram(da, db, bins, RANGE, dmask).cpu().numpy()
        want = mi_ref.joint_histogram(a, b, bins, RANGE, m)
        assert np.array_equal(got, want), (shape, kind, bins, m is not None, int(got.sum()), int(want.sum()))
    if kind == "const":
        assert int(want.max()) == int(mask.sum()) > 0 or mask.sum() == 0


@pytest.mark.parametrize("bins", (23, 200))
@pytest.mark.parametrize("kind", ("noise", "const"))
def test_joint_histogram_of_three_items_is_exact(kind, bins):
    from mpgan_amd import metrics
    a, b, mask = _pair(ITEMS, kind)
    da, db, dm = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(mask).cuda()
    for m, dmask in ((None, None), (mask, dm)):
        got = metrics.joint_histogram(da, db, bins, RANGE, dmask, batched=True).cpu().numpy()
        for i in range(ITEMS[0]):
            want = mi_ref.joint_histogram(a[i], b[i], bins, RANGE, None if m is None else m[i])
            assert np.array_equal(got[i], want), (kind, bins, i, m is not None)


def _counts(x, items, threshold, bins):
    """Per item: the number of values above the threshold, Otsu's (foreground_ref, over RANGE) when it is "otsu"."""
    flat = x.reshape(items, -1)
    thr = [FR.otsu_threshold(v, *RANGE, bins) if threshold == "otsu" else np.float32(threshold) for v in flat]
    with np.errstate(invalid="ignore"):
        return np.array([int((v > t).sum()) for v, t in zip(flat, thr)], dtype=np.int64)


@pytest.mark.parametrize("threshold", (99.5, "otsu"))
@pytest.mark.parametrize("shape,kind", CASES)
def test_foreground_count_of_one_item_is_exact(shape, kind, threshold):
    from mpgan_amd import preprocess
    a, _, _ = _pair(shape, kind)
    x = a.reshape((1,) + shape if len(shape) == 1 else shape)             # (1, n) is an (H, W) image
    got = preprocess.foreground_count(torch.from_numpy(x).cuda(), threshold, bins=64, value_range=RANGE)
    assert got.dim() == 0 and int(got) == int(_counts(a, 1, threshold, 64)[0]), (shape, kind, threshold, int(got))


@pytest.mark.parametrize("threshold", (99.5, "otsu"))
@pytest.mark.parametrize("kind", ("noise", "const"))
def test_foreground_count_of_three_items_is_exact(kind, threshold):
    from mpgan_amd import preprocess
    a, _, _ = _pair(ITEMS, kind)
    x = torch.from_numpy(a.reshape(ITEMS[0], 1, 1, ITEMS[1])).cuda()
    got = preprocess.foreground_count(x, threshold, bins=64, value_range=RANGE).cpu().numpy()
    assert got.shape == (ITEMS[0], 1) and np.array_equal(got[:, 0], _counts(a, ITEMS[0], threshold, 64)), (kind, threshold)
