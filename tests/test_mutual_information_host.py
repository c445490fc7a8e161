"""The numpy restatement of the joint histogram and mutual information (mi_ref.py) against np.histogram2d, its
own properties, and the argument checks of the two C entry points (host-side, no device)."""
import ctypes
import os

import numpy as np
import pytest

import mi_ref

SHAPE = (40, 40, 40)


def _hist2d(a, b, bins, lo, hi):
    h, _, _ = np.histogram2d(a.ravel().astype(np.float64), b.ravel().astype(np.float64), bins=bins,
                             range=((lo, hi), (lo, hi)))
    return h.astype(np.int64)


@pytest.mark.parametrize("bins,lo,hi", [(256, 0, 256), (64, 0, 256), (32, 0, 256), (256, 0, 255), (23, 0, 255),
                                        (100, 0, 255)])
def test_restatement_equals_histogram2d_on_integer_levels(bins, lo, hi):
    """On integer-valued data the fp32 rule and np.histogram2d's float64 edge search agree exactly, for dyadic
    and non-dyadic bin widths alike.  (On continuous data they do not for non-dyadic bin counts: with 23 or 100
    bins over [-1, 1] about one voxel in 64,000 lands in the neighbouring bin under float64, so there the
    restatement is the only yardstick of the kernel.)"""
    a, b = mi_ref.mri_like_pair(SHAPE, seed=11)
    got = mi_ref.joint_histogram(a, b, bins, (float(lo), float(hi)))
    want = _hist2d(a, b, bins, lo, hi)
    assert got.sum() == a.size
    assert np.array_equal(got, want), int(np.abs(got - want).sum())


@pytest.mark.parametrize("bins", [64, 256, 23, 100])
def test_restatement_on_continuous_data_differs_from_float64_only_at_bin_edges(bins):
    """Continuous data in [-1, 1]: the fp32 rule rounds (v - lo), s and their product, three roundings of at most
    2^-24 relative each on a t below `bins`, so its t is within bins * 2^-22 of the float64 one.  A voxel may
    therefore sit in the neighbouring bin only when its float64 t is that close to an integer, and never further
    than one bin away.  np.histogram2d is no exact yardstick here; the restatement is."""
    a, _ = mi_ref.continuous_pair(SHAPE, seed=12)
    idx, inside = mi_ref.bin_index(a, -1.0, 1.0, bins)
    assert inside.all()
    t64 = (a.ravel().astype(np.float64) + 1.0) * (bins / 2.0)
    idx64 = np.minimum(np.floor(t64).astype(np.int64), bins - 1)
    moved = idx != idx64
    assert moved.sum() <= 8                          # 64,000 voxels x bins x 2^-22 per unit of t: a handful at most
    assert np.all(np.abs(idx - idx64)[moved] == 1)
    assert np.all(np.abs(t64 - np.rint(t64))[moved] <= bins * 2.0 ** -22)


def test_restatement_selection_rules():
    a = np.array([0.0, 255.0, 256.0, 256.5, -0.5, np.nan, 0.0, 3.0], dtype=np.float32)
    b = np.array([0.0, 256.0, 0.0, 1.0, 1.0, 1.0, 7.0, np.nan], dtype=np.float32)
    h = mi_ref.joint_histogram(a, b, 256, (0.0, 256.0))
    assert h.sum() == 4 and h[0, 0] == 1 and h[255, 255] == 1 and h[255, 0] == 1 and h[0, 7] == 1
    assert mi_ref.joint_histogram(a, b, 256, (0.0, 256.0), "both_nonzero").sum() == 1
    assert mi_ref.joint_histogram(a, b, 256, (0.0, 256.0), "either_nonzero").sum() == 3
    keep = np.array([1, 0, 1, 1, 1, 1, 0, 1], dtype=np.uint8)
    assert mi_ref.joint_histogram(a, b, 256, (0.0, 256.0), keep).sum() == 2
    # separate ranges per image
    h = mi_ref.joint_histogram(a, b, 4, ((0.0, 4.0), (0.0, 8.0)))
    assert h.sum() == 2 and h[0, 0] == 1 and h[0, 3] == 1


def test_restatement_properties():
    a, b = mi_ref.mri_like_pair(SHAPE, seed=13)
    for bins in (256, 23):
        aa = mi_ref.mutual_information(a, a, bins, (0.0, 255.0))
        assert aa["mi"] == aa["h_a"] == aa["h_b"] == aa["h_ab"] and aa["nmi"] == 2.0
        ab, ba = mi_ref.mutual_information(a, b, bins, (0.0, 255.0)), mi_ref.mutual_information(b, a, bins, (0.0, 255.0))
        # the marginals swap exactly; the joint sum runs over the transposed order, so it may round differently
        assert ab["h_a"] == ba["h_b"] and ab["h_b"] == ba["h_a"]
        assert abs(ab["h_ab"] - ba["h_ab"]) < 1e-12 and abs(ab["mi"] - ba["mi"]) < 1e-12
        assert ab["count"] == a.size
        rng = np.random.default_rng(14)
        sh = mi_ref.mutual_information(rng.permutation(a.ravel()), rng.permutation(b.ravel()), bins, (0.0, 255.0))
        assert 0.0 <= sh["mi"] < ab["mi"]
        assert ab["mi"] <= min(ab["h_a"], ab["h_b"]) + 1e-12
    # edge cases
    empty = mi_ref.mutual_information_from_histogram(np.zeros((8, 8), dtype=np.int64))
    assert empty["count"] == 0.0 and all(np.isnan(empty[k]) for k in ("mi", "h_a", "h_b", "h_ab", "nmi"))
    one = np.zeros((8, 8), dtype=np.int64)
    one[3, 5] = 1000
    one = mi_ref.mutual_information_from_histogram(one)
    assert one["mi"] == 0.0 and one["nmi"] == 1.0 and one["h_ab"] == 0.0 and one["count"] == 1000.0
    # two equally filled bins on the diagonal: one bit
    two = np.zeros((4, 4), dtype=np.int64)
    two[0, 0] = two[2, 2] = 50
    assert abs(mi_ref.mutual_information_from_histogram(two)["mi"] - np.log(2.0)) < 1e-15


def test_argument_checks_without_gpu():
    """Argument validation happens on the host before any launch, and the message names the function."""
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.lib()
    one = ctypes.c_void_p(64)                       # never dereferenced: every call below is refused before a launch

    def jh(a=one, b=one, mask=None, mode=0, n=8, batch=1, lo=0.0, hi=256.0, lo_b=0.0, hi_b=256.0, bins=256, hist=one):
        return lib.mpgan_joint_histogram(a, b, mask, mode, n, batch, lo, hi, lo_b, hi_b, bins, hist, None)

    bad = [dict(bins=1), dict(bins=257), dict(hi=0.0), dict(hi=-1.0), dict(hi_b=0.0), dict(lo=float("nan")),
           dict(hi=float("inf")), dict(lo=-3e38, hi=3e38), dict(batch=0), dict(n=-1), dict(mode=4), dict(mode=-1),
           dict(mode=3, mask=None), dict(hist=None), dict(a=None), dict(b=None)]
    for kw in bad:
        assert jh(**kw) == -1, kw
        assert b"joint_histogram" in lib.mpgan_last_error(), (kw, lib.mpgan_last_error())
    for args in [(None, 1, 256, one), (one, 1, 256, None), (one, 0, 256, one), (one, 1, 1, one), (one, 1, 257, one)]:
        assert lib.mpgan_mutual_information(*args, None) == -1, args
        assert b"mutual_information" in lib.mpgan_last_error()
