"""The decision table of the four sliding-window launches (csrc/window_ops.hip: choose_sw_gather / _count / _blend /
_finalize), read through mpgan_sw_kernel_name with fake pointers: no GPU, nothing is launched or dereferenced.  One
predicate flips at a time and the label must follow; together the table reaches all 14 kernel instances."""
import ctypes as C
import os

import pytest

from mpgan_amd import _lib
from mpgan_amd import inference as inf

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")

A, U = 16, 20            # a 16-byte aligned fake pointer and one 4 bytes off
SEEN = set()


def _geom(W=24, padded_x=24, roi_x=12, pad_lo_x=0, x_starts=(0, 12)):
    """A (3, 5, W) image with roi (2, 3, roi_x); only the x dim varies.  Returns (geometry, keep-alive)."""
    starts = (C.c_int32 * (3 + len(x_starts)))(0, 1, 0, *x_starts)        # z: 0, 1; y: 0; x: x_starts
    g = _lib.SwGeomC()
    g.batch = 2
    for d, (s, p, pp, r, n) in enumerate(((3, 0, 3, 2, 2), (5, 0, 5, 5, 1),
                                          (W, pad_lo_x, padded_x, roi_x, len(x_starts)))):
        g.dhw[d], g.pad_lo[d], g.padded[d], g.roi[d], g.num[d] = s, p, pp, r, n
    g.starts_dev = A                                                        # never dereferenced
    g.starts_host = C.cast(starts, C.POINTER(C.c_int32))
    return g, starts


def _name(launch, geom, *ptrs):
    g, keep = geom
    name = inf.sw_kernel_name(launch, g, *ptrs)
    SEEN.add(name)
    return name


def _status(launch, geom, *ptrs):
    g, keep = geom
    p = tuple(ptrs) + (None,) * (3 - len(ptrs))
    buf = C.create_string_buffer(64)
    return _lib.lib().mpgan_sw_kernel_name(inf.SW_LAUNCHES[launch], C.byref(g), *p, buf, len(buf))


def test_gather_forms():
    assert _name("gather", _geom(roi_x=12), A, A) == "sw_gather_kernel<true, true>"
    assert _name("gather", _geom(roi_x=10), A, A) == "sw_gather_kernel<false, true>"       # roi_x % 4
    assert _name("gather", _geom(roi_x=12), U, A) == "sw_gather_kernel<true, false>"       # input base off by 4 bytes
    assert _name("gather", _geom(roi_x=10), U, A) == "sw_gather_kernel<false, false>"
    assert _name("gather", _geom(roi_x=10), A, U) == "sw_gather_kernel<false, true>"       # scalar stores: any batch
    assert _status("gather", _geom(roi_x=12), A, U) == -2                                  # MPGAN_ERR_UNSUPPORTED
    assert b"16-byte aligned" in _lib.lib().mpgan_last_error()
    assert _status("gather", _geom(roi_x=12), None, A) == -1 and _status("gather", _geom(roi_x=12), A, None) == -1


# the predicates count and blend share: (geometry arguments, quads possible)
_QUADS = [
    (dict(), True),
    (dict(roi_x=10, x_starts=(0, 12)), False),                    # roi_x % 4
    (dict(W=26, padded_x=26, x_starts=(0, 12)), False),           # padded_x % 4
    (dict(x_starts=(0, 6, 12)), False),                           # one x start not a multiple of 4
    (dict(x_starts=(0, 4, 12)), True),
    (dict(W=10, padded_x=12, pad_lo_x=1, x_starts=(0,)), True),   # the x padding does not enter count / blend
]


@pytest.mark.parametrize("kw,quads", _QUADS)
def test_count_forms(kw, quads):
    v = "true" if quads else "false"
    assert _name("count", _geom(**kw), None, A) == f"sw_count_kernel<{v}, true>"           # imp null: constant
    assert _name("count", _geom(**kw), A, A) == f"sw_count_kernel<{v}, false>"             # imp given
    # each pointer off by 4 bytes on its own sends the launch to the scalar form
    assert _name("count", _geom(**kw), None, U) == "sw_count_kernel<false, true>"
    assert _name("count", _geom(**kw), A, U) == "sw_count_kernel<false, false>"
    assert _name("count", _geom(**kw), U, A) == "sw_count_kernel<false, false>"
    assert _status("count", _geom(**kw), A, None) == -1


@pytest.mark.parametrize("kw,quads", _QUADS)
def test_blend_forms(kw, quads):
    v = "true" if quads else "false"
    assert _name("blend", _geom(**kw), A, None, A) == f"sw_blend_kernel<{v}, true>"
    assert _name("blend", _geom(**kw), A, A, A) == f"sw_blend_kernel<{v}, false>"
    assert _name("blend", _geom(**kw), U, None, A) == "sw_blend_kernel<false, true>"       # pred
    assert _name("blend", _geom(**kw), A, None, U) == "sw_blend_kernel<false, true>"       # acc
    assert _name("blend", _geom(**kw), U, A, A) == "sw_blend_kernel<false, false>"         # pred
    assert _name("blend", _geom(**kw), A, U, A) == "sw_blend_kernel<false, false>"         # imp
    assert _name("blend", _geom(**kw), A, A, U) == "sw_blend_kernel<false, false>"         # acc
    assert _status("blend", _geom(**kw), None, A, A) == -1 and _status("blend", _geom(**kw), A, A, None) == -1


def test_finalize_forms():
    q, s = "sw_finalize_kernel<true>", "sw_finalize_kernel<false>"
    assert _name("finalize", _geom(), A, A, A) == q
    assert _name("finalize", _geom(roi_x=10, x_starts=(0, 5, 14)), A, A, A) == q           # roi and starts do not enter
    assert _name("finalize", _geom(W=22, padded_x=24), A, A, A) == s                       # W % 4
    assert _name("finalize", _geom(W=24, padded_x=26), A, A, A) == s                       # padded_x % 4
    for pad, want in ((0, q), (4, q), (2, s)):                                             # pad_lo_x % 4
        assert _name("finalize", _geom(W=8, padded_x=16, roi_x=16, pad_lo_x=pad, x_starts=(0,)), A, A, A) == want
    for k in range(3):                                                                     # acc, count, out
        ptrs = [A, A, A]
        ptrs[k] = U
        assert _name("finalize", _geom(), *ptrs) == s
        ptrs[k] = None
        assert _status("finalize", _geom(), *ptrs) == -1


def test_query_validates_like_the_launch():
    L = _lib.lib()
    g = _geom(x_starts=(0, 13))                                    # 13 > 24 - 12
    for launch in inf.SW_LAUNCHES:
        assert _status(launch, g, A, A, A) == -1 and b"window start 13" in L.mpgan_last_error()
    assert _status("count", _geom(roi_x=28), None, A) == -1 and b"padded extent" in L.mpgan_last_error()
    g, keep = _geom()
    buf = C.create_string_buffer(64)
    assert L.mpgan_sw_kernel_name(4, C.byref(g), A, A, A, buf, len(buf)) == -1             # no such launch
    assert L.mpgan_sw_kernel_name(0, None, A, A, A, buf, len(buf)) == -1
    assert L.mpgan_sw_kernel_name(0, C.byref(g), A, A, A, buf, 8) == -1 and b"needs" in L.mpgan_last_error()
    assert L.mpgan_sw_kernel_name(0, C.byref(g), A, A, A, None, 64) == -1


def test_the_table_reaches_all_14_instances():
    """Runs last in this file: every label the tests above read."""
    want = ({f"sw_gather_kernel<{a}, {b}>" for a in ("true", "false") for b in ("true", "false")}
            | {f"sw_{k}_kernel<{a}, {b}>" for k in ("count", "blend") for a in ("true", "false")
               for b in ("true", "false")}
            | {"sw_finalize_kernel<true>", "sw_finalize_kernel<false>"})
    assert len(want) == 14
    assert SEEN == want, (sorted(want - SEEN), sorted(SEEN - want))
