"""Every refusal of the statistics layer, pinned row by row (in the manner of test_warp_refusals_gpu.py):

  PY_ROWS  the Python layer's refusals of the mask argument and of the SSIM shape and device checks, through
           metrics.image_errors / ssim / ssim_map / joint_histogram and losses.ssim_loss / masked_l1_loss: a row is
           (function, label, what to change in the good call, the word its ValueError must contain).  Every row raises
           before a launch; the inputs are compared once at the end.  Two rows are the opposite: a mask with channel
           extent 1 is taken by the two losses (and gives the bits of the expanded mask) and refused by the metrics.
  C_ROWS   the library's own range, reduction, wrt, upstream_stride and workspace refusals, called through ctypes with
           host pointers that are never dereferenced: a row is (entry point, label, change, status, message fragment).
           No device is needed, so these carry no gpu mark."""
import ctypes
import os

import pytest
import torch

IMG, VOL, PAIR = (9, 11), (9, 9, 11), (2, 2, 9, 11)


def _mask(shape, dev="cuda", dtype=torch.uint8):
    return torch.ones(shape, dtype=dtype, device=dev)


def _metric_good(shape=IMG):
    return dict(a=torch.zeros(shape, device="cuda"), b=torch.ones(shape, device="cuda"), mask=_mask(shape))


def _loss_good():
    return dict(pred=torch.zeros(PAIR, device="cuda"), target=torch.ones(PAIR, device="cuda"), mask=_mask(PAIR))


MASK_ROWS = [("mask of the wrong type", lambda g: dict(mask=[[1]]), "bool / uint8"),
             ("mask float32", lambda g: dict(mask=g["mask"].float()), "bool / uint8"),
             ("mask int64", lambda g: dict(mask=g["mask"].long()), "bool / uint8"),
             ("mask on the CPU", lambda g: dict(mask=g["mask"].cpu()), "inputs' device")]
METRIC_MASK_ROWS = MASK_ROWS + [
    ("mask one column short", lambda g: dict(mask=g["mask"][..., :-1].contiguous()), "same-shape"),
    ("mask of one more rank", lambda g: dict(mask=g["mask"][None]), "same-shape")]
LOSS_MASK_ROWS = MASK_ROWS + [
    ("mask one column short", lambda g: dict(mask=g["mask"][..., :-1].contiguous()), "channel extent 1"),
    ("mask with batch extent 1", lambda g: dict(mask=g["mask"][:1]), "channel extent 1"),
    ("mask without the channel axis", lambda g: dict(mask=g["mask"][:, 0]), "channel extent 1")]
SSIM_ROWS = [("b one column short", lambda g: dict(b=g["b"][..., :-1].contiguous()), "same-shape"),
             ("a pair of rank 4", lambda g: dict(a=g["a"][None, None], b=g["b"][None, None], mask=None), "same-shape")]
WEIGHTED_SSIM_ROWS = [("a on the CPU", lambda g: dict(a=g["a"].cpu()), "device"),
                      ("both on the CPU", lambda g: dict(a=g["a"].cpu(), b=g["b"].cpu()), "device"),
                      ("data_range 0", lambda g: dict(data_range=0.0), "data_range"),
                      ("extents below the window", lambda g: {k: v[:6].contiguous() for k, v in g.items()},
                       "below the 7-wide window")]
PAIR_ROWS = [("target one column short", lambda g: dict(target=g["target"][..., :-1].contiguous()), "shape mismatch"),
             ("pred float64", lambda g: dict(pred=g["pred"].double()), "fp32 device"),
             ("pred and its mask on the CPU", lambda g: dict(pred=g["pred"].cpu(), mask=g["mask"].cpu()), "fp32 device"),
             ("target on the CPU", lambda g: dict(target=g["target"].cpu()), "fp32 device")]


def _cut(g, sl):
    return {k: v[sl].contiguous() for k, v in g.items()}


def _py_tables():
    from mpgan_amd import losses, metrics
    return {
        "metrics.image_errors": (metrics.image_errors, _metric_good, METRIC_MASK_ROWS + [
            ("b one column short", lambda g: dict(b=g["b"][..., :-1].contiguous()), "shape mismatch"),
            ("a float64", lambda g: dict(a=g["a"].double()), "fp32 device"),
            ("both on the CPU", lambda g: dict(a=g["a"].cpu(), b=g["b"].cpu()), "fp32 device"),
            ("mask with channel extent 1", lambda g: dict(a=g["a"].expand(PAIR), b=g["b"].expand(PAIR),
                                                          mask=_mask((2, 1, 9, 11))), "same-shape")]),
        "metrics.ssim": (metrics.ssim, _metric_good, METRIC_MASK_ROWS + SSIM_ROWS + WEIGHTED_SSIM_ROWS + [
            ("extents below the window, no mask", lambda g: dict(a=g["a"][:6].contiguous(), b=g["b"][:6].contiguous(),
                                                                mask=None), "below the 7-wide window"),
            ("mask with depth extent 1", lambda g: dict(_metric_good(VOL), mask=_mask((1, 9, 11))), "same-shape")]),
        "metrics.ssim_map": (metrics.ssim_map, lambda: {k: v for k, v in _metric_good().items() if k != "mask"},
                             [(label, change, word) for label, change, word in SSIM_ROWS + WEIGHTED_SSIM_ROWS
                              if "rank 4" not in label] +
                             [("a pair of rank 4", lambda g: dict(a=g["a"][None, None], b=g["b"][None, None]),
                               "same-shape")]),
        "metrics.joint_histogram": (metrics.joint_histogram, _metric_good, METRIC_MASK_ROWS[1:] + [
            ("mask names no rule", lambda g: dict(mask="foreground"), "unknown mask"),
            ("b one column short", lambda g: dict(b=g["b"][..., :-1].contiguous()), "shape mismatch"),
            ("a float64", lambda g: dict(a=g["a"].double()), "fp32 device"),
            ("a on the CPU", lambda g: dict(a=g["a"].cpu()), "fp32 device"),
            ("mask with channel extent 1", lambda g: dict(a=g["a"].expand(PAIR), b=g["b"].expand(PAIR), batched=True,
                                                          mask=_mask((2, 1, 9, 11))), "same-shape")]),
        "losses.ssim_loss": (losses.ssim_loss, _loss_good, LOSS_MASK_ROWS + PAIR_ROWS + [
            ("mask and threshold", lambda g: dict(threshold=0.0), "at most one of mask and threshold"),
            ("extents below the window", lambda g: _cut(g, (Ellipsis, slice(0, 6), slice(None))),
             "below the 7-wide window"),
            ("a depth of 3", lambda g: {k: v[:, :, None].expand(2, 2, 3, 9, 11) for k, v in g.items()},
             "below the 7-wide window"),
            ("a pair of rank 3", lambda g: _cut(g, (0,)), "expects")]),
        "losses.masked_l1_loss": (losses.masked_l1_loss, _loss_good, LOSS_MASK_ROWS + PAIR_ROWS + [
            ("mask and threshold", lambda g: dict(threshold=0.0), "exactly one of mask and threshold"),
            ("neither mask nor threshold", lambda g: dict(mask=None), "exactly one of mask and threshold"),
            ("a pair of rank 3", lambda g: _cut(g, (0,)), "expects")])}


PY_FUNCTIONS = ("metrics.image_errors", "metrics.ssim", "metrics.ssim_map", "metrics.joint_histogram",
                "losses.ssim_loss", "losses.masked_l1_loss")


@pytest.mark.gpu
@pytest.mark.parametrize("name", PY_FUNCTIONS)
def test_every_python_row_raises_and_leaves_the_inputs_alone(name):
    fn, good, rows = _py_tables()[name]
    g = good()
    kept = [(t, t.clone()) for t in g.values()]
    for label, change, word in rows:
        with pytest.raises(ValueError) as e:
            fn(**dict(g, **change(g)))
        assert word in str(e.value), (name, label, word, str(e.value))
    assert len(rows) >= 6, (name, len(rows))
    torch.cuda.synchronize()
    for t, was in kept:
        assert torch.equal(t, was), name


@pytest.mark.gpu
def test_channel_extent_one_is_broadcast_by_the_losses_alone():
    from mpgan_amd import losses
    gen = torch.Generator().manual_seed(3)
    pred, target = torch.rand(PAIR, generator=gen).cuda(), torch.rand(PAIR, generator=gen).cuda()
    one = (torch.rand((2, 1, 9, 11), generator=gen) < 0.6).cuda()
    for fn in (losses.ssim_loss, losses.masked_l1_loss):
        for mask in (one, one.view(torch.uint8)):
            got, want = fn(pred, target, mask=mask), fn(pred, target, mask=one.expand(PAIR).contiguous())
            assert torch.equal(got, want) and bool(torch.isfinite(got)), fn.__name__


# ---- the library's own refusals: no device -----------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -2
INF, NAN = float("inf"), float("nan")
TINY = 1e-45                                            # the smallest fp32 subnormal: bins / TINY overflows fp32


def _dhw(*v):
    return (ctypes.c_int32 * 3)(*v)


def _lib():
    from mpgan_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmpgan_hip.so not built (run __graft_entry__.build())")
    return _lib.lib()


def _entry_points(lib, p):
    """name -> (call(**changes), the names of its keyword arguments' defaults); p is an 8-byte-aligned host address that
    no call dereferences."""
    big = 1 << 16

    def jh(lo=0.0, hi=256.0, lo_b=0.0, hi_b=256.0):
        return lib.mpgan_joint_histogram(p, p, None, 0, 8, 1, lo, hi, lo_b, hi_b, 256, p, None)

    def otsu(lo=-1.0, hi=1.0, wsp=p):
        return lib.mpgan_otsu_threshold(p, 64, 1, lo, hi, 64, wsp, p, None)

    def pmi_f(lo=0.0, hi=1.0, lo_b=0.0, hi_b=1.0, reduction=0, wsp=p, ws=big):
        return lib.mpgan_parzen_mi_forward(p, p, 64, 1, lo, hi, lo_b, hi_b, 23, 0.5, 1e-7, 1e-7, wsp, ws, None, p, None,
                                           reduction, p, None)

    def pmi_b(lo=0.0, hi=1.0, lo_b=0.0, hi_b=1.0, stride=0, wrt=0):
        return lib.mpgan_parzen_mi_backward(p, p, 64, 1, lo, hi, lo_b, hi_b, 23, 0.5, p, p, stride, 1.0, wrt, p, None)

    def ssim_f(entry, extra):
        def call(items=1, ch=1, lo=0.0, hi=1.0, reduction=0, wsp=p, ws=big):
            return entry(p, p, _dhw(1, 9, 9), items, ch, lo, hi, *extra[:2], 1, wsp, ws, p, big, *extra[2:], reduction, p,
                         None)
        return call

    def ssim_b(entry, extra):
        def call(items=1, ch=1, lo=0.0, stride=0, scale=-1.0, wrt=0):
            return entry(p, p, _dhw(1, 9, 9), items, ch, lo, 1, p, big, *extra, p, stride, scale, wrt, p, None)
        return call

    def edge_f(items=1, ch=1, reduction=0, wsp=p, ws=big):
        return lib.mpgan_edge_loss_forward(p, p, _dhw(1, 9, 9), items, ch, 1e-6, wsp, ws, reduction, p, None)

    def edge_b(items=1, ch=1, stride=0, scale=1.0, wrt=0):
        return lib.mpgan_edge_loss_backward(p, p, _dhw(1, 9, 9), items, ch, 1e-6, p, stride, scale, wrt, p, None)

    def l1_f(items=1, ch=1, reduction=0, wsp=p, ws=big, den=p):
        return lib.mpgan_masked_l1_forward(p, p, 64, items, ch, p, None, 1.0, 0.0, wsp, ws, den, reduction, p, None)

    def l1_b(items=1, ch=1, stride=0, scale=1.0):
        return lib.mpgan_masked_l1_backward(p, p, 64, items, ch, p, None, 1.0, 0.0, p, p, stride, scale, p, None, None)

    def ssim(dhw=(1, 9, 9), wsp=p, ws=big):
        return lib.mpgan_ssim(p, p, _dhw(*dhw), 256.0, wsp, ws, p, None)

    return {"joint_histogram": jh, "otsu_threshold": otsu, "parzen_mi_forward": pmi_f, "parzen_mi_backward": pmi_b,
            "ssim_loss_forward": ssim_f(lib.mpgan_ssim_loss_forward, ()),
            "masked_ssim_loss_forward": ssim_f(lib.mpgan_masked_ssim_loss_forward, (p, None, p, None)),
            "ssim_loss_backward": ssim_b(lib.mpgan_ssim_loss_backward, ()),
            "masked_ssim_loss_backward": ssim_b(lib.mpgan_masked_ssim_loss_backward, (p,)),
            "edge_loss_forward": edge_f, "edge_loss_backward": edge_b, "masked_l1_forward": l1_f,
            "masked_l1_backward": l1_b, "ssim": ssim}


RANGE_A = [("hi == lo", dict(hi=0.0, lo=0.0), b"value range needs hi > lo"),
           ("hi < lo", dict(hi=-2.0), b"value range needs hi > lo"),
           ("hi infinite", dict(hi=INF), b"non-finite value range"),
           ("lo NaN", dict(lo=NAN), b"non-finite value range"),
           ("an infinite span", dict(lo=-3e38, hi=3e38), b"non-finite value range")]
RANGE_B = [("hi_b == lo_b", dict(hi_b=0.0), b"value range needs hi > lo"),
           ("lo_b infinite", dict(lo_b=-INF), b"non-finite value range")]
NARROW = ("too narrow", dict(lo=0.0, hi=TINY), b"value range too narrow for fp32 binning")
SSIM_RANGE = [("hi == lo", dict(hi=0.0), b"hi > lo"), ("hi infinite", dict(hi=INF), b"hi > lo"),
              ("lo NaN", dict(lo=NAN), b"hi > lo")]
CHANNELS = [("no channel", dict(ch=0), b"channels"), ("items no multiple of the channels", dict(items=3, ch=2), b"channels")]
REDUCTION = [("reduction 3", dict(reduction=3), b"unknown reduction"), ("reduction -1", dict(reduction=-1), b"unknown reduction")]
WORKSPACE = [("workspace one byte short", dict(ws=8), b"workspace too small"),
             ("workspace misaligned", dict(wsp=4), b"workspace must be 8-byte aligned")]
WRT = [("wrt 2", dict(wrt=2), b"wrt"), ("wrt -1", dict(wrt=-1), b"wrt")]
STRIDE = [("upstream_stride 2", dict(stride=2), b"upstream_stride"), ("upstream_stride -1", dict(stride=-1), b"upstream_stride")]
SCALE = [("scale infinite", dict(scale=INF), b"non-finite"), ("scale NaN", dict(scale=NAN), b"non-finite")]

C_ROWS = {
    "joint_histogram": RANGE_A + RANGE_B + [NARROW, ("b too narrow", dict(lo_b=0.0, hi_b=TINY), NARROW[2])],
    "otsu_threshold": RANGE_A + [NARROW, ("workspace misaligned", dict(wsp=4), b"workspace must be 8-byte aligned")],
    "parzen_mi_forward": RANGE_A + RANGE_B + REDUCTION + WORKSPACE,
    "parzen_mi_backward": RANGE_A + RANGE_B + WRT + STRIDE,
    "ssim_loss_forward": SSIM_RANGE + CHANNELS + REDUCTION + WORKSPACE,
    "masked_ssim_loss_forward": SSIM_RANGE + CHANNELS + REDUCTION + WORKSPACE,
    "ssim_loss_backward": CHANNELS + WRT + STRIDE + SCALE + [("lo NaN", dict(lo=NAN), b"non-finite")],
    "masked_ssim_loss_backward": CHANNELS + WRT + STRIDE + SCALE + [("lo NaN", dict(lo=NAN), b"non-finite")],
    "edge_loss_forward": CHANNELS + REDUCTION + WORKSPACE,
    "edge_loss_backward": CHANNELS + WRT + STRIDE + SCALE,
    "masked_l1_forward": CHANNELS + REDUCTION + WORKSPACE[:1] + [("workspace misaligned", dict(wsp=4), b"8-byte aligned"),
                                                                  ("den misaligned", dict(den=4), b"8-byte aligned")],
    "masked_l1_backward": CHANNELS + STRIDE + SCALE,
    "ssim": [("workspace one byte short", dict(ws=7), b"workspace too small"),
             ("extents below the window", dict(dhw=(1, 6, 9)), b"below the 7-wide window"),
             ("no plane", dict(dhw=(0, 9, 9)), b"below the 7-wide window")]}
UNSUPPORTED_ROWS = {"ssim": [("a depth of 3", dict(dhw=(3, 9, 9)), b"depth 3"), ("a depth of 6", dict(dhw=(6, 9, 9)), b"depth 6")]}


@pytest.mark.parametrize("name", sorted(C_ROWS))
def test_every_c_row_is_refused_on_the_host(name):
    lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    call = _entry_points(lib, p)[name]
    for status, rows in ((INVALID, C_ROWS[name]), (UNSUPPORTED, UNSUPPORTED_ROWS.get(name, []))):
        for label, change, word in rows:
            change = {k: (p + v if k in ("wsp", "den") else v) for k, v in change.items()}
            rc = call(**change)
            msg = lib.mpgan_last_error()
            assert rc == status and word in msg and name.encode() in msg, (name, label, rc, msg)


def test_ssim_workspace_is_one_double_per_tile():
    lib = _lib()
    for dhw, tiles in (((1, 7, 7), 1), ((1, 136, 544), 17 * 17), ((9, 17, 39), 1 * 2 * 2), ((13, 9, 40), 2 * 1 * 2),
                       ((3, 9, 9), 3), ((1, 15, 39), 2 * 2)):
        assert lib.mpgan_ssim_workspace(_dhw(*dhw)) == 8 * tiles, dhw
    for bad in ((1, 6, 9), (1, 9, 6), (0, 9, 9)):
        assert lib.mpgan_ssim_workspace(_dhw(*bad)) == -1, bad
    assert lib.mpgan_ssim_workspace(None) == -1
