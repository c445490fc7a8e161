"""The profiling labels, variant codes and partial-row counts of the convs come from one choice per family
(choose_gather in conv_igemm.hip, choose_bf16 in conv_bf16.hip, choose_wgrad in conv_wgrad.hip): they must name the
instance the launch runs and agree with each other.  Library queries only: no GPU."""
import ctypes as C
import itertools
import re
import shutil
import subprocess

import pytest

from mpgan_amd import engine, ops
from mpgan_amd._lib import lib


def _g(n, spatial, cin, cout, k, s, p, **kw):
    d = len(spatial)
    t = (lambda v, fill: tuple(v) if not isinstance(v, int) else ((v,) * 3 if d == 3 else (fill, v, v)))
    sp = tuple(spatial) if d == 3 else (1,) + tuple(spatial)
    return ops.ConvGeom(n, sp, cin, cout, t(k, 1), t(s, 1), t(p, 0), **kw)


# C5's discriminator at 128^3 bs 4 (D.conv2..conv4 of the bf16 path): (geometry, forward label, backward-data label)
C5_DENSE = [
    (_g(4, (126, 126, 126), 64, 128, 3, 1, 0),
     "gather_conv_bf16_wide_kernel<4, 2, false, true, false>", "gather_patch8_bf16_kernel<64>"),
    (_g(4, (124, 124, 124), 128, 256, 4, 2, 0),
     "gather_conv_bf16_wide_kernel<2, 4, false, true, false>", "gather_conv_bf16_wide_kernel<2, 4, true, true, true>"),
    (_g(4, (61, 61, 61), 256, 256, 4, 2, 0),
     "gather_conv_bf16_kernel<128, false, 8>", "gather_conv_bf16_wide_kernel<2, 4, true, true, false>"),
]


@pytest.mark.parametrize("i", range(len(C5_DENSE)))
def test_c5_discriminator_labels(i):
    g, fwd, bwd = C5_DENSE[i]
    assert engine._bf16_kernel_name(g, False) == fwd
    assert engine._bf16_kernel_name(g, True) == bwd


def test_c5_generator_mm16_label():
    # C5's generator runs its K-stepped convs with bf16 matrix operands (MPGAN_CONV_MM_BF16): the pipelined kernel's
    # MM16 instance, never the DMA-staged fp32 kernel whose variant code it keeps
    g = _g(4, (32, 32, 32), 32, 32, 3, 1, 1, mm_bf16=True)
    gc = g.c()
    assert lib().mpgan_conv_variant(C.byref(gc), 1, 0) == 3032
    assert engine.gather_kernel_name(g, True, False) == "gather_conv_pipe_kernel<32, 1, 1, 1, 1, 0, false, 1, true>"
    g = _g(4, (16, 16, 16), 192, 32, 3, 2, 1, transposed=True, out_pad=(1, 1, 1), mm_bf16=True)
    assert engine.gather_kernel_name(g, False, False) == "gather_conv_pipe_kernel<32, 1, 1, 1, 1, 0, false, 1, true>"


def _bf16_sweep():
    for d, sp in [(2, (17, 23)), (2, (64, 64)), (3, (9, 10, 11)), (3, (18, 17, 19)), (3, (33, 32, 30))]:
        for cin, cout, k, s, p, mb in itertools.product((64, 128, 256), (64, 72, 128, 256), (1, 3, 4), (1, 2), (0, 1),
                                                        (0, 1)):
            g = _g(2 if d == 2 else 1, sp, cin, cout, k, s, p, min_blocks=mb)
            if min(g.out_dhw) >= 1:
                yield g


BF16_FAMILY = {0: "gather_conv_bf16_kernel<", 1: "gather_patch_bf16_kernel<", 2: "gather_conv_bf16_wide_kernel<2, 4,",
               3: "gather_conv_bf16_wide_kernel<4, 2,", 4: "gather_conv_bf16_wide_kernel<2, 4,",
               5: "gather_patch8_bf16_kernel<"}


def test_bf16_label_code_and_rows_agree():
    seen = set()
    for g in _bf16_sweep():
        gc = g.c()
        for bwd in (0, 1):
            code = lib().mpgan_conv_variant_bf16(C.byref(gc), bwd)
            name = engine._bf16_kernel_name(g, bool(bwd))
            seen.add(code)
            assert name.startswith(BF16_FAMILY[code]), (g, bwd, code, name)
            assert name.endswith("true>") == (code == 4) or code not in (2, 3, 4), (g, bwd, code, name)
            bn = 128 if (g.cin if bwd else g.cout) > 64 else 64
            if code in (0, 1, 5):
                assert name.startswith(f"{BF16_FAMILY[code]}{bn}"), (g, bwd, name)
        fwd_rows, bwd_rows = lib().mpgan_conv_stats_rows_bf16(C.byref(gc)), lib().mpgan_conv_bwd_stats_rows_bf16(C.byref(gc))
        assert fwd_rows > 0
        bcode = lib().mpgan_conv_variant_bf16(C.byref(gc), 1)
        assert (bwd_rows == 0) == (bcode == 0), (g, bcode, bwd_rows)      # the narrow kernel has no fused sums
        if lib().mpgan_conv_variant_bf16(C.byref(gc), 0) == 5:            # one statistics row per 8 x 8 x 8 tile
            o = g.out_dhw
            assert fwd_rows == g.n * ((o[0] + 7) // 8) * ((o[1] + 7) // 8) * ((o[2] + 7) // 8)
    assert seen == set(BF16_FAMILY), seen


def test_fp32_label_and_code_agree():
    for d, sp in [(2, (40, 36)), (2, (130, 126)), (3, (18, 17, 19))]:
        for cin, cout, k, s, p, tr, pro, mm in itertools.product((1, 16, 32, 64), (1, 16, 64, 128), (3, 4), (1, 2),
                                                                 (0, 1), (False, True), (0, 1, 3), (False, True)):
            g = _g(2, sp, cin, cout, k, s, p, transposed=tr, out_pad=(0, 0, 0), mm_bf16=mm)
            if min(g.out_dhw) < 1:
                continue
            gc = g.c()
            for bwd in (0, 1):
                pc = 0 if bwd else pro
                code = lib().mpgan_conv_variant(C.byref(gc), bwd, pc)
                name = engine.gather_kernel_name(g, bool(bwd), pc != 0, False, pc == 3)
                if code in (1, 2):
                    assert name.startswith(("thin_", "convt_")), (g, bwd, code, name)
                elif code in (16, 17):
                    assert name.startswith(("gather_patch_kernel<", "gather_patch_persist_kernel<")), (g, code, name)
                    assert name.endswith("true>" if code == 17 else "false>"), (g, code, name)
                elif code == 18:
                    assert name.startswith("gather_patch3d_c16_kernel<"), (g, code, name)
                elif name.endswith(", true>") and name.startswith("gather_conv_pipe_kernel<"):   # MM16 instance
                    assert mm and code % 1000 in (32, 64, 128), (g, code, name)
                    assert name.startswith(f"gather_conv_pipe_kernel<{code % 1000},"), (g, code, name)
                else:
                    bn = code % 1000
                    assert name.split("<")[1].startswith(f"{bn},"), (g, code, name)
                    if code >= 3000:
                        assert name.startswith("gather_conv_dma_kernel<"), (g, code, name)
                    elif code >= 2000:
                        assert name.startswith("gather_conv_pipe_kernel<") and name.endswith(", 2, false>"), (g, name)
                    elif code == 1128:
                        assert name == "gather_conv_pipe_kernel<128, 2, 2, 2, 1, 3, true, 1, false>", (g, name)


# The weight gradient (choose_wgrad in conv_wgrad.hip): labels of C3's discriminator (D.conv1 .. conv4; pro code 3 =
# BatchNorm + LeakyReLU(0.2) of the producer) and of C5's generator (MM16 pipelined, 3-D patch and generic forms) and
# discriminator (D.conv1 with a bf16 dy), as the launches of the parent's steps ran them.
WGRAD_LABELS = [
    (_g(16, (256, 256), 1, 64, 3, 1, 0), 0, False, "wgrad_thin_rows_kernel<9, false>"),
    (_g(16, (254, 254), 64, 128, 3, 1, 0), 3, False, "wgrad_pipe_kernel<128, 128, 2, 2, 2, 3, false, false>"),
    (_g(16, (252, 252), 128, 256, 4, 2, 0), 3, False, "wgrad_pipe_kernel<128, 128, 2, 2, 2, 3, false, false>"),
    (_g(16, (125, 125), 256, 256, 4, 2, 0), 3, False, "wgrad_pipe_kernel<128, 128, 2, 2, 2, 3, false, false>"),
    (_g(4, (32, 32, 32), 32, 32, 3, 1, 1, mm_bf16=True), 1, False, "wgrad_pipe_kernel<32, 128, 1, 1, 4, 1, true, true>"),
    (_g(4, (16, 16, 16), 192, 32, 3, 2, 1, transposed=True, out_pad=(1, 1, 1), mm_bf16=True), 0, False,
     "wgrad_pipe_kernel<128, 128, 2, 2, 2, 0, true, true>"),
    (_g(4, (64, 64, 64), 16, 16, 3, 1, 1, mm_bf16=True), 1, False, "wgrad_patch3d_c16_kernel<true, true>"),
    (_g(4, (64, 64, 64), 32, 1, 3, 2, 1, transposed=True, out_pad=(1, 1, 1), mm_bf16=True), 0, False,
     "wgrad_kernel<32, 32, 1, 1, 1, 4, false, true>"),
    (_g(4, (128, 128, 128), 1, 64, 3, 1, 0), 0, True, "wgrad_thin_rows_kernel<27, true>"),
]


def _wgrad_label(g, pro_code, bf16_dy):
    gc = g.c()
    return engine.kernel_label(lib().mpgan_conv_wgrad_kernel_name, C.byref(gc), pro_code, int(bf16_dy))


@pytest.mark.parametrize("i", range(len(WGRAD_LABELS)))
def test_wgrad_labels(i):
    g, pro_code, bf16_dy, label = WGRAD_LABELS[i]
    assert _wgrad_label(g, pro_code, bf16_dy) == label


def _library_kernels():
    from mpgan_amd import _lib
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "no nm on PATH"
    out = subprocess.run([nm, "-C", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"void mpgan::(\w+<[^()]*>)\(mpgan::WgradParams", out))


def test_wgrad_labels_name_library_kernels():
    kernels = _library_kernels()
    seen = set()
    for d, sp in [(2, (40, 36)), (2, (130, 126)), (3, (18, 17, 19)), (3, (34, 33, 32))]:
        for cin, cout, (k, s, p), tr, mm in itertools.product((1, 16, 32, 64, 128), (1, 16, 32, 64, 128),
                                                             [(1, 1, 0), (3, 1, 1), (3, 1, 0), (3, 2, 1), (4, 2, 1)],
                                                             (False, True), (False, True)):
            op = (1, 1, 1) if tr and (k, s) == (3, 2) else (0, 0, 0)
            g = _g(2, sp, cin, cout, k, s, p, transposed=tr, out_pad=op, mm_bf16=mm)
            if min(g.out_dhw) < 1:
                continue
            for pro_code in ((0,) if tr else (0, 1, 2, 3)):
                name = _wgrad_label(g, pro_code, False)
                assert name.startswith("wgrad") and name in kernels, (g, pro_code, name)
                seen.add(name.split("<")[0])
            if not tr and cin == 1 and cout % 4 == 0 and cout <= 64 and k != 4:   # what the bf16-dy entry takes
                name = _wgrad_label(g, 0, True)
                assert name.startswith("wgrad") and name in kernels and name.endswith(", true>"), (g, name)
    assert seen == {"wgrad_patch3d_c16_kernel", "wgrad_patch2d_kernel", "wgrad_thin_rows_kernel", "wgrad_thin_kernel",
                    "wgrad_pipe_kernel", "wgrad_kernel"}, seen


def _fp32_sweep():
    for sp in [(40, 36), (130, 126), (13, 21), (18, 17, 19), (34, 33, 32)]:
        for cin, cout, (k, s, p), tr, mm, mb in itertools.product(
                (1, 16, 32, 64, 128, 192), (1, 8, 16, 24, 32, 64, 128),
                [(1, 1, 0), (3, 1, 1), (3, 1, 0), (3, 2, 1), (4, 2, 1), (2, 1, 0)], (False, True), (False, True), (0, 1)):
            # a transposed k3 s2 layer doubles its extent: output padding 1 in every dimension it strides
            op = ((1, 1, 1) if len(sp) == 3 else (0, 1, 1)) if tr and (k, s) == (3, 2) else (0, 0, 0)
            g = _g(2, sp, cin, cout, k, s, p, transposed=tr, out_pad=op, mm_bf16=mm, min_blocks=mb)
            if min(g.out_dhw) >= 1:
                yield g


def test_fp32_labels_name_library_kernels():
    # every label the fp32 gather choice prints is an instance the library holds, whatever the form
    from mpgan_amd import _lib
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "no nm on PATH"
    out = subprocess.run([nm, "-C", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    kernels = set(re.findall(r"void mpgan::(\w+(?:<[^()]*>)?)\(mpgan::GatherConv", out))
    seen, labels = set(), set()
    for g in _fp32_sweep():
        gc = g.c()
        for pro_code, bwd in itertools.product((0, 1, 2, 3), (0, 1)):
            labels.add(engine.kernel_label(lib().mpgan_conv_kernel_name, C.byref(gc), bwd, pro_code))
    for name in labels:
        assert name in kernels, name
        seen.add(name.split("_kernel")[0])
    assert seen == {"thin_cin1", "thin_cin1_full", "thin_cin1_rows", "thin_cout1", "thin_c1c1_rows4", "convt_quad_cout1",
                    "convt_oct_cout1", "gather_patch", "gather_patch_persist", "gather_patch3d_c16", "gather_conv_pipe",
                    "gather_conv_dma", "gather_conv"}, seen
