#!/usr/bin/env python3
"""Dump what the fp32 gather dispatcher decides over a sweep of geometries: one line per (geometry, direction,
prologue code) with mpgan_conv_variant, mpgan_conv_stats_rows, mpgan_conv_acc_supported, mpgan_conv_fold_supported,
mpgan_conv_bwd_stats_rows and the kernel label.  Library queries only: no GPU.

    python tools/dump_conv_choices.py OUT.txt
    MPGAN_LIB_PATH=.../libmpgan_hip_dev.so MPGAN_DBG_NO_MERGE=1 python tools/dump_conv_choices.py OUT.txt

Two libraries decide the same when their dumps are byte-identical (a host-side refactor of conv_igemm.hip: compare the
parent's library with the new one, product and DEV build, the DEV build once per MPGAN_DBG_* form switch -- the switches
are read once per process).  The sweep is the one of tests/test_conv_choice.py::test_fp32_labels_name_library_kernels.
"""
import ctypes as C
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mpgan_amd import engine, ops      # noqa: E402
from mpgan_amd._lib import lib          # noqa: E402

EXTENTS = [(40, 36), (130, 126), (13, 21), (18, 17, 19), (34, 33, 32)]
KSP = [(1, 1, 0), (3, 1, 1), (3, 1, 0), (3, 2, 1), (4, 2, 1), (2, 1, 0)]


def sweep():
    for sp in EXTENTS:
        d3 = len(sp) == 3
        t = (lambda v, fill: (v,) * 3 if d3 else (fill, v, v))
        for cin, cout, (k, s, p), tr, mm, mb in itertools.product((1, 16, 32, 64, 128, 192), (1, 8, 16, 24, 32, 64, 128),
                                                                  KSP, (False, True), (False, True), (0, 1)):
            op = t(1, 0) if tr and (k, s) == (3, 2) else (0, 0, 0)
            g = ops.ConvGeom(2, sp if d3 else (1,) + sp, cin, cout, t(k, 1), t(s, 1), t(p, 0), transposed=tr, out_pad=op,
                             mm_bf16=mm, min_blocks=mb)
            if min(g.out_dhw) >= 1:
                yield g


def main():
    L = lib()
    n = 0
    with open(sys.argv[1], "w") as f:
        for g in sweep():
            gc = g.c()
            r = C.byref(gc)
            for pro, bwd in itertools.product((0, 1, 2, 3), (0, 1)):
                label = engine.kernel_label(L.mpgan_conv_kernel_name, r, bwd, pro)
                f.write("%s %s cin%d cout%d k%d s%d p%d tr%d mm%d mb%d pro%d bwd%d | %d %d %d %d %d %s\n" % (
                    "x".join(map(str, g.in_dhw)), "x".join(map(str, g.out_dhw)), g.cin, g.cout, g.k[2], g.stride[2],
                    g.pad[2], g.transposed, g.mm_bf16, g.min_blocks, pro, bwd, L.mpgan_conv_variant(r, bwd, pro),
                    L.mpgan_conv_stats_rows(r, pro), L.mpgan_conv_acc_supported(r, pro), L.mpgan_conv_fold_supported(r),
                    L.mpgan_conv_bwd_stats_rows(r), label))
                n += 1
    print("%d queries -> %s (%s)" % (n, sys.argv[1], os.environ.get("MPGAN_LIB_PATH", "product library")))


if __name__ == "__main__":
    main()
