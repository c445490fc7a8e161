"""The case table of the weight-gradient kernel instances (csrc/conv_wgrad.hip and the MM16 half of csrc/conv_mm16.hip:
what choose_wgrad picks between), with the operands, the fp64 reference and the checks every case is held to.

One table serves three files: tests/test_wgrad_forms.py reads every case's label on the host (fake pointers),
tests/test_wgrad_forms_gpu.py launches every case and compares it with the reference in both tiers of tests/conv_ref.py,
and tests/test_wgrad_planted.py shows on the host that those comparisons reject planted faults.  tools/wgrad_forms_table.py
prints the table of DESIGN.md section 8.3 from it.  Nothing in here needs a GPU: operands and references are CPU tensors.

Shapes are the smallest that still hold a form's failure points (the `why` of each case names them):
  M%32   M = N Mz My Mx is no multiple of WBK = 32          split   M >= 512, no multiple of 256: nsplit >= 2, ragged last
  nb     a sample boundary inside a chunk (N >= 2)          rag     Cd no multiple of BD / T Cg no multiple of BG
  odd    odd extents, padding on every side                 s2odd   stride 2 on an odd input extent
  narrow slabs >= 64 and Cd Cg T <= 16384: the narrow reducer (every other case: the wide one)
  cap    more tiles than the persistent form's block cap    rtile   ragged 8x16 / 8x8 / 2x8x8 tiles
  row    a chunk boundary inside a row                      fold2   two fold rounds        lds>64K   the raised LDS limit
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import re
import shutil
import subprocess
from typing import Optional, Tuple

import torch

import conv_ref as R

TILE = {(128, 128): (2, 2, 2, 1), (128, 64): (1, 2, 1, 1), (128, 32): (1, 1, 1, 1), (64, 128): (2, 1, 4, 1),
        (64, 64): (1, 1, 2, 1), (64, 32): (2, 1, 1, 4), (32, 128): (1, 1, 4, 1), (32, 64): (1, 2, 1, 4),
        (32, 32): (1, 1, 1, 4)}
PIPE_TILES = [t for t, w in TILE.items() if w[3] == 1]        # one wave per K-step: the tiles the pipelined form has
PROS = (None, "ch", "nc", "leaky", "leaky_hi", "leaky_ptr")
HI_SLOPE = 2.0                                                # a host slope outside [0, 1] (dyadic: tier X stays exact)


def b(v):
    return "true" if v else "false"


def generic_label(bd, bg, sd, sg):
    tm, tn, wn, kw = TILE[bd, bg]
    return f"wgrad_kernel<{bd}, {bg}, {tm}, {tn}, {wn}, {kw}, {b(sd)}, {b(sg)}>"


def pipe_label(bd, bg, pro, pad, mm16):
    tm, tn, wn, _ = TILE[bd, bg]
    return f"wgrad_pipe_kernel<{bd}, {bg}, {tm}, {tn}, {wn}, {pro}, {b(pad)}, {b(mm16)}>"


def geom(n, spatial, cin, cout, k, s, p, tr=False, op=0, mm=False):
    """ops.ConvGeom of a 2-D (spatial (H, W)) or 3-D layer; k / s / p / op an int or a full (z, y, x) triple."""
    from mpgan_amd import ops
    d = len(spatial)
    t = (lambda v, fill: tuple(v) if not isinstance(v, int) else ((v,) * 3 if d == 3 else (fill, v, v)))
    sp = tuple(spatial) if d == 3 else (1,) + tuple(spatial)
    return ops.ConvGeom(n, sp, cin, cout, t(k, 1), t(s, 1), t(p, 0), transposed=tr, out_pad=t(op, 0), mm_bf16=mm)


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    g: object                                  # ops.ConvGeom
    label: str
    x: Tuple[Optional[int], int] = (None, 0)   # (pitch or None = compact, offset in elements from a 16-byte aligned base)
    dy: Tuple[Optional[int], int] = (None, 0)
    pro: Optional[str] = None                  # one of PROS
    pro_off: Tuple[int, int] = (0, 0)          # offsets (floats) of the prologue's scale and shift from an aligned base
    entry: str = "f32"                         # f32: conv_backward_weight; bf16dy: .._bf16dy; 2p / 2p_bf16: conv2p_..
    dbias: bool = True
    why: str = ""                              # the predicates of choose_wgrad and the failure points the shapes hold
    slabs: Optional[int] = None                # asserted through the workspace query where the case is about the reducer

    @property
    def bf16_dy(self):
        return self.entry in ("bf16dy", "2p_bf16")

    @property
    def mm16(self):
        """The instance rounds its matrix operands to bf16."""
        return bool(re.search(r"wgrad_pipe_kernel<.*, true>$|wgrad_patch3d_c16_kernel<\w+, true>$", self.label))

    @property
    def M(self):
        g = self.g
        e = g.in_dhw if g.transposed else g.out_dhw
        return g.n * e[0] * e[1] * e[2]


# ---------------------------------------------------------------------------------------------------------- the table
K23, P23 = (1, 2, 3), (0, 1, 1)          # a 2 x 3 kernel: T Cg <= 32 with Cg % 4 == 0
S1 = dict(spatial=(19, 21), k=3, s=1, p=1)                  # out 19 x 21, M = 798 = 24 * 32 + 30: three chunks of 288
S2 = dict(spatial=(37, 41), k=3, s=2, p=1)                  # the same output from an odd input under stride 2
KS = "M%32 split nb odd"


def _generic_cases():
    """All 36 wgrad_kernel instances.  Cd / Cg and the layout give SCALAR_D / SCALAR_G through each of their causes in
    turn (channel count % 4, pitch % 4, base off by one float); the one-wave-per-K-step tiles reach <false, false> only
    through a per-(sample, channel) prologue (vector operands otherwise run the pipelined form)."""
    dense = {32: (24, 22), 64: (40, 42), 128: (72, 130)}       # BD: Cd % 4 == 0 / != 0, never a multiple of BD
    gath = {32: ((4, K23, P23), (3, 3, 1)), 64: ((4, 3, 1), (6, 3, 1)), 128: ((12, 3, 1), (10, 3, 1))}
    out = []
    for i, (bd, bg) in enumerate(TILE):
        kw = TILE[bd, bg][3]
        for sd in (False, True):
            for sg in (False, True):
                cause_d, cause_g = ("chan", "pitch", "base")[i % 3], ("base", "chan", "pitch")[i % 3]
                cd = dense[bd][1] if sd and cause_d == "chan" else dense[bd][0]
                cg, k, p = gath[bg][1] if sg and cause_g == "chan" else gath[bg][0]
                lay = {"chan": (None, 0), "pitch": None, "base": (None, 1)}
                dyl = (lay[cause_d] or (cd + 5, 0)) if sd else ((cd + 8, 4) if i % 2 else (None, 0))
                xl = (lay[cause_g] or (cg + 3, 0)) if sg else ((cg + 4, 8) if i % 2 == 0 else (None, 0))
                pro = "nc" if (kw == 1 and not sd and not sg) else PROS[(i + 2 * sd + sg) % 6]
                sp = dict(S2 if (i + sd) % 2 else S1)
                sp.update(k=k, p=p)
                why = [KS, "rag", f"Cd {cd} Cg {cg}", "s2odd" if sp["s"] == 2 else "s1"]
                if sd:
                    why.append(f"SCALAR_D by {cause_d}")
                if sg:
                    why.append(f"SCALAR_G by {cause_g}")
                if kw == 4:
                    why.append("kw 4: never pipelined")
                elif not sd and not sg:
                    why.append("vector operands kept off the pipelined form by n_stride != 0")
                out.append(Case(f"generic-{bd}x{bg}-{'s' if sd else 'v'}{'s' if sg else 'v'}",
                                geom(2, sp["spatial"], cg, cd, sp["k"], sp["s"], sp["p"]), generic_label(bd, bg, sd, sg),
                                x=xl, dy=dyl, pro=pro, dbias=(i + sd + sg) % 4 != 0, why=", ".join(why)))
    return out


def _pipe_cases(mm):
    """The pipelined instances: six padded tiles x PRO 0 / 1 and the pad-free 128 x 128 tile at PRO 0 / 1 (/ 3: fp32 only)."""
    dense = {32: 24, 64: 40, 128: 72}
    gath = {32: (4, K23, P23), 64: (4, 3, 1), 128: (12, 3, 1)}
    tag = "mm16" if mm else "pipe"
    out = []
    for i, (bd, bg) in enumerate(PIPE_TILES):
        for pro in (0, 1):
            cd, (cg, k, p) = dense[bd], gath[bg]
            sp = dict(S2 if (i + pro) % 2 else S1)
            sp.update(k=k, p=p)
            kind = (None if not pro else ("ch", "leaky", "leaky_ptr", "leaky_hi")[i % 4])
            sl = (i + pro) % 2 == 0                 # operands as 16-byte aligned channel slices of wider buffers
            out.append(Case(f"{tag}-{bd}x{bg}-pro{pro}", geom(2, sp["spatial"], cg, cd, sp["k"], sp["s"], sp["p"], mm=mm),
                            pipe_label(bd, bg, pro, True, mm), x=(cg + 8, 4) if sl else (None, 0),
                            dy=(cd + 4, 8) if sl else (None, 0), pro=kind, dbias=(i + pro) % 3 != 0,
                            why=f"{KS}, rag, Cd {cd} Cg {cg}, {'s2odd' if sp['s'] == 2 else 's1'}, padded"
                                + (", aligned slices" if sl else "") + (f", prologue {kind}" if kind else "")))
    # pad-free 128 x 128: a valid 3x3 conv, two dense tiles (Cd 132) and two gathered ones (T Cg = 216)
    nopad = dict(spatial=(21, 23), k=3, s=1, p=0)            # out 19 x 21
    for pro, kind in ((0, None), (1, "ch"), (3, "leaky")) if not mm else ((0, None), (1, "leaky")):
        out.append(Case(f"{tag}-128x128-nopad-pro{pro}", geom(2, nopad["spatial"], 24, 132, 3, 1, 0, mm=mm),
                        pipe_label(128, 128, pro, False, mm), pro=kind, dy=(136, 4) if pro else (None, 0),
                        why=f"{KS}, rag, two tiles each way, pad 0" + (f", prologue {kind}" if kind else "")))
    if not mm:   # LeakyReLU kinds that must NOT take PRO 3 at the pad-free tile
        out.append(Case("pipe-128x128-nopad-slope-ptr", geom(2, nopad["spatial"], 24, 132, 3, 1, 0),
                        pipe_label(128, 128, 1, False, False), pro="leaky_ptr", why=f"{KS}, slope_ptr keeps PRO 1"))
        out.append(Case("pipe-128x128-nopad-slope-hi", geom(2, nopad["spatial"], 24, 132, 3, 1, 0),
                        pipe_label(128, 128, 1, False, False), pro="leaky_hi", dbias=False,
                        why=f"{KS}, host slope outside [0, 1] keeps PRO 1"))
    # slabs >= 64: 2 x 95 x 97 = 18430 pixels in 64 chunks of 288; the narrow reducer
    out.append(Case(f"{tag}-32x128-narrow", geom(2, (95, 97), 12, 24, 3, 1, 1, mm=mm), pipe_label(32, 128, 1, True, mm),
                    pro="ch", why="narrow: 64 slabs, nb, odd", slabs=64))
    # transposed, 3-D, k3 s2 p1 with output padding 1: dense = x (24 channels), gathered = dy (12 channels, 324 columns)
    out.append(Case(f"{tag}-convT3d", geom(2, (5, 7, 9), 24, 12, 3, 2, 1, tr=True, op=1, mm=mm),
                    pipe_label(32, 128, 0, True, mm), dbias=False, why="transposed 3-D k3 s2 p1 op1, M 630: M%32 split nb odd"))
    return out


def _patch_cases():
    out = []
    # 3-D 16 -> 16 3x3x3 stride 1: <HAS_PRO, MM16>; ragged 2 x 8 x 8 tiles everywhere
    for pro in (False, True):
        for mm in (False, True):
            pad = 1 if pro == mm else 0
            sp = (5, 17, 11) if pad else (7, 19, 13)
            out.append(Case(f"patch3d-{'pro' if pro else 'nopro'}-{'mm16' if mm else 'f32'}",
                            geom(2, sp, 16, 16, 3, 1, pad, mm=mm), f"wgrad_patch3d_c16_kernel<{b(pro)}, {b(mm)}>",
                            pro="leaky_ptr" if pro else None, dbias=not (pro and mm),
                            x=(24, 4) if mm else (None, 0), dy=(None, 0) if mm else (20, 4),
                            why=f"pad {pad}, rtile 2x8x8, 36 tiles: wide reducer, nb, odd, M%32", slabs=36))
    out.append(Case("patch3d-cap", geom(2, (9, 65, 65), 16, 16, 3, 1, 1), "wgrad_patch3d_c16_kernel<true, false>", pro="ch",
                    why="cap: 810 tiles on 512 blocks, narrow reducer", slabs=512))
    # 2-D patch form: <CD, CG, S, TX, HAS_PRO>
    for cd, cg, s, tx in ((16, 16, 1, 16), (32, 32, 1, 16), (32, 16, 2, 16), (64, 16, 2, 8)):
        for pro in (False, True):
            sp = (19, 21) if s == 1 else (37, 41)
            sl = pro == (s == 1)
            out.append(Case(f"patch2d-{cd}x{cg}s{s}-{'pro' if pro else 'nopro'}", geom(2, sp, cg, cd, 3, s, 1),
                            f"wgrad_patch2d_kernel<{cd}, {cg}, {s}, {tx}, {b(pro)}>", pro=("ch", "leaky")[s - 1] if pro else None,
                            x=(cg + 4, 4) if sl else (None, 0), dy=(cd + 8, 8) if sl else (None, 0), dbias=not (pro and s == 2),
                            why=f"rtile 8x{tx}, {'s2odd' if s == 2 else 's1'}, odd, nb, M%32, below the cap"
                                + (", aligned slices" if sl else "")))
    out.append(Case("patch2d-32x32s1-cap", geom(3, (56, 104), 32, 32, 3, 1, 1), "wgrad_patch2d_kernel<32, 32, 1, 16, true>",
                    pro="ch", why="cap: 147 tiles on 128 blocks, narrow reducer", slabs=128))
    out.append(Case("patch2d-convT-64x16", geom(2, (9, 11), 64, 16, 3, 2, 1, tr=True, op=(0, 1, 1)),
                    "wgrad_patch2d_kernel<64, 16, 2, 8, false>", dbias=False,
                    why="transposed 2-D k3 s2 p1 op1 (out = 2 in), rtile 8x8, odd"))
    return out


def _thin_cases():
    out = []
    T = {1: (1, 0), 9: (3, 1), 27: (3, 1)}
    # pixels per sample and chunk: T 1 2173 / 1449, T 9 1517 / 1012, T 27 1755 / 878: chunk boundaries inside rows
    sp1, sp2, sp3 = (53, 41), (37, 41), (9, 13, 15)
    for t in (1, 9, 27):
        k, p = T[t]
        sp = {1: sp1, 9: sp2, 27: sp3}[t]
        cd4 = 16 if t == 27 else 8
        out.append(Case(f"thin-v4-t{t}", geom(2, sp, 1, cd4, k, 1, p), f"wgrad_thin_kernel<4, {t}, false>",
                        dy=(cd4 + 4, 4) if t == 9 else (None, 0), dbias=t != 1,
                        why=f"Cg 1, Cd {cd4}, row, nb, odd, M%32" + (", fold2" if t == 27 else "")))
        cause = {1: "chan", 9: "pitch", 27: "base"}[t]
        cd1 = 6 if cause == "chan" else 8
        out.append(Case(f"thin-v1-t{t}", geom(2, sp, 1, cd1, k, 1, p), f"wgrad_thin_kernel<1, {t}, false>",
                        dy={"chan": (None, 0), "pitch": (11, 0), "base": (None, 1)}[cause], dbias=t != 27,
                        why=f"Cg 1, Cd {cd1}, scalar dense lanes by {cause}, row, nb, odd"))
        cdb = 64 if t == 27 else 12
        out.append(Case(f"thin-bf16dy-t{t}", geom(2, sp if t != 27 else (5, 9, 11), 1, cdb, k, 1, p),
                        f"wgrad_thin_kernel<4, {t}, true>", entry="bf16dy", dy=(cdb + 4, 4) if t == 1 else (None, 0),
                        dbias=t != 9, why=f"bf16 dy, Cd {cdb}" + (", pad 1 keeps it off the row walker, lds>64K" if t == 27 else ", row, nb")))
    out.append(Case("thin-convT2d", geom(2, (17, 19), 8, 1, 3, 2, 1, tr=True, op=(0, 1, 1)), "wgrad_thin_kernel<4, 9, false>",
                    dbias=False, why="transposed 2-D k3 s2 p1 op1: dense = x (8 channels), gathered = dy (1 channel)"))
    out.append(Case("thin-convT3d", geom(2, (5, 7, 9), 16, 1, 3, 2, 1, tr=True, op=1), "wgrad_thin_kernel<4, 27, false>",
                    dbias=False, why="transposed 3-D k3 s2 p1 op1, fold2"))
    out.append(Case("thin-narrow", geom(2, (181, 183), 1, 8, 3, 1, 1), "wgrad_thin_kernel<4, 9, false>",
                    why="narrow: 65 blocks of 1020 pixels", slabs=65))
    # the row walkers: 1 -> 64, pad-free stride 1, compact x
    # (wgrad_thin_rows_kernel<27, false> is not in the table: UNREACHABLE below)
    for t, bf in ((9, False), (9, True), (27, True)):
        sp = (232, 7) if t == 9 else (11, 33, 6)            # Mx = 5 (2-D) and Mx = 4 (3-D); three blocks each
        out.append(Case(f"thinrows-t{t}-{'bf16dy' if bf else 'f32'}", geom(2, sp, 1, 64, 3, 1, 0),
                        f"wgrad_thin_rows_kernel<{t}, {b(bf)}>", entry="bf16dy" if bf else "f32",
                        dy=(72, 8) if bf and t == 9 else ((None, 0) if bf else (67, 1)), dbias=not (bf and t == 27),
                        why=f"Mx {5 if t == 9 else 4}, row, nb, odd" + ("" if bf else ", dy pitch 67 off by one float")))
    out.append(Case("thinrows-narrow", geom(2, (183, 185), 1, 64, 3, 1, 0), "wgrad_thin_rows_kernel<9, false>",
                    why="narrow: 65 blocks, Cd Cg T = 576", slabs=65))
    for t, bf in ((9, False), (27, False), (9, True), (27, True)):
        sp = (231, 6) if t == 9 else (11, 33, 7)
        out.append(Case(f"thin2rows-t{t}-{'bf16dy' if bf else 'f32'}", geom(2, sp, 2, 64, 3, 1, 0),
                        f"wgrad_thin2_rows_kernel<{t}, {b(bf)}>", entry="2p_bf16" if bf else "2p",
                        dy=(68, 4) if t == 27 else (None, 0), dbias=not (bf and t == 9),
                        why=f"two planes, Mx {4 if t == 9 else 5}, row, nb, odd"))
    out.append(Case("thin2rows-narrow", geom(2, (183, 185), 2, 64, 3, 1, 0), "wgrad_thin2_rows_kernel<9, false>", entry="2p",
                    why="narrow: 65 blocks, Cd Cg T = 1152", slabs=65))
    return out


def _extra_cases():
    """Causes of a scalar gathered operand that only the prologue has, the fold-round refusal, the wave-split-K tiles at
    slabs >= 64, and the C5 generator's ConvTranspose 32 -> 1."""
    return [
        Case("generic-scale-off", geom(2, (19, 21), 12, 72, 3, 1, 1), generic_label(128, 128, False, True), pro="ch",
             pro_off=(1, 0), why=f"{KS}, SCALAR_G by the prologue's scale off by one float"),
        Case("generic-shift-off", geom(2, (19, 21), 12, 40, 3, 1, 1), generic_label(64, 128, False, True), pro="leaky",
             pro_off=(0, 3), why=f"{KS}, SCALAR_G by the prologue's shift off by three floats"),
        Case("generic-nstride", geom(2, (19, 21), 12, 24, 3, 1, 1), generic_label(32, 128, False, False), pro="nc",
             x=(16, 4), why=f"{KS}, per-(sample, channel) prologue on an aligned slice"),
        Case("generic-nstride-odd", geom(3, (19, 21), 6, 24, 3, 1, 1), generic_label(32, 64, False, True), pro="nc",
             why="three samples, n_stride 6"),
        Case("generic-fold-refusal", geom(2, (5, 9, 11), 1, 64, 3, 1, 1), generic_label(64, 32, False, True),
             why="Cg 1, Cd 64, T 27: two fold rounds with Cd > 16 leave the thin form; M 990"),
        Case("generic-32x32-narrow", geom(2, (47, 49), 3, 24, 3, 1, 1), generic_label(32, 32, False, True), pro="ch",
             why="narrow: 16 splits x 4 wave slabs = 64", slabs=64),
        # 3-D ConvNd through the K-stepped forms (depth taps and depth padding), and the discriminator's 4x4 stride-2 kernel
        Case("pipe-3d", geom(2, (5, 7, 9), 8, 40, 3, 1, 1), pipe_label(64, 128, 1, True, False), pro="leaky",
             why="3-D 3x3x3 pad 1, M 630: M%32 split nb odd, rag"),
        Case("mm16-3d-s2", geom(2, (9, 13, 15), 8, 40, 3, 2, 1, mm=True), pipe_label(64, 128, 0, True, True),
             why="3-D 3x3x3 stride 2 on odd input, M 560: split nb s2odd, rag"),
        Case("generic-3d-s2", geom(2, (9, 13, 15), 6, 40, 3, 2, 1), generic_label(64, 128, False, True), pro="ch", x=(9, 1),
             why="3-D 3x3x3 stride 2 on odd input, SCALAR_G by chan, pitch and base"),
        Case("pipe-128x128-nopad-k4s2", geom(2, (40, 44), 24, 72, 4, 2, 0), pipe_label(128, 128, 3, False, False),
             pro="leaky", why=f"{KS}, 4x4 stride 2 pad 0 (T Cg = 384: three gathered tiles), PRO 3"),
        Case("generic-convT3d-32to1", geom(2, (5, 7, 9), 32, 1, 3, 2, 1, tr=True, op=1), generic_label(32, 32, False, True),
             dbias=False, why="transposed 3-D k3 s2 p1 op1, Cd 32 Cg 1 (two fold rounds, Cd > 16)"),
    ]


# Instances the library holds that no public entry can reach, with the line of choose_wgrad's path that proves it.
UNREACHABLE = {
    "wgrad_thin_rows_kernel<27, false>":
        "thin_rows_ok needs Cd == 64 and T == 27; the fp32 entry takes a thin form only if plan_thin_wgrad's ok holds "
        "(`} else if (bf16_dy || (tp.ok && kshape && !no_thin)) {`), and plan_thin_wgrad clears it for this shape: V = 4 "
        "lane rows of 64 * 28 floats are 112 KiB > the 64 KiB fp32 cap, so thin_fold_rounds gives 2 and "
        "`if (rounds > 1 && Cd > 16) t.ok = false;`.  Only the bf16-dy entry (cap 150 KiB) walks 3x3x3 rows.",
}

# What admits a launch to each form, in choose_wgrad's order of precedence (the first form that admits it serves it).
ADMISSION = {
    "wgrad_thin2_rows_kernel": "mpgan_conv2p_backward_weight only: ConvNd 2 -> 64 over two 1-channel planes, 3x3 or 3x3x3, "
                               "stride 1, pad 0, Mx >= 4 (else refused).  <T, dy is bf16>",
    "wgrad_patch3d_c16_kernel": "fp32 dy; ConvNd 16 -> 16, 3x3x3, stride 1, pad 0 or 1 per dimension, out >= (2, 4, 4); both "
                                "operands and the prologue read as 16-byte vectors (pitches % 4, 16-byte aligned bases, "
                                "per-channel prologue).  <prologue given, mm_bf16>",
    "wgrad_patch2d_kernel": "fp32 dy; 1x3x3, pad 1, depth 1, stride 1 with (Cd, Cg) = (16, 16) or (32, 32), stride 2 with "
                            "(32, 16) or (64, 16) -- a ConvNd, or a ConvTransposeNd with out = 2 in -- My, Mx >= 4; 16-byte "
                            "vectors as above.  <Cd, Cg, S, tile width, prologue given>",
    "wgrad_thin_rows_kernel": "a thin launch (next row) with Cd == 64, T in {9, 27}, stride 1, pad 0, Mx >= 4, compact x "
                              "(ldg == 1).  <T, dy is bf16>",
    "wgrad_thin_kernel": "the bf16-dy entry always (it refuses Cd % 4, ldd % 4, dy off 8 bytes, other kernels, Cd > 64); "
                         "fp32: Cg == 1, no prologue, Cd <= 64, kernel 1 / 3x3 / 3x3x3, lane rows within 64 KiB after at "
                         "most one halving, and two fold rounds only for Cd <= 16.  <V = 4 if Cd % 4 == 0, ldd % 4 == 0 "
                         "and dy 16-byte aligned else 1, T, dy is bf16>",
    "wgrad_pipe_kernel": "the K-stepped tile BD x BG by Cd and T Cg (<= 32, <= 64, more) has one wave per K-step (not "
                         "32x32, 64x32, 32x64); vector operands (Cd % 4, Cg % 4, pitches % 4, aligned bases, prologue "
                         "vectors aligned); operands below 4 GiB; no per-(sample, channel) prologue.  MM16 = mm_bf16.  PAD = "
                         "false at the 128 x 128 tile of a pad-free conv; PRO 3 there for LeakyReLU with a host slope in "
                         "[0, 1] (fp32 operands only), else PRO = prologue given.",
    "wgrad_kernel": "everything else.  SCALAR_D / SCALAR_G: that operand fails Cd (Cg) % 4, pitch % 4 or base alignment "
                    "(gathered: or a prologue vector is misaligned, or n_stride % 4).",
}


def family(label):
    return label.split("<")[0]


def design_table():
    """The form -> admission -> cases table of DESIGN.md's weight-gradient test section (tools/wgrad_forms_table.py
    prints it, tests/test_wgrad_forms.py holds DESIGN.md to it)."""
    symbols = sorted({c.label for c in CASES} | set(UNREACHABLE))
    rows = ["| kernel | admitted when | instances launched | cases (tests/wgrad_cases.py) |", "|---|---|---|---|"]
    for fam, text in ADMISSION.items():
        mine = [c for c in CASES if family(c.label) == fam]
        labels = {c.label for c in mine}
        total = sum(1 for s in symbols if family(s) == fam)
        groups = {}
        for c in mine:
            groups.setdefault(c.id.split("-")[0], []).append(c.id)
        special = [c.id for c in mine if (c.slabs or 0) >= 64 or c.g.transposed]
        ids = ", ".join(f"`{p}-*` ({len(v)})" for p, v in groups.items())
        if special:
            ids += "; reducer / cap / transposed: " + ", ".join(f"`{i}`" for i in special)
        dead = [s for s in UNREACHABLE if family(s) == fam]
        count = f"{len(labels)} of {total}" + (f" (`{'`, `'.join(dead)}` unreachable)" if dead else "")
        rows.append(f"| `{fam}` | {text} | {count} | {ids} |")
    return "\n".join(rows)


CASES = _generic_cases() + _pipe_cases(False) + _pipe_cases(True) + _patch_cases() + _thin_cases() + _extra_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ------------------------------------------------------------------------------------------------------- the library
def library_symbols():
    """Every weight-gradient kernel instance the library holds, as the labels spell them."""
    from mpgan_amd import _lib
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "no nm on PATH"
    out = subprocess.run([nm, "-C", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"void mpgan::(wgrad\w*_kernel<[^()]*>)\(mpgan::WgradParams", out))


A16 = 1 << 20            # a fake 16-byte aligned base


def fake_pro(kind, cin, off=(0, 0)):
    """A prologue struct of fake pointers for one of PROS (a ready struct passes through)."""
    from mpgan_amd._lib import PrologueC
    if kind is None or isinstance(kind, PrologueC):
        return kind
    p = PrologueC()
    p.scale, p.shift = 2 * A16 + 4 * off[0], 3 * A16 + 4 * off[1]
    p.n_stride = cin if kind == "nc" else 0
    p.act = 1 if kind.startswith("leaky") else 0
    p.slope = HI_SLOPE if kind == "leaky_hi" else (0.25 if kind.startswith("leaky") else 1.0)
    p.slope_ptr = 4 * A16 if kind == "leaky_ptr" else None
    return p


def label_at(g, x=(None, 0), dy=(None, 0), pro=None, pro_off=(0, 0), bf16_dy=False, gc=None):
    """(status, label or message) of mpgan_conv_wgrad_kernel_name_at for fake operands of these layouts."""
    from mpgan_amd._lib import lib
    gc = gc if gc is not None else g.c()
    p = fake_pro(pro, g.cin, pro_off)
    buf = C.create_string_buffer(160)
    rc = lib().mpgan_conv_wgrad_kernel_name_at(C.byref(gc), A16 + 4 * x[1], x[0] or g.cin, None if p is None else C.byref(p),
                                               5 * A16 + (2 if bf16_dy else 4) * dy[1], dy[0] or g.cout, int(bf16_dy), buf,
                                               len(buf))
    return rc, (buf.value.decode() if rc == 0 else lib().mpgan_last_error().decode())


def case_label(c: Case):
    """The label the library gives a case's operand layout (host only)."""
    from mpgan_amd import ops
    if c.entry.startswith("2p"):
        return ops.conv2p_wgrad_kernel_name(c.g, c.bf16_dy)
    rc, name = label_at(c.g, c.x, c.dy, c.pro, c.pro_off, c.bf16_dy)
    assert rc == 0, (c.id, rc, name)
    return name


def workspace_bytes(c: Case):
    from mpgan_amd import ops
    return {"f32": ops.conv_wgrad_workspace, "bf16dy": ops.conv_wgrad_workspace_bf16dy, "2p": ops.conv2p_wgrad_workspace,
            "2p_bf16": ops.conv2p_wgrad_workspace}[c.entry](c.g)


def case_slabs(c: Case):
    """The partial slabs of a case's launch, from its workspace: slabs x Cd x T Cg floats and one bias row of Cd floats
    per split (K-stepped forms: kw slabs per split) or per slab.  For a thin or patch form behind the fp32 entry the
    query also covers the K-stepped form, so the table's own count is only checked to fit."""
    g = c.g
    cd, cg = (g.cin, g.cout) if g.transposed else (g.cout, g.cin)
    nc = g.taps * cg
    m = re.match(r"wgrad_(?:pipe_)?kernel<(\d+), (\d+)", c.label)
    kw = TILE[int(m.group(1)), int(m.group(2))][3] if m else 1
    per = 4 * cd * (kw * nc + 1)
    ws = workspace_bytes(c)
    if c.entry == "f32" and not m:      # the fp32 query covers the K-stepped form as well: a lower bound only
        assert ws >= per * c.slabs, (c.id, ws, per)
        return c.slabs
    assert ws % per == 0, (c.id, ws, per)
    return ws // per * kw


# ------------------------------------------------------------------------------------------------ operands, reference
@dataclasses.dataclass
class Operands:
    x: torch.Tensor                    # (N, D, H, W, cin) float32
    dy: torch.Tensor                   # (N, D, H, W, cout) float32 (bf16-representable for a bf16 dy)
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    slope: float
    old_w: torch.Tensor                # dyadic contents of dw / dbias for the beta = 1 launch
    old_b: torch.Tensor


def _ints(shape, gen, density):
    v = torch.randint(-3, 4, shape, generator=gen).float()
    if density < 1.0:
        v = v * (torch.rand(shape, generator=gen) < density)
    return v


def _sign(shape, gen):
    return torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)


def operands(c: Case, tier: str, rounding: bool = False) -> Operands:
    """Tier X: integers in [-3, 3] (thinned so that the magnitude sums stay below R.EXACT_LIMIT), prologue scale +-4,
    integer shift, slope 0.25 (2 where the case asks for a slope outside [0, 1]): every partial sum is dyadic.  Tier R:
    uniform in (-1, 1); an MM16 instance gets an fp32-exact prologue (scale +-2^k, shift 0, slope 0.25: the kernel's
    fp32 prologue then rounds to the bf16 the reference's does).  rounding: tier X operands 2^-9 off their integers,
    which an MM16 instance must round to nearest (the planted-fault test; needs a case without a prologue)."""
    g = c.g
    gen = torch.Generator().manual_seed(1000 + CASES.index(c) * 2 + (tier == "R"))
    in5, out5 = (g.n, *g.in_dhw, g.cin), (g.n, *g.out_dhw, g.cout)
    wshape = (g.cin, g.cout, *g.k) if g.transposed else (g.cout, g.cin, *g.k)
    vshape = (g.n, g.cin) if c.pro == "nc" else (g.cin,)
    leaky = c.pro is not None and c.pro.startswith("leaky")
    scale = shift = None
    if tier == "X":
        rho = min(1.0, math.sqrt(2.0 ** 20 / (90.0 * c.M)))
        x, dy = _ints(in5, gen, rho), _ints(out5, gen, rho)
        if rounding:
            x = x + (x != 0) * _sign(in5, gen) * 2.0 ** -9          # RNE gives the integer back, truncation does not
            dy = dy + (dy != 0) * _sign(out5, gen) * 2.0 ** -9
        slope = HI_SLOPE if c.pro == "leaky_hi" else 0.25
        if c.pro:
            scale = 4.0 * _sign(vshape, gen)
            shift = torch.randint(-2, 3, vshape, generator=gen).float()
    else:
        x, dy = torch.rand(in5, generator=gen) * 2 - 1, torch.rand(out5, generator=gen) * 2 - 1
        slope = HI_SLOPE if c.pro == "leaky_hi" else (0.25 if (c.mm16 or c.pro == "leaky_ptr") else 0.2)
        if c.pro and c.mm16:
            scale = _sign(vshape, gen) * torch.exp2(torch.randint(-1, 2, vshape, generator=gen).float())
            shift = torch.zeros(vshape)
        elif c.pro:
            scale = _sign(vshape, gen) * (torch.rand(vshape, generator=gen) + 0.5)
            shift = (torch.rand(vshape, generator=gen) * 2 - 1) * 0.5
    if c.bf16_dy:
        dy = R.bf16_rne(dy)
    if not leaky:
        slope = 1.0
    return Operands(x, dy, scale, shift, slope, _ints(wshape, gen, 1.0) * 0.5, _ints((g.cout,), gen, 1.0) * 0.5)


@dataclasses.dataclass
class Reference:
    dw: torch.Tensor        # fp64, torch layout
    absref: torch.Tensor
    dw32: torch.Tensor      # the same sums in float32
    db: torch.Tensor        # fp64 (cout,)
    db_mag: torch.Tensor
    L: int


def activated(c: Case, o: Operands, dtype=torch.float64):
    """(a, |a| bound): the gathered operand behind the prologue, as the reference sees it."""
    x = o.x.to(dtype)
    if c.pro is None:
        return x, x.abs()
    act = R.ACT_LEAKY if c.pro.startswith("leaky") else R.ACT_NONE
    ns = c.g.cin if c.pro == "nc" else 0
    a = R.prologue(x, o.scale.to(dtype), o.shift.to(dtype), ns, act, o.slope)
    mag = R.prologue(x, o.scale.to(dtype), o.shift.to(dtype), ns, act, o.slope, absolute=True) * max(1.0, abs(o.slope))
    return a, mag


def reference(c: Case, o: Operands, round_ops=R.bf16_rne) -> Reference:
    """The fp64 weight gradient of a case's operands, its magnitude sums and its fp32 yardstick (beta = 0).  An MM16
    instance's matrix operands are rounded to bf16 behind the prologue; the bias gradient sums the unrounded dy."""
    g = c.g
    a, amag = activated(c, o)
    d = o.dy.double()
    db, db_mag = R.bias_grad(d), R.bias_grad(d.abs())
    if c.mm16:
        a, d = round_ops(a), round_ops(d)
        amag = torch.maximum(amag, a.abs())
    dw = R.conv_backward_weight(a, d, g.k, g.stride, g.pad, g.transposed)
    absref = R.conv_backward_weight(amag, d.abs(), g.k, g.stride, g.pad, g.transposed)
    dw32 = R.conv_backward_weight(a.float(), d.float(), g.k, g.stride, g.pad, g.transposed)
    return Reference(dw, absref, dw32, db, db_mag, c.M + 2 + (2 if c.pro else 0) + 1)


def with_beta(c: Case, o: Operands, ref: Reference, beta: float):
    """The expected dw / dbias (and magnitudes, fp32 yardstick) of a launch with this beta onto old_w / old_b."""
    if beta == 0.0:
        return ref
    ow, ob = beta * o.old_w.double(), beta * o.old_b.double()
    return Reference(ref.dw + ow, ref.absref + ow.abs(), ref.dw32 + ow.float(), ref.db + ob, ref.db_mag + ob.abs(), ref.L)


def check(c: Case, tier: str, got_dw, got_db, want: Reference):
    """The failures (strings) of one launch's outputs against the expected values; got_db None: no bias gradient."""
    fails = []
    got_dw = got_dw.reshape(want.dw.shape)
    if tier == "X":
        assert want.absref.max().item() < R.EXACT_LIMIT, f"{c.id}: tier X operands too dense ({want.absref.max().item()})"
        ok, msg = R.check_exact(got_dw, want.dw)
        if not ok:
            fails.append(f"{c.id} tier X dw: {msg}")
    else:
        ok, re_, rn = R.check_random(got_dw, want.dw, want.absref, want.dw32, want.L)
        if not ok:
            fails.append(f"{c.id} tier R dw: elementwise {re_:.3g} norm-wise {rn:.3g}")
    if got_db is not None:
        if tier == "X":
            assert R.exact_sums_ok(want.db_mag, 1), f"{c.id}: tier X dy too dense for an exact bias gradient"
            ok, _ = R.check_sums(got_db, want.db, want.db_mag, 0, exact=True)
        else:
            ok, ratio = R.check_sums(got_db, want.db, want.db_mag, c.M)
        if not ok:
            fails.append(f"{c.id} tier {tier} dbias: " + ("not exact" if tier == "X" else f"ratio {ratio:.3g}"))
    return fails
