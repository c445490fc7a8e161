"""The decision table of the weight gradient (choose_wgrad, csrc/conv_wgrad.hip), read through
mpgan_conv_wgrad_kernel_name_at with fake pointers: no GPU, nothing is launched or dereferenced.  From one baseline
geometry per form one predicate flips at a time and the label must follow; then every case of tests/wgrad_cases.py (the
table tests/test_wgrad_forms_gpu.py launches) must name its instance.  Together the labels read here are the library's
whole set of weight-gradient kernel instances, but for the ones proven unreachable (wgrad_cases.UNREACHABLE)."""
import ctypes as C
import os

import pytest

import wgrad_cases as W
from mpgan_amd import _lib, ops

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")

SEEN = set()
UNSUPPORTED, INVALID = -2, -1
G, P = W.generic_label, W.pipe_label


def name(g, **kw):
    rc, label = W.label_at(g, **kw)
    assert rc == 0, (rc, label)
    SEEN.add(label)
    return label


def refusal(g, **kw):
    rc, msg = W.label_at(g, **kw)
    assert rc != 0, msg
    return rc, msg


def leaky(slope, ptr=False):
    p = W.fake_pro("leaky_ptr" if ptr else "leaky", 0)
    p.slope = slope
    return p


# ------------------------------------------------------------------------------------------------ the K-stepped forms
def ks(cin=12, cout=72, mm=False, **kw):
    """2 x 19 x 21, 3x3 stride 1 pad 1: Cd 72 -> BD 128, T Cg = 108 -> BG 128; vector operands: the pipelined form."""
    a = dict(n=2, spatial=(19, 21), k=3, s=1, p=1)
    a.update(kw)
    return W.geom(a["n"], a["spatial"], cin, cout, a["k"], a["s"], a["p"], mm=mm)


def test_scalar_operands_by_channels_pitch_and_base():
    assert name(ks()) == P(128, 128, 0, True, False)
    assert name(ks(cout=74)) == G(128, 128, True, False)                       # Cd % 4
    assert name(ks(cin=10)) == G(128, 128, False, True)                        # Cg % 4
    assert name(ks(cin=10, cout=74)) == G(128, 128, True, True)
    assert name(ks(), dy=(76, 0)) == P(128, 128, 0, True, False)               # pitch > channels, still % 4
    assert name(ks(), dy=(77, 0)) == G(128, 128, True, False)                  # ldd % 4
    assert name(ks(), x=(16, 0)) == P(128, 128, 0, True, False)
    assert name(ks(), x=(15, 0)) == G(128, 128, False, True)                   # ldg % 4
    assert name(ks(), dy=(76, 4), x=(16, 8)) == P(128, 128, 0, True, False)    # slices 16 / 32 bytes into a wider buffer
    for off in (1, 2, 3):                                                      # base 4, 8, 12 bytes off
        assert name(ks(), dy=(None, off)) == G(128, 128, True, False)
        assert name(ks(), x=(None, off)) == G(128, 128, False, True)
    assert name(ks(), dy=(76, 1), x=(16, 2)) == G(128, 128, True, True)


def test_prologue_kinds_and_alignment():
    assert name(ks(), pro="ch") == P(128, 128, 1, True, False)
    assert name(ks(), pro="ch", pro_off=(1, 0)) == G(128, 128, False, True)    # scale off by one float
    assert name(ks(), pro="ch", pro_off=(0, 1)) == G(128, 128, False, True)    # shift
    assert name(ks(), pro="ch", pro_off=(4, 8)) == P(128, 128, 1, True, False)
    assert name(ks(), pro="nc") == G(128, 128, False, False)                   # per (sample, channel): never pipelined
    assert name(ks(cin=10), pro="nc") == G(128, 128, False, True)              # n_stride % 4
    for kind in ("leaky", "leaky_hi", "leaky_ptr"):                            # PRO 3 is the pad-free tile's alone
        assert name(ks(), pro=kind) == P(128, 128, 1, True, False)


def nopad(cin=24, cout=132, mm=False, p=0):
    return W.geom(2, (21, 23), cin, cout, 3, 1, p, mm=mm)


def test_pad_free_tile_and_its_leaky_prologue():
    assert name(nopad()) == P(128, 128, 0, False, False)
    assert name(nopad(), pro="ch") == P(128, 128, 1, False, False)
    assert name(nopad(), pro="leaky") == P(128, 128, 3, False, False)          # host slope 0.25
    for slope in (0.0, 1.0):                                                   # [0, 1] is closed
        assert name(nopad(), pro=leaky(slope)) == P(128, 128, 3, False, False)
    for slope in (-0.25, 1.5):
        assert name(nopad(), pro=leaky(slope)) == P(128, 128, 1, False, False)
    assert name(nopad(), pro="leaky_hi") == P(128, 128, 1, False, False)
    assert name(nopad(), pro=leaky(0.25, ptr=True)) == P(128, 128, 1, False, False)   # slope_ptr given
    for pad in ((0, 0, 1), (0, 1, 0), 1):                                      # padding in any dimension: PAD
        assert name(nopad(p=pad)) == P(128, 128, 0, True, False)
        assert name(nopad(p=pad), pro="leaky") == P(128, 128, 1, True, False)
    assert name(nopad(cout=64)) == P(64, 128, 0, True, False)                  # pad-free, but not the 128 x 128 tile
    assert name(nopad(cin=4)) == P(128, 64, 0, True, False)


# (cout, (cin, k, pad)) that give each BD / BG with vector operands
DENSE = {32: 24, 64: 40, 128: 72}
GATH = {32: (4, W.K23, W.P23), 64: (4, 3, 1), 128: (12, 3, 1)}


@pytest.mark.parametrize("bd,bg", list(W.TILE))
def test_nine_tiles_and_the_wave_split_boundary(bd, bg):
    cin, k, p = GATH[bg]
    kw = W.TILE[bd, bg][3]
    g = ks(cin=cin, cout=DENSE[bd], k=k, p=p)
    want = P(bd, bg, 0, True, False) if kw == 1 else G(bd, bg, False, False)    # kw == 4 keeps a tile off the pipeline
    assert name(g) == want
    assert name(g, pro="ch") == (P(bd, bg, 1, True, False) if kw == 1 else G(bd, bg, False, False))
    gm = ks(cin=cin, cout=DENSE[bd], k=k, p=p, mm=True)
    assert name(gm) == (P(bd, bg, 0, True, True) if kw == 1 else G(bd, bg, False, False))
    assert name(gm, pro="leaky") == (P(bd, bg, 1, True, True) if kw == 1 else G(bd, bg, False, False))
    for sd, sg in ((True, False), (False, True), (True, True)):                 # scalar operands: the generic kernel,
        lay = dict(dy=(None, 1) if sd else (None, 0), x=(None, 1) if sg else (None, 0))
        assert name(g, **lay) == G(bd, bg, sd, sg)
        assert name(gm, **lay) == G(bd, bg, sd, sg)                             # ... whatever mm_bf16 asks for
    # the tile boundaries: 32 / 33 and 64 / 65 dense channels or gathered columns
    assert name(ks(cout=32)).startswith(("wgrad_pipe_kernel<32, 128", "wgrad_kernel<32, 128"))
    assert name(ks(cout=36)).startswith("wgrad_pipe_kernel<64, 128")
    assert name(ks(cout=64)).startswith("wgrad_pipe_kernel<64, 128")
    assert name(ks(cout=68)).startswith("wgrad_pipe_kernel<128, 128")


def test_mm_bf16():
    assert name(ks(mm=True)) == P(128, 128, 0, True, True)
    assert name(ks(mm=True), pro="ch") == P(128, 128, 1, True, True)
    assert name(ks(mm=True), pro="nc") == G(128, 128, False, False)            # per-sample vectors stay fp32
    assert name(nopad(mm=True)) == P(128, 128, 0, False, True)
    assert name(nopad(mm=True), pro="leaky") == P(128, 128, 1, False, True)    # no PRO 3 among the MM16 instances
    assert name(nopad(mm=True), pro="ch") == P(128, 128, 1, False, True)


def test_transposed():
    # ConvTranspose3d 24 -> 12, k3 s2 p1 op1: dense = x (Cd 24), gathered = dy (T Cg = 324)
    g = W.geom(2, (5, 7, 9), 24, 12, 3, 2, 1, tr=True, op=1)
    assert name(g) == P(32, 128, 0, True, False)
    assert name(g, x=(None, 1)) == G(32, 128, True, False)                     # x is the DENSE operand here
    assert name(g, dy=(None, 1)) == G(32, 128, False, True)
    assert name(W.geom(2, (5, 7, 9), 24, 12, 3, 2, 1, tr=True, op=1, mm=True)) == P(32, 128, 0, True, True)
    assert name(W.geom(2, (5, 7, 9), 22, 12, 3, 2, 1, tr=True, op=1)) == G(32, 128, True, False)     # cin % 4
    rc, msg = refusal(g, pro="ch")
    assert rc == UNSUPPORTED and "prologue on a transposed conv input" in msg
    g2 = W.geom(2, (17, 19), 24, 12, 3, 2, 1, tr=True, op=(0, 1, 1))           # 2-D
    assert name(g2) == P(32, 128, 0, True, False)


# ---------------------------------------------------------------------------------------------------- the thin forms
def thin(cin=1, cout=8, k=3, p=1, s=1, spatial=(37, 41)):
    return W.geom(2, spatial, cin, cout, k, s, p)


def test_thin_admission():
    T = "wgrad_thin_kernel<{}, {}, false>".format
    assert name(thin()) == T(4, 9)
    assert name(thin(cout=6)) == T(1, 9)                                       # Cd % 4: scalar lanes
    assert name(thin(), dy=(11, 0)) == T(1, 9)                                 # ldd % 4
    assert name(thin(), dy=(None, 1)) == T(1, 9)                               # base
    assert name(thin(), dy=(12, 4)) == T(4, 9)
    assert name(thin(), x=(None, 1)) == T(4, 9)                                # the gathered plane's alignment: no matter
    assert name(thin(k=1, p=0)) == T(4, 1)
    assert name(thin(k=1, p=0, cout=6)) == T(1, 1)
    assert name(thin(spatial=(9, 13, 15))) == T(4, 27)
    assert name(thin(spatial=(9, 13, 15)), dy=(None, 1)) == T(1, 27)
    assert name(thin(s=2)) == T(4, 9)                                          # any stride / padding
    assert name(thin(cin=2)) == G(32, 32, False, True)                         # Cg == 1 only
    assert name(thin(), pro="ch") == G(32, 32, False, True)                    # no prologue
    assert name(thin(cout=64)) == T(4, 9)
    assert name(thin(cout=68)) == G(128, 32, False, True)                      # Cd <= 64
    assert name(thin(k=(1, 2, 3), p=(0, 1, 1))) == G(32, 32, False, True)      # T in {1, 9, 27} ...
    assert name(thin(k=(1, 1, 9), p=(0, 0, 4))) == G(32, 32, False, True)      # ... as 1, 3x3 or 3x3x3
    assert name(thin(spatial=(9, 13, 15), k=(3, 3, 1), p=(1, 1, 0))) == G(32, 32, False, True)
    # fold rounds: 3x3x3 lane rows beyond 64 KiB are halved, which pays for at most 16 dense channels
    assert name(thin(spatial=(9, 13, 15), cout=16)) == T(4, 27)
    assert name(thin(spatial=(9, 13, 15), cout=32)) == G(32, 32, False, True)
    assert name(thin(spatial=(9, 13, 15), cout=64)) == G(64, 32, False, True)
    # transposed: the roles swap (dense = x, gathered = dy)
    assert name(W.geom(2, (17, 19), 8, 1, 3, 2, 1, tr=True, op=(0, 1, 1))) == T(4, 9)
    assert name(W.geom(2, (17, 19), 8, 1, 3, 2, 1, tr=True, op=(0, 1, 1)), x=(None, 1)) == T(1, 9)
    assert name(W.geom(2, (5, 7, 9), 32, 1, 3, 2, 1, tr=True, op=1)) == G(32, 32, False, True)


def rows(cout=64, k=3, p=0, s=1, spatial=(232, 7)):
    return W.geom(2, spatial, 1, cout, k, s, p)


def test_thin_rows_admission():
    R9, T9 = "wgrad_thin_rows_kernel<9, false>", "wgrad_thin_kernel<4, 9, false>"
    assert name(rows()) == R9
    assert name(rows(), dy=(67, 1)) == R9                                      # the row walker reads dy by elements
    assert name(rows(spatial=(232, 6))) == R9                                  # Mx == 4
    assert name(rows(spatial=(232, 5))) == T9                                  # Mx >= 4
    assert name(rows(), x=(2, 0)) == T9                                        # ldg == 1
    assert name(rows(p=1)) == T9
    assert name(rows(s=2)) == T9
    assert name(rows(cout=60)) == T9                                           # Cd == 64
    assert name(rows(k=1)) == "wgrad_thin_kernel<4, 1, false>"
    assert name(rows(), pro="ch") == G(64, 32, False, True)
    assert name(rows(), bf16_dy=True) == "wgrad_thin_rows_kernel<9, true>"
    assert name(rows(spatial=(11, 33, 6)), bf16_dy=True) == "wgrad_thin_rows_kernel<27, true>"
    assert name(rows(spatial=(11, 33, 5)), bf16_dy=True) == "wgrad_thin_kernel<4, 27, true>"
    assert name(rows(spatial=(11, 33, 6), p=1), bf16_dy=True) == "wgrad_thin_kernel<4, 27, true>"
    # fp32 dy, 3x3x3: the fold-round rule refuses every thin form, the row walker with it (W.UNREACHABLE)
    assert name(rows(spatial=(11, 33, 6))) == G(64, 32, False, True)


def test_two_plane_row_walker():
    for sp, t in (((231, 6), 9), ((11, 33, 7), 27)):
        for bf in (False, True):
            label = ops.conv2p_wgrad_kernel_name(W.geom(2, sp, 2, 64, 3, 1, 0), bf)
            assert label == f"wgrad_thin2_rows_kernel<{t}, {W.b(bf)}>"
            SEEN.add(label)
    with pytest.raises(RuntimeError, match="pad-free stride-1 ConvNd 2 -> 64"):
        ops.conv2p_wgrad_kernel_name(W.geom(2, (231, 5), 2, 64, 3, 1, 0), False)                # Mx < 4
    with pytest.raises(RuntimeError, match="pad-free stride-1 ConvNd 2 -> 64"):
        ops.conv2p_wgrad_kernel_name(W.geom(2, (231, 6), 2, 64, 3, 1, 1), False)


# --------------------------------------------------------------------------------------------------- the patch forms
def p3(spatial=(5, 17, 11), cin=16, cout=16, k=3, s=1, p=1, mm=False):
    return W.geom(2, spatial, cin, cout, k, s, p, mm=mm)


def test_patch3d_admission():
    L = "wgrad_patch3d_c16_kernel<{}, {}>".format
    assert name(p3()) == L("false", "false")
    assert name(p3(), pro="ch") == L("true", "false")
    assert name(p3(), pro="leaky_ptr") == L("true", "false")
    assert name(p3(mm=True)) == L("false", "true")
    assert name(p3(mm=True), pro="leaky") == L("true", "true")
    assert name(p3(p=0, spatial=(7, 19, 13))) == L("false", "false")           # pad in {0, 1}
    assert name(p3(p=(0, 1, 0))) == L("false", "false")
    assert name(p3(p=2)) == P(32, 128, 0, True, False)
    assert name(p3(spatial=(2, 4, 4))) == L("false", "false")                  # out_dhw >= (2, 4, 4)
    for sp in ((1, 17, 11), (5, 3, 11), (5, 17, 3)):
        assert name(p3(spatial=sp)) == P(32, 128, 0, True, False)
    assert name(p3(s=2)) == P(32, 128, 0, True, False)
    assert name(p3(cin=32)) == P(32, 128, 0, True, False)
    assert name(p3(cout=32)) == P(32, 128, 0, True, False)
    # 16-byte vectors on both operands and the prologue, one scale per channel
    assert name(p3(), x=(20, 4), dy=(24, 8)) == L("false", "false")
    assert name(p3(), x=(None, 1)) == G(32, 128, False, True)
    assert name(p3(), dy=(None, 2)) == G(32, 128, True, False)
    assert name(p3(), x=(18, 0)) == G(32, 128, False, True)
    assert name(p3(), dy=(17, 0)) == G(32, 128, True, False)
    assert name(p3(), pro="ch", pro_off=(1, 0)) == G(32, 128, False, True)
    assert name(p3(), pro="ch", pro_off=(0, 2)) == G(32, 128, False, True)
    assert name(p3(), pro="nc") == G(32, 128, False, False)
    assert name(p3(mm=True), dy=(None, 2)) == G(32, 128, True, False)


def p2(cin, cout, s=1, spatial=None, p=1, k=3):
    return W.geom(2, spatial or ((19, 21) if s == 1 else (37, 41)), cin, cout, k, s, p)


def test_patch2d_admission():
    L = "wgrad_patch2d_kernel<{}, {}, {}, {}, {}>".format
    for cd, cg, s, tx in ((16, 16, 1, 16), (32, 32, 1, 16), (32, 16, 2, 16), (64, 16, 2, 8)):
        assert name(p2(cg, cd, s)) == L(cd, cg, s, tx, "false")
        assert name(p2(cg, cd, s), pro="leaky") == L(cd, cg, s, tx, "true")
        assert name(p2(cg, cd, s), x=(cg + 4, 4), dy=(cd + 8, 8)) == L(cd, cg, s, tx, "false")
        assert name(p2(cg, cd, s), x=(None, 1)).startswith("wgrad_kernel<")    # vectors only
        assert name(p2(cg, cd, s), dy=(cd + 1, 0)).startswith("wgrad_kernel<")
        assert name(p2(cg, cd, s), pro="nc").startswith("wgrad_kernel<")
        assert name(p2(cg, cd, s), pro="ch", pro_off=(0, 1)).startswith("wgrad_kernel<")
        assert name(p2(cg, cd, s, p=0)).startswith("wgrad_pipe_kernel<")       # pad 1 only
        assert name(p2(cg, cd, 3 - s)).startswith("wgrad_pipe_kernel<")        # each channel pair has one stride
    assert name(p2(16, 16, spatial=(4, 4))) == L(16, 16, 1, 16, "false")       # My, Mx >= 4
    assert name(p2(16, 16, spatial=(3, 21))) == P(32, 128, 0, True, False)
    assert name(p2(16, 16, spatial=(19, 3))) == P(32, 128, 0, True, False)
    assert name(p2(16, 32, 2, spatial=(7, 8))) == L(32, 16, 2, 16, "false")    # stride 2: odd or even input
    assert name(p2(16, 32, 2, spatial=(5, 9))) == P(32, 128, 0, True, False)   # My 3
    assert name(p2(32, 64, 2)) == P(64, 128, 0, True, False)                   # 32 -> 64: left to the K-stepped kernel
    assert name(W.geom(2, (2, 19, 21), 16, 16, (1, 3, 3), 1, (0, 1, 1))) == P(32, 128, 0, True, False)   # depth 1 only
    # out = ceil(in / S) holds for every geometry whose extents agree (odd inputs under stride 2 too): only extents that
    # do not belong together leave the form
    g = p2(16, 32, 2)
    gc = g.c()
    gc.out_dhw[1] += 1
    assert name(g, gc=gc) == P(32, 128, 0, True, False)
    # transposed k3 s2 p1 with output padding 1 (out = 2 in): the same instances with the roles swapped
    assert name(W.geom(2, (9, 11), 64, 16, 3, 2, 1, tr=True, op=(0, 1, 1))) == L(64, 16, 2, 8, "false")
    assert name(W.geom(2, (9, 11), 32, 16, 3, 2, 1, tr=True, op=(0, 1, 1))) == L(32, 16, 2, 16, "false")
    assert name(W.geom(2, (9, 11), 64, 16, 3, 2, 1, tr=True, op=0)) == P(64, 128, 0, True, False)   # out = 2 in - 1
    assert name(W.geom(2, (9, 11), 64, 16, 3, 2, 1, tr=True, op=(0, 1, 1)), x=(None, 1)) == G(64, 128, True, False)


# ------------------------------------------------------------------------------------------------ the bf16-dy entry
def test_bf16_dy_entry_and_its_refusals():
    T = "wgrad_thin_kernel<4, {}, true>".format
    assert name(thin(cout=12), bf16_dy=True) == T(9)
    assert name(thin(cout=12, k=1, p=0), bf16_dy=True) == T(1)
    assert name(thin(cout=12, spatial=(9, 13, 15)), bf16_dy=True) == T(27)
    for cout in (32, 64):                                                      # 112 KiB of lane rows: this entry's cap
        assert name(thin(cout=cout, spatial=(5, 9, 11)), bf16_dy=True) == T(27)
    assert name(thin(cout=12), bf16_dy=True, dy=(16, 4)) == T(9)               # 8 bytes into a pitch-16 buffer
    assert name(thin(cout=12), bf16_dy=True, x=(None, 1)) == T(9)
    thin_only = "conv_backward_weight_bf16dy: thin path only"
    for g, kw in ((thin(cout=6), {}),                                          # Cout % 4
                  (thin(cout=68), {}),                                         # Cout <= 64
                  (thin(cout=12, k=4), {}),                                    # 1 / 3x3 / 3x3x3
                  (thin(cout=12, k=(1, 1, 9), p=(0, 0, 4)), {}),
                  (thin(cout=12), dict(dy=(14, 0))),                           # pitch % 4
                  (thin(cout=12), dict(dy=(None, 1))),                         # 2 bytes off
                  (thin(cout=12), dict(dy=(None, 2)))):                        # 4 bytes off: 8-byte vectors
        rc, msg = refusal(g, bf16_dy=True, **kw)
        assert rc == UNSUPPORTED and thin_only in msg, (g, kw, msg)
    one = "conv_backward_weight_bf16dy: ConvNd with one input channel only"
    rc, msg = refusal(thin(cin=2, cout=12), bf16_dy=True)
    assert rc == UNSUPPORTED and one in msg
    rc, msg = refusal(W.geom(2, (17, 19), 1, 8, 3, 2, 1, tr=True, op=(0, 1, 1)), bf16_dy=True)
    assert rc == UNSUPPORTED and one in msg


def test_query_validates_like_the_launch():
    L = _lib.lib()
    g = ks()
    gc = g.c()
    buf = C.create_string_buffer(160)
    A = W.A16
    ok = (C.byref(gc), A, 12, None, A, 72)
    assert L.mpgan_conv_wgrad_kernel_name_at(*ok, 0, buf, len(buf)) == 0
    assert L.mpgan_conv_wgrad_kernel_name_at(C.byref(gc), A, 11, None, A, 72, 0, buf, len(buf)) == INVALID
    assert b"conv_backward_weight: bad pitch" in L.mpgan_last_error()
    assert L.mpgan_conv_wgrad_kernel_name_at(C.byref(gc), A, 12, None, A, 71, 0, buf, len(buf)) == INVALID
    for args in ((None, A, 12, None, A, 72), (C.byref(gc), None, 12, None, A, 72), (C.byref(gc), A, 12, None, None, 72)):
        assert L.mpgan_conv_wgrad_kernel_name_at(*args, 0, buf, len(buf)) == INVALID
        assert b"conv_backward_weight: null pointer" in L.mpgan_last_error()
    assert L.mpgan_conv_wgrad_kernel_name_at(*ok, 0, buf, 8) == INVALID and b"needs" in L.mpgan_last_error()
    assert L.mpgan_conv_wgrad_kernel_name_at(*ok, 0, None, 160) == INVALID
    g1 = thin(cout=12)
    g1c = g1.c()
    assert L.mpgan_conv_wgrad_kernel_name_at(C.byref(g1c), None, 1, None, A, 12, 1, buf, len(buf)) == INVALID
    assert b"conv_backward_weight_bf16dy: null pointer" in L.mpgan_last_error()
    big = W.geom(1 << 12, (1 << 10, 1 << 10), 12, 72, 3, 1, 1)
    rc, msg = refusal(big)
    assert rc == INVALID and "more than 2^31 pixels" in msg
    # the query for compact aligned stand-ins is this one's special case
    for c in W.CASES:
        if c.entry == "f32" and c.pro in (None, "ch") and c.x == c.dy == (None, 0) and c.pro_off == (0, 0):
            gcc = c.g.c()
            buf2 = C.create_string_buffer(160)
            assert L.mpgan_conv_wgrad_kernel_name(C.byref(gcc), 1 if c.pro else 0, 0, buf2, len(buf2)) == 0
            assert buf2.value.decode() == c.label, c.id


# ------------------------------------------------------------------------------------------------ the launched table
@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.id)
def test_case_names_its_instance(c):
    label = W.case_label(c)
    SEEN.add(label)
    assert label == c.label
    if c.slabs is not None:
        assert W.case_slabs(c) == c.slabs
    # what the comments of the table promise about the reducer: narrow from 64 slabs of at most 16384 sums, fp32 dy
    g = c.g
    if "narrow" in c.why:
        assert c.slabs >= 64 and g.cin * g.cout * g.taps <= 16384 and not c.bf16_dy


def test_every_case_has_exact_operands_within_the_exact_limit():
    """Tier X may skip no case: the magnitude sums of the dyadic operands stay below conv_ref.EXACT_LIMIT (and the bias
    gradient's below 2^24).  Checked here because the reference is CPU fp64 either way."""
    import conv_ref as R
    for c in W.CASES:
        o = W.operands(c, "X")
        a, amag = W.activated(c, o)
        d = o.dy.double()
        g = c.g
        absref = R.conv_backward_weight(amag, d.abs(), g.k, g.stride, g.pad, g.transposed) + o.old_w.double().abs()
        assert absref.max().item() < R.EXACT_LIMIT, (c.id, absref.max().item())
        assert R.exact_sums_ok(R.bias_grad(d.abs()) + o.old_b.abs(), 1), c.id
        assert (a * 4 == (a * 4).round()).all() and (d == d.round()).all(), c.id          # dyadic: two fractional bits
        if c.mm16 or c.bf16_dy:
            assert (R.bf16_rne(a) == a).all() and (R.bf16_rne(d) == d).all(), c.id        # and exact in bf16


def test_design_table_is_generated_from_the_case_table():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert W.design_table() in open(os.path.join(root, "DESIGN.md")).read(), "run tools/wgrad_forms_table.py"


def test_the_table_reaches_every_reachable_instance():
    """Runs last in this file: the labels read above are the library's symbols, but for the proven-unreachable ones."""
    symbols = W.library_symbols()
    assert len(symbols) == 94, len(symbols)
    unreachable = set(W.UNREACHABLE)
    assert not (SEEN & unreachable), sorted(SEEN & unreachable)
    assert SEEN | unreachable == symbols, (sorted(symbols - SEEN - unreachable), sorted(SEEN - symbols))
    launched = {c.label for c in W.CASES}
    assert launched | unreachable == symbols, sorted(symbols - launched - unreachable)
