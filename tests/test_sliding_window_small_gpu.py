"""Every form of the sliding-window kernels (csrc/window_ops.hip: 4 gather, 4 count, 4 blend, 2 finalize) on the
MI355X at the smallest geometries that reach it, bit for bit (torch.equal everywhere: the kernels move bytes, do one
rounded product and one rounded add per window and one IEEE division, so there is nothing to tolerate).

(a) named cases and (b) a seeded sweep through sliding_window_inference against the CPU restatement of MONAI
(sliding_window_ref.py); (c) the four C entries directly, with buffers the test owns (alignment fallbacks, start
tables the planner never makes, a non-zero accumulator), against per-kernel references written in plain CPU torch
from the definitions in include/mpgan_hip.h.  Each test reads the label of what it launches from
mpgan_sw_kernel_name; the last test asserts that all 14 instances ran."""
import ctypes as C
import random

import pytest
import torch
import torch.nn.functional as F

import sliding_window_ref as ref
from mpgan_amd import _lib
from mpgan_amd import inference as inf
from sw_helpers import Recorder, at_offset, noisy

pytestmark = pytest.mark.gpu

CVAL = -0.75
ALIGNED = 16             # stand-in for the buffers sliding_window_inference allocates itself (fresh, so aligned)
LAUNCHED = set()         # labels of every launch of this file
T, Fa = "true", "false"


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def _offset_output(fn, off):
    """`fn` with its output moved `off` elements into a larger allocation (still contiguous)."""
    return fn if off == 0 else (lambda x: at_offset(fn(x), off))


def _labels(plan, batch, mode, in_ptr, pred_ptrs):
    """Labels of the launches sliding_window_inference makes for this plan, from the launches' own choice; the
    pointers the test cannot see are fresh allocations."""
    g, keep = inf._geometry(plan, batch, torch.device("cuda", torch.cuda.current_device()))
    imp = None if mode == "constant" else ALIGNED
    out = {"gather": inf.sw_kernel_name("gather", g, in_ptr, ALIGNED),
           "count": inf.sw_kernel_name("count", g, imp, ALIGNED),
           "blend": {inf.sw_kernel_name("blend", g, p, imp, ALIGNED) for p in pred_ptrs},
           "finalize": inf.sw_kernel_name("finalize", g, ALIGNED, ALIGNED, ALIGNED)}
    LAUNCHED.update({out["gather"], out["count"], out["finalize"]} | out["blend"])
    return out


def _through_inference(shape, roi, sw, overlap, mode, cout, in_off=0, out_off=0, seed=0, note=""):
    x = at_offset(_rand(shape, 100 + seed), in_off)
    rec = Recorder(_offset_output(noisy(cout, seed), out_off))
    got = inf.sliding_window_inference(x, roi, sw, rec, overlap=overlap, mode=mode, cval=CVAL)
    torch.cuda.synchronize()
    want, batches = ref.sliding_window(x.cpu(), roi, sw, rec.replay(), overlap=overlap, mode=mode, cval=CVAL)
    assert len(batches) == len(rec.inputs), note
    for i, (a, b) in enumerate(zip(rec.inputs, batches)):
        assert a.shape == b.shape and torch.equal(a, b), f"window batch {i} differs from the padded slices {note}"
    assert got.shape == want.shape, note
    assert torch.equal(got.cpu(), want), f"max |diff| {(got.cpu() - want).abs().max().item():.3e} {note}"
    plan = inf.plan_windows(shape[2:], roi, overlap)
    return plan, _labels(plan, shape[0], mode, x.data_ptr(), rec.output_ptrs)


# ---- (a) named cases -------------------------------------------------------------------------------------------
# name: (input shape, roi, sw, overlap, cout, in_off, out_off,
#        what plan_windows must give: x starts, windows per image, pad_lo,
#        the forms it must reach: gather, count/blend in quads, finalize in quads)
CASES = {
    "x_starts_odd": ((1, 1, 20, 22, 26), (8, 8, 12), 3, 0.25, 1, 0, 0, (0, 9, 14), 36, (0, 0, 0), (T, T), Fa, Fa),
    "roi_x_10_cin2": ((1, 2, 13, 17, 23), (6, 7, 10), 4, 0.25, 1, 0, 0, (0, 7, 13), 27, (0, 0, 0), (Fa, T), Fa, Fa),
    "roi_x_10_unaligned": ((1, 2, 13, 17, 23), (6, 7, 10), 4, 0.25, 1, 1, 0, (0, 7, 13), 27, (0, 0, 0), (Fa, Fa), Fa,
                           Fa),
    "vec_unaligned_in": ((2, 1, 16, 16, 24), (8, 8, 16), 3, 0.5, 2, 1, 0, (0, 8), 18, (0, 0, 0), (T, Fa), T, T),
    "vec_unaligned_pred": ((2, 1, 16, 16, 24), (8, 8, 16), 3, 0.5, 2, 0, 1, (0, 8), 18, (0, 0, 0), (T, T), (T, Fa), T),
    "pad_x_odd": ((1, 1, 19, 21, 9), (8, 8, 16), 2, 0.25, 1, 0, 0, (0,), 12, (0, 0, 3), (T, T), T, Fa),
    "pad_x_4": ((1, 1, 19, 21, 8), (8, 8, 16), 2, 0.25, 1, 0, 0, (0,), 12, (0, 0, 4), (T, T), T, T),
    "pad_x_2": ((1, 1, 19, 21, 12), (8, 8, 16), 2, 0.25, 1, 0, 0, (0,), 12, (0, 0, 2), (T, T), T, Fa),
    "pad_all": ((2, 2, 5, 3, 7), (8, 8, 12), 3, 0.25, 3, 0, 0, (0,), 1, (1, 2, 2), (T, T), T, Fa),
    "span_images": ((4, 1, 8, 8, 12), (8, 8, 8), 7, 0.5, 1, 0, 0, (0, 4), 2, (0, 0, 0), (T, T), T, T),
    "dense_overlap": ((1, 1, 6, 7, 9), (4, 4, 4), 16, 0.9, 1, 0, 0, (0, 1, 2, 3, 4, 5), 72, (0, 0, 0), (T, T), Fa, Fa),
    "roi_fallback": ((1, 1, 10, 12, 20), (0, 8, None), 2, 0.25, 1, 0, 0, (0,), 2, (0, 0, 0), (T, T), T, T),
    "2d_odd": ((1, 3, 31, 45), (9, 14), 5, 0.25, 2, 0, 0, (0, 10, 20, 30, 31), 25, (0, 0), (Fa, T), Fa, Fa),
    "2d_quads": ((3, 1, 24, 40), (16, 16), 4, 0.5, 1, 0, 0, (0, 8, 16, 24), 8, (0, 0), (T, T), T, T),
    "one_call": ((1, 1, 20, 22, 26), (8, 8, 12), 1000, 0.25, 1, 0, 0, (0, 9, 14), 36, (0, 0, 0), (T, T), Fa, Fa),
}


@pytest.mark.parametrize("mode", ["constant", "gaussian"])
@pytest.mark.parametrize("name", list(CASES))
def test_named_case(name, mode):
    shape, roi, sw, overlap, cout, in_off, out_off, xs, nwin, pad_lo, gather, wq, fq = CASES[name]
    plan, lab = _through_inference(shape, roi, sw, overlap, mode, cout, in_off, out_off, seed=len(name), note=name)
    # the case still means what its name says
    assert plan.starts[-1] == xs and plan.num_windows == nwin and plan.pad_lo == pad_lo, plan
    ci = T if mode == "constant" else Fa
    cq, bq = wq if isinstance(wq, tuple) else (wq, wq)
    assert lab["gather"] == f"sw_gather_kernel<{gather[0]}, {gather[1]}>"
    assert lab["count"] == f"sw_count_kernel<{cq}, {ci}>"
    assert lab["blend"] == {f"sw_blend_kernel<{bq}, {ci}>"}
    assert lab["finalize"] == f"sw_finalize_kernel<{fq}>"


def test_named_cases_reach_what_they_claim():
    """Properties of the cases beyond the labels (host arithmetic on the plans)."""
    def plan(name):
        c = CASES[name]
        return c, inf.plan_windows(c[0][2:], c[1], c[3])
    c, p = plan("span_images")                       # a call of 7 windows over images of 2: three and a half images
    assert c[2] / p.num_windows == 3.5
    c, p = plan("pad_all")                           # one call spans both images
    assert p.num_windows == 1 and c[2] >= c[0][0]
    c, p = plan("dense_overlap")
    assert p.interval == (1, 1, 1)
    c, p = plan("roi_fallback")
    assert p.roi == (10, 8, 20)
    c, p = plan("one_call")
    assert c[2] >= p.num_windows


# ---- (b) seeded sweep ------------------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_N = 36, 64


def _draw_sweep():
    rng = random.Random(SWEEP_SEED)
    cases = []
    for _ in range(SWEEP_N):
        nsd = rng.choice((2, 3))
        size = tuple(rng.randint(1, 28) for _ in range(nsd))
        roi = tuple(rng.choice((None, 0, rng.randint(1, 16), 4 * rng.randint(1, 4))) for _ in range(nsd))
        cases.append(dict(shape=(rng.randint(1, 3), rng.randint(1, 3)) + size, roi=roi, cout=rng.randint(1, 3),
                          overlap=rng.choice((0, 0.1, 0.25, 0.5, 0.75, 0.9)), sw=rng.choice((1, 2, 3, 5, 8, 64)),
                          mode=rng.choice(("constant", "gaussian")), in_off=rng.randint(0, 3),
                          out_off=rng.randint(0, 3)))
    return cases


SWEEP = _draw_sweep()


@pytest.mark.parametrize("i", range(SWEEP_N))
def test_sweep(i):
    c = SWEEP[i]
    _through_inference(c["shape"], c["roi"], c["sw"], c["overlap"], c["mode"], c["cout"], c["in_off"], c["out_off"],
                       seed=i, note=f"sweep case {i}: {c}")


def test_sweep_takes_both_values_of_every_dispatch_predicate():
    """From the plans alone: a changed seed or range cannot quietly lose coverage."""
    seen = {}
    labels = set()
    most = 0
    dev = torch.device("cpu")                       # the label query never reads the start table's device copy
    for c in SWEEP:
        p = inf.plan_windows(c["shape"][2:], c["roi"], c["overlap"])
        total = c["shape"][0] * p.num_windows
        most = max(most, total)
        facts = {"roi_x % 4": p.roi[-1] % 4 == 0, "padded_x % 4": p.padded[-1] % 4 == 0,
                 "x starts % 4": all(s % 4 == 0 for s in p.starts[-1]), "W % 4": c["shape"][-1] % 4 == 0,
                 "pad_lo_x % 4": p.pad_lo[-1] % 4 == 0, "pad_lo_x > 0": p.pad_lo[-1] > 0,
                 "input aligned": c["in_off"] == 0, "pred aligned": c["out_off"] == 0,
                 "imp null": c["mode"] == "constant", "3-D": len(p.roi) == 3, "cin > 1": c["shape"][1] > 1,
                 "cout > 1": c["cout"] > 1, "a call spans more than two images": c["sw"] > 2 * p.num_windows
                 and c["shape"][0] > 2, "several calls": total > c["sw"]}
        for k, v in facts.items():
            seen.setdefault(k, set()).add(v)
        g, keep = inf._geometry(p, c["shape"][0], dev)
        imp = None if c["mode"] == "constant" else ALIGNED
        labels |= {inf.sw_kernel_name("gather", g, ALIGNED + 4 * c["in_off"], ALIGNED),
                   inf.sw_kernel_name("count", g, imp, ALIGNED),
                   inf.sw_kernel_name("blend", g, ALIGNED + 4 * c["out_off"], imp, ALIGNED),
                   inf.sw_kernel_name("finalize", g, ALIGNED, ALIGNED, ALIGNED)}
    assert all(v == {True, False} for v in seen.values()), {k: v for k, v in seen.items() if len(v) < 2}
    assert len(labels) == 14, sorted(labels)
    assert most <= 400, most                       # windows in the largest case: the sweep stays quick


# ---- (c) the four C entries directly ---------------------------------------------------------------------------
class Geom:
    """An mpgan_sw_geom with its start tables, on the host and on the device."""

    def __init__(self, batch, dhw, pad_lo, padded, roi, starts):
        self.batch, self.dhw, self.pad_lo, self.padded, self.roi = batch, dhw, pad_lo, padded, roi
        self.starts = starts
        flat = [s for ss in starts for s in ss]
        self.host = (C.c_int32 * len(flat))(*flat)
        self.dev = torch.tensor(flat, dtype=torch.int32).cuda()
        g = self.c = _lib.SwGeomC()
        g.batch = batch
        for d in range(3):
            g.dhw[d], g.pad_lo[d], g.padded[d], g.roi[d], g.num[d] = dhw[d], pad_lo[d], padded[d], roi[d], len(starts[d])
        g.starts_dev = self.dev.data_ptr()
        g.starts_host = C.cast(self.host, C.POINTER(C.c_int32))
        self.nwin = len(starts[0]) * len(starts[1]) * len(starts[2])

    def window(self, i):
        """(image, slices in padded coordinates) of global window i: image-major, z slowest."""
        b, w = divmod(i, self.nwin)
        ny, nx = len(self.starts[1]), len(self.starts[2])
        st = (self.starts[0][w // (nx * ny)], self.starts[1][(w // nx) % ny], self.starts[2][w % nx])
        return b, tuple(slice(s, s + r) for s, r in zip(st, self.roi))


def _name(launch, geom, *ptrs):
    name = inf.sw_kernel_name(launch, geom.c, *ptrs)
    LAUNCHED.add(name)
    return name


def _ptr(t):
    return None if t is None else t.data_ptr()


def gather_ref(x, g, first, n, cval):
    pad = []
    for d in (2, 1, 0):
        pad += [g.pad_lo[d], g.padded[d] - g.dhw[d] - g.pad_lo[d]]
    xp = F.pad(x, pad, value=cval)
    out = []
    for i in range(first, first + n):
        b, sl = g.window(i)
        out.append(xp[(b, slice(None)) + sl])
    return torch.stack(out)


def count_ref(g, imp):
    count = torch.zeros(g.padded)
    w = torch.ones(g.roi) if imp is None else imp
    for i in range(g.nwin):
        count[g.window(i)[1]] += w
    return count


def blend_ref(acc, g, pred, first, n, imp):
    w = torch.ones(g.roi) if imp is None else imp
    for k in range(n):
        b, sl = g.window(first + k)
        acc[(b, slice(None)) + sl] += w * pred[k]
    return acc


def finalize_ref(acc, count, g):
    crop = tuple(slice(p, p + s) for p, s in zip(g.pad_lo, g.dhw))
    return (acc / count)[(slice(None), slice(None)) + crop]


def _calls(total, size):
    return [(f, min(size, total - f)) for f in range(0, total, size)]


def _pipeline(g, cin, cout, use_imp, calls, off=(), seed=0, acc_init=None):
    """Gather, count, blend (the given calls) and finalize through the C entries, each against its reference.  `off`
    names the buffers that start one element into their allocation.  Returns (labels, device acc)."""
    L, lab = _lib.lib(), {}
    o = {k: int(k in off) for k in ("in", "count", "imp", "pred", "acc", "out")}
    x = _rand((g.batch, cin) + g.dhw, seed)
    imp = (torch.rand(g.roi, generator=torch.Generator().manual_seed(seed + 1)) + 0.25) if use_imp else None
    acc0 = torch.zeros((g.batch, cout) + g.padded) if acc_init is None else acc_init
    xd, impd = at_offset(x, o["in"]), None if imp is None else at_offset(imp, o["imp"])
    countd = at_offset(torch.full(g.padded, float("nan")), o["count"])
    accd = at_offset(acc0, o["acc"])
    outd = at_offset(torch.full((g.batch, cout) + g.dhw, float("nan")), o["out"])

    lab["count"] = _name("count", g, _ptr(impd), countd.data_ptr())
    inf.check(L.mpgan_sw_count(C.byref(g.c), _ptr(impd), countd.data_ptr(), None), "sw_count")
    count = count_ref(g, imp)
    assert torch.equal(countd.cpu(), count), "count"

    acc = acc0.clone()
    lab["blend"] = set()
    for j, (first, n) in enumerate(calls):
        win = torch.full((n, cin) + g.roi, float("nan"), device="cuda")
        lab["gather"] = _name("gather", g, xd.data_ptr(), win.data_ptr())
        inf.check(L.mpgan_sw_gather(C.byref(g.c), xd.data_ptr(), cin, first, n, CVAL, win.data_ptr(), None), "sw_gather")
        assert torch.equal(win.cpu(), gather_ref(x, g, first, n, CVAL)), f"gather of call {j}"
        pred = _rand((n, cout) + g.roi, 1000 * seed + j)
        predd = at_offset(pred, o["pred"])
        lab["blend"].add(_name("blend", g, predd.data_ptr(), _ptr(impd), accd.data_ptr()))
        inf.check(L.mpgan_sw_blend(C.byref(g.c), predd.data_ptr(), cout, first, n, _ptr(impd), accd.data_ptr(), None),
                  "sw_blend")
        blend_ref(acc, g, pred, first, n, imp)
        assert torch.equal(accd.cpu(), acc), f"accumulator after call {j}"

    lab["finalize"] = _name("finalize", g, accd.data_ptr(), countd.data_ptr(), outd.data_ptr())
    inf.check(L.mpgan_sw_finalize(C.byref(g.c), accd.data_ptr(), cout, countd.data_ptr(), outd.data_ptr(), None),
              "sw_finalize")
    torch.cuda.synchronize()
    assert torch.equal(outd.cpu(), finalize_ref(acc, count, g)), "finalize"
    return lab, accd


def _quad_geom():
    """Everything in quads, roi_z != roi_y != roi_x, two images: (5, 6, 16) under roi (3, 4, 8)."""
    return Geom(2, (5, 6, 16), (0, 0, 0), (5, 6, 16), (3, 4, 8), ((0, 2), (0, 2), (0, 4, 8)))


@pytest.mark.parametrize("off,use_imp", [(o, u) for o in (None, "in", "count", "imp", "pred", "acc", "out")
                                         for u in (False, True) if u or o != "imp"])
def test_alignment_fallbacks(off, use_imp):
    """Each buffer on its own one element off 16-byte alignment, where quads would otherwise run: the launches that
    read or write it fall back to the scalar form (label) and compute the same bits."""
    g = _quad_geom()
    lab, _ = _pipeline(g, 2, 2, use_imp, _calls(2 * g.nwin, 3), off=() if off is None else (off,), seed=3)
    ci = Fa if use_imp else T
    scalar = {None: (), "in": (), "count": ("count", "finalize"), "imp": ("count", "blend"), "pred": ("blend",),
              "acc": ("blend", "finalize"), "out": ("finalize",)}[off]
    q = {k: (Fa if k in scalar else T) for k in ("count", "blend", "finalize")}
    assert lab["gather"] == f"sw_gather_kernel<true, {Fa if off == 'in' else T}>"
    assert lab["count"] == f"sw_count_kernel<{q['count']}, {ci}>"
    assert lab["blend"] == {f"sw_blend_kernel<{q['blend']}, {ci}>"}
    assert lab["finalize"] == f"sw_finalize_kernel<{q['finalize']}>"


# start tables the planner never produces, valid under the library's checks; every image voxel stays covered
TABLES = {
    "unsorted": (2, (6, 7, 16), (0, 0, 0), (6, 7, 16), (3, 4, 8), ((3, 0), (3, 0, 2), (8, 0, 4))),
    "duplicates": (1, (6, 7, 16), (0, 0, 0), (6, 7, 16), (3, 4, 8), ((0, 3, 3), (0, 0, 3), (0, 8, 8, 4))),
    "x_0_2_3_11": (2, (4, 5, 17), (0, 0, 0), (4, 5, 17), (2, 5, 6), ((0, 2), (0,), (0, 2, 3, 11, 6))),
    "padded_high": (2, (4, 5, 8), (1, 0, 4), (9, 8, 20), (3, 4, 8), ((0, 3, 6), (0, 4, 1), (0, 8, 12, 4))),
    "padded_high_odd": (1, (4, 5, 7), (1, 2, 3), (8, 9, 14), (3, 4, 5), ((0, 3, 5), (0, 4, 5), (0, 5, 9, 2))),
}


@pytest.mark.parametrize("use_imp", [False, True])
@pytest.mark.parametrize("name", list(TABLES))
def test_unplanned_start_tables(name, use_imp):
    g = Geom(*TABLES[name])
    _pipeline(g, 2, 2, use_imp, _calls(g.batch * g.nwin, 5), seed=5)


@pytest.mark.parametrize("use_imp", [False, True])
@pytest.mark.parametrize("quads", [True, False])
def test_blend_onto_nonzero_accumulator(quads, use_imp):
    """A call of a few windows from the middle of the list onto a random accumulator: what no window of the call
    covers comes back bit-identical (the kernel writes only where it added)."""
    g = _quad_geom()
    init = _rand((2, 2) + g.padded, 77)
    first, n = 5, 4
    lab, accd = _pipeline(g, 1, 2, use_imp, [(first, n)], off=() if quads else ("acc",), seed=7, acc_init=init)
    assert lab["blend"] == {f"sw_blend_kernel<{T if quads else Fa}, {Fa if use_imp else T}>"}
    covered = torch.zeros((2, 2) + g.padded, dtype=torch.bool)
    for i in range(first, first + n):
        b, sl = g.window(i)
        covered[(b, slice(None)) + sl] = True
    assert covered.any() and not covered.all()
    got = accd.cpu()
    assert torch.equal(got[~covered], init[~covered])
    assert not torch.equal(got[covered], init[covered])


@pytest.mark.parametrize("use_imp", [False, True])
@pytest.mark.parametrize("name", ["quads", "x_0_2_3_11"])
def test_blend_split_differently(name, use_imp):
    """The same windows blended one per call, all in one call and three per call: identical bits."""
    g = _quad_geom() if name == "quads" else Geom(*TABLES[name])
    L = _lib.lib()
    total, cout = g.batch * g.nwin, 2
    pred = _rand((total, cout) + g.roi, 9)
    imp = (torch.rand(g.roi, generator=torch.Generator().manual_seed(10)) + 0.25) if use_imp else None
    impd = None if imp is None else imp.cuda()
    want = blend_ref(torch.zeros((g.batch, cout) + g.padded), g, pred, 0, total, imp)
    for size in (1, total, 3):
        accd = torch.zeros((g.batch, cout) + g.padded, device="cuda")
        for first, n in _calls(total, size):
            predd = pred[first:first + n].contiguous().cuda()
            _name("blend", g, predd.data_ptr(), _ptr(impd), accd.data_ptr())
            inf.check(L.mpgan_sw_blend(C.byref(g.c), predd.data_ptr(), cout, first, n, _ptr(impd), accd.data_ptr(),
                                       None), "sw_blend")
        assert torch.equal(accd.cpu(), want), f"{size} windows per call"


def test_all_14_instances_ran():
    """Runs last: the labels of everything this file launched."""
    want = ({f"sw_{k}_kernel<{a}, {b}>" for k in ("gather", "count", "blend") for a in (T, Fa) for b in (T, Fa)}
            | {"sw_finalize_kernel<true>", "sw_finalize_kernel<false>"})
    assert len(want) == 14
    assert LAUNCHED == want, (sorted(want - LAUNCHED), sorted(LAUNCHED - want))
