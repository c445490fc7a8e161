"""Every convolution launch of the headline steps, replayed at its exact production geometry against the fp64
reference of tests/conv_ref.py.

The launch inventory is taken from the plans, not from a hand-written list: the test builds the networks, runs one
step, walks every `engine.Program` of the plans they built (`_plans` on the modules; `names`, `calls`, `keep`) and
decodes each call whose C entry is a convolution launch -- the full `mpgan_conv_geom` (flags, min_blocks), the row
pitches, which optional pointers are set, every pointer's offset mod 16 bytes, the prologue's n_stride / act /
device slope, the weight gradients' beta and workspace size.  Launches equal in all of that are replayed once.  A
conv entry the replayer does not know fails the test, and so does an empty inventory.
Configs: C5's train step (128^3, batch 4, bf16 storage in D, bf16 matrix operands in G), C5's generator in eval mode
at batch 1 (the sliding-window predictor), and C3 (256^2, batch 16, fp32).

Each launch runs on fresh buffers of the production shape, pitch and pointer offset mod 16 (input channels outside
the slice hold other values; outputs and partial-row buffers are pre-filled with NaN, so an unwritten element fails,
and a guard region behind each output must stay NaN; accumulating weight gradients start from known values and must
come out as beta*old + new).  Each distinct launch is one test, with a readable id that `-k` selects
(`c5-train-D-64to128-k3x3x3-s1-in126x126x126-backward_data_bf16`).  The rules:
  * tier X (exact): integer operands (x and dy sparse, weights dense, all in [-3, 3]; prologue scales +-4, shift 0,
    slope 0.25 -- an integer on both sides of the kink; epilogue scales +-4, shift 0, slope 0.25), with densities chosen
    so that the fp64 magnitude sum behind every output stays below 2^21 (checked) -- any fp32 summation order is
    exact, so y / dx / dw must equal the reference bit for bit (after one RNE to bf16 for a bf16 output).
  * tier Xs (sparse exact, launches with fused sums): the same with operands thinned (and bias 0) until the magnitude
    sums of the fused statistics / norm-backward sums stay below 2^24 per channel; those sums must then be exact too.
  * tier R (random): operands uniform in (-1, 1), weights / sqrt(K), rounded where the contract rounds (bf16 storage;
    bf16 matrix operands of G's MFMA convs, whose prologue stays +-2^k with slope 0.25 so the rounding is
    reproducible; elsewhere production's host slope); conv_ref.RandomCheck with
    L = K + 2 + 2 (prologue) + 1 (residual) + 3 (epilogue BatchNorm + PReLU) + 1 (beta).
  * fused reductions: exact wherever the magnitude sums allow it (tier Xs always; tier X where they happen to); else
    statistics rows and norm-backward sums are held to (L + 1) 2^-24 sum|terms| with L = conv_ref.row_chain (the rows
    are added in fp64 here, so the kernel's chain is one row's pixels) plus what the kernel's own y may differ by.  The
    bias gradient of a weight-gradient launch is exact in tier X; in tier R its slab structure is the library's own
    and it is held only to L = M (all pixels), a loose bound.  NaN pre-fill and guards catch unwritten and stray rows.
Every launch prints its dispatch label, both tiers' ratios, its wall time and its peak device memory."""
import ctypes as C
import gc
import math
import time

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

# C entry -> its arguments in order (the stream, appended by Program.run, excluded)
LAYOUT = {
    "mpgan_conv_forward": "g x ldx w bias pro resid ldr tanh stats y ldy",
    "mpgan_conv_forward_act": "g x ldx w escale eshift eslope resid ldr tanh y ldy",
    "mpgan_conv_forward_bf16": "g x ldx w bias stats y ldy",
    "mpgan_conv_forward_f32_to_bf16": "g x ldx w bias stats y ldy",
    "mpgan_conv_backward_data": "g dy lddy w resid ldr dx lddx",
    "mpgan_conv_backward_data_stats": "g dy lddy w dx lddx z ldz scale shift mean invstd act slope partials",
    "mpgan_conv_backward_data_bf16": "g dy lddy w dx lddx",
    "mpgan_conv_backward_data_stats_bf16": "g dy lddy w dx lddx z ldz scale shift mean invstd slope partials",
    "mpgan_conv_backward_data_bf16_to_f32": "g dy lddy w dx lddx",
    "mpgan_conv_backward_weight": "g x ldx pro dy lddy dw dbias beta ws ws_bytes",
    "mpgan_conv_backward_weight_bf16": "g x ldx dy lddy dw beta ws ws_bytes",
    "mpgan_conv_backward_weight_bf16dy": "g x ldx dy lddy dw dbias beta ws ws_bytes",
}
# conv launch entries this replayer does not handle (they must not appear in the steps checked here)
UNHANDLED = {"mpgan_conv_forward_fold", "mpgan_conv_forward_splitk"}
PTRS = {"x", "w", "bias", "resid", "stats", "y", "escale", "eshift", "eslope", "dy", "dx", "z", "scale", "shift", "mean",
        "invstd", "partials", "dw", "dbias", "ws"}
GUARD = 1024                 # elements behind every output view that must stay NaN


def _kind(entry):
    return "fwd" if "forward" in entry else ("wgrad" if "weight" in entry else "dgrad")


def _val(a):
    return a.value if isinstance(a, C.c_void_p) else a


def _decode(entry, args):
    names = LAYOUT[entry].split()
    assert len(args) == len(names), (entry, len(args))
    a = dict(zip(names, args))
    gs = a["g"]._obj
    geom = (gs.n, tuple(gs.in_dhw), tuple(gs.out_dhw), gs.cin, gs.cout, tuple(gs.k), tuple(gs.stride), tuple(gs.pad),
            gs.transposed, gs.flags, gs.min_blocks)
    rec = {"entry": entry, "kind": _kind(entry), "geom": geom, "ld": {}, "off": {}, "pro": None, "scal": {}}
    for k, v in a.items():
        if k == "g":
            continue
        if k in PTRS:
            v = _val(v)
            if v:
                rec["off"][k] = int(v) % 16
        elif k.startswith("ld"):
            rec["ld"][k] = int(v)
        elif k == "pro":
            if v is not None:
                p = v._obj
                rec["pro"] = (p.n_stride, p.act, bool(p.slope_ptr), float(p.slope))
                rec["off"]["pscale"], rec["off"]["pshift"] = int(p.scale) % 16, int(p.shift) % 16
                if p.slope_ptr:
                    rec["off"]["pslope"] = int(p.slope_ptr) % 16
        else:
            rec["scal"][k] = float(v) if isinstance(v, float) else int(v)
    rec["key"] = repr((entry, geom, sorted(rec["ld"].items()), sorted(rec["off"].items()), rec["pro"],
                       sorted(rec["scal"].items())))
    return rec


def _programs(obj, depth=0, seen=None):
    from mpgan_amd.engine import Program
    seen = set() if seen is None else seen
    if id(obj) in seen or depth > 3:
        return
    seen.add(id(obj))
    for v in list(vars(obj).values()):
        for el in (v if isinstance(v, (list, tuple)) else (v,)):
            if isinstance(el, Program):
                if id(el) not in seen:
                    seen.add(id(el))
                    yield el
            elif hasattr(el, "__dict__") and type(el).__module__.endswith(".engine"):
                yield from _programs(el, depth + 1, seen)


def _collect(mods):
    recs = {}
    for label, mod in mods:
        for pool in mod._plans.values():
            for plan in pool:
                for prog in _programs(plan):
                    for i, (fn, args) in enumerate(prog.calls):
                        name = getattr(fn, "__name__", "") if fn is not None else ""
                        if not name.startswith("mpgan_conv_"):
                            continue
                        assert name not in UNHANDLED and name in LAYOUT, f"conv launch {name} has no replayer"
                        r = _decode(name, args)
                        r["label"] = f"{label} {prog.descs[i]}".strip()
                        recs.setdefault(r["key"], r)
    return list(recs.values())


def _geom(r):
    from mpgan_amd import ops
    n, ind, outd, cin, cout, k, s, p, tr, flags, mb = r["geom"]
    assert flags in (0, 1), flags
    op = tuple(o - ((i - 1) * ss - 2 * pp + kk) for i, o, ss, pp, kk in zip(ind, outd, s, p, k)) if tr else (0, 0, 0)
    g = ops.ConvGeom(n, ind, cin, cout, k, s, p, bool(tr), op, bool(flags & 1), mb)
    assert g.out_dhw == outd, (g.out_dhw, outd)
    return g


def _dispatch(r, g):
    from mpgan_amd import engine
    from mpgan_amd._lib import lib
    gc_ = g.c()
    e = r["entry"]
    if e == "mpgan_conv_backward_weight_bf16":
        return f"wgrad_bf16 v{lib().mpgan_conv_wgrad_variant_bf16(C.byref(gc_))}"
    bwd = int(r["kind"] == "dgrad")
    if e in ("mpgan_conv_forward_bf16", "mpgan_conv_backward_data_bf16", "mpgan_conv_backward_data_stats_bf16"):
        return f"bf16 v{lib().mpgan_conv_variant_bf16(C.byref(gc_), bwd)}"
    code = 0
    if r["pro"] is not None:
        ns, act, sp, slope = r["pro"]
        code = 2 if ns else (3 if act == R.ACT_LEAKY and not sp and 0.0 <= slope <= 1.0 else 1)
    if r["kind"] == "wgrad":
        return engine.kernel_label(lib().mpgan_conv_wgrad_kernel_name, C.byref(gc_), code,
                                   int(e == "mpgan_conv_backward_weight_bf16dy"))
    return f"f32 v{lib().mpgan_conv_variant(C.byref(gc_), bwd, code)}"


_INV = {}


def _batch(n, S, dims, seed):
    gen = torch.Generator().manual_seed(seed)
    shp = (n, 1) + (S,) * dims
    return {"t1w": (torch.rand(*shp, generator=gen) * 2 - 1).cuda(), "t2w": (torch.rand(*shp, generator=gen) * 2 - 1).cuda()}


def _inventory(cfg):
    if cfg in _INV:
        return _INV[cfg]
    from mpgan_amd.gan import GAN
    torch.manual_seed(0)
    if cfg.startswith("c5"):
        m, b = GAN(1, 128, 128, 128, dimensions=3, storage_dtype="bf16"), _batch(4, 128, 3, 5)
    else:
        m, b = GAN(1, 256, 256, dimensions=2), _batch(16, 256, 2, 6)
    m.train()
    opts, _ = m.configure_optimizers()
    m.fit_batch(b, 0, opts)
    torch.cuda.synchronize()
    train = _collect([("G", m.generator), ("D", m.discriminator)])
    if cfg.startswith("c5"):
        _INV["c5-train"] = train
        m.generator.eval()
        with torch.no_grad():
            m.generator(b["t1w"][:1])                 # the sliding-window predictor: eval mode, batch 1
        torch.cuda.synchronize()
        keys = {r["key"] for r in train}
        _INV["c5-eval"] = [r for r in _collect([("G", m.generator)]) if r["key"] not in keys]
    else:
        _INV["c3"] = train
    del m, opts, b
    gc.collect()
    torch.cuda.empty_cache()
    for c in [c for c in _INV if c.startswith(cfg[:2])]:
        print(f"\n[inventory {c}] {len(_INV[c])} distinct conv launches")
        for r in _INV[c]:
            print(f"  {r['label']:<44} {r['entry'][11:]:<26} {_dispatch(r, _geom(r)):<14} geom {r['geom']} ld {r['ld']} "
                  f"off16 {r['off']} pro {r['pro']} {r['scal']}")
    return _INV[cfg]


# ------------------------------------------------------------------ buffers and operands
def _flat(numel, dtype, off, fill):
    es = torch.empty((), dtype=dtype).element_size()
    assert off % es == 0, (off, dtype)
    base = torch.full((off // es + numel + GUARD,), fill, dtype=dtype, device="cuda")
    return base, base[off // es:off // es + numel]


def _act(shape, ld, off, dtype, fill):
    n, d, h, w, c = shape
    assert ld >= c
    base, flat = _flat(n * d * h * w * ld, dtype, off, fill)
    return base, flat.as_strided(shape, (d * h * w * ld, h * w * ld, w * ld, ld, 1))


class _Ops:
    def __init__(self, tier, seed):
        self.exact = tier in ("X", "Xs")
        self.gen = torch.Generator(device="cuda").manual_seed(seed)

    def u(self, shape):
        return torch.rand(shape, generator=self.gen, device="cuda") * 2 - 1

    def ints(self, shape, density=1.0):
        v = torch.randint(-3, 4, shape, generator=self.gen, device="cuda").float()
        if density < 1.0:
            v = v * (torch.rand(shape, generator=self.gen, device="cuda") < density)
        return v

    def data(self, shape, density):
        return self.ints(shape, density) if self.exact else self.u(shape)

    def pow2(self, shape):
        k = torch.randint(-1, 2, shape, generator=self.gen, device="cuda").float()
        return torch.where(torch.rand(shape, generator=self.gen, device="cuda") < 0.5, -1.0, 1.0) * torch.exp2(k)

    def scale(self, shape, pow2):
        if self.exact:       # +-4: with slope 0.25 an integer on both sides of the kink
            return torch.where(torch.rand(shape, generator=self.gen, device="cuda") < 0.5, -4.0, 4.0)
        if pow2:
            return self.pow2(shape)
        return torch.where(torch.rand(shape, generator=self.gen, device="cuda") < 0.5, -1.0, 1.0) * (
            torch.rand(shape, generator=self.gen, device="cuda") + 0.5)

    def shift(self, shape, zero):
        return torch.zeros(shape, device="cuda") if zero or self.exact else self.u(shape) * 0.5


def _into(t, off, name, offs):
    """A copy of vector / weight t placed at production's offset mod 16."""
    _, v = _flat(t.numel(), t.dtype, offs.get(name, off), 0)
    v.copy_(t.reshape(-1))
    return v


def _served(g):
    """bf16 matrix operands apply (oracle/mm16_emul.py: the MFMA kernels; 1-channel layers run on the VALU in fp32)."""
    return g.mm_bf16 and g.cin >= 16 and g.cout >= 16


def _outside_ok(base, view):
    view.fill_(float("nan"))
    return bool(torch.isnan(base).all())


# ------------------------------------------------------------------ the replay
def _replay(r, tier, seed, thin=1):
    """Run one inventory entry in one tier; returns a list of failure strings (printing every ratio), or None when the
    sparse exact tier's operands turned out too dense for exact sums (the caller retries with `thin` doubled)."""
    from mpgan_amd import ops
    from mpgan_amd._lib import check, lib
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    e, kind, g = r["entry"], r["kind"], _geom(r)
    O = _Ops(tier, seed)
    offs, ld, sc = r["off"], r["ld"], r["scal"]
    n, cin, cout, k, s, p, tr = g.n, g.cin, g.cout, g.k, g.stride, g.pad, g.transposed
    T = g.taps
    f32, bf = torch.float32, torch.bfloat16
    in5, out5 = (n, *g.in_dhw, cin), (n, *g.out_dhw, cout)
    M_in, M_out = n * g.in_dhw[0] * g.in_dhw[1] * g.in_dhw[2], n * g.out_dhw[0] * g.out_dhw[1] * g.out_dhw[2]
    res, fails = [], []
    fill_in = 3.0 if O.exact else 0.75
    served = _served(g) and e in ("mpgan_conv_forward", "mpgan_conv_forward_act", "mpgan_conv_backward_data",
                                  "mpgan_conv_backward_weight")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def note(what, ok, txt):
        res.append(f"{what} {txt}")
        if not ok:
            fails.append(f"{r['label']} [{e[11:]}] tier {tier}: {what} {txt}")

    def guard(what, base, view):
        ok = _outside_ok(base, view)
        note(what, ok, "untouched" if ok else "WRITTEN")

    def sums_note(what, ok_ratio, exact):
        ok, ratio = ok_ratio
        note(what, ok, ("exact" if ok else "NOT exact") if exact else f"{ratio:.3g}")

    def make_pro():
        ns, act, sp, slope = r["pro"]
        vshape = (n, cin) if ns else (cin,)
        psc = _into(O.scale(vshape, served), 0, "pscale", offs)
        psh = _into(O.shift(vshape, served), 0, "pshift", offs)
        slope_t = _into(torch.full((1,), 0.25, device="cuda"), 0, "pslope", offs) if sp else None
        # tier R passes production's host slope (C3's discriminator: 0.2); the exact tiers and the bf16-operand
        # contract keep 0.25, a power of two
        host = slope if (tier == "R" and not sp and not served) else 0.25
        return ops.Prologue(psc, psh, cin if ns else 0, act, host, slope_t)

    # the weight (torch layout) and its packs
    wshape = (cin, cout, *k) if tr else (cout, cin, *k)
    if kind != "wgrad":
        Kred = (cin if kind == "fwd" else cout) * T
        w = O.ints(wshape) if O.exact else O.u(wshape) / math.sqrt(Kred)
        packed_bf16 = e in ("mpgan_conv_forward_bf16", "mpgan_conv_backward_data_bf16", "mpgan_conv_backward_data_stats_bf16")
        if packed_bf16:
            wp = ops.pack_weight_bf16(w, for_dgrad=kind == "dgrad")
        else:
            wp = ops.pack_weight(w, transposed=tr, for_dgrad=kind == "dgrad")
        wp = _into(wp, 0, "w", offs)
        w_ref = R.bf16_rne(w) if (packed_bf16 or served) else w

    if kind == "fwd":
        x_dt = bf if e == "mpgan_conv_forward_bf16" else f32
        y_dt = bf if e in ("mpgan_conv_forward_bf16", "mpgan_conv_forward_f32_to_bf16") else f32
        has_stats = "stats" in offs
        tanh = bool(sc.get("tanh", 0))
        assert not (has_stats and ("resid" in offs or tanh)), "statistics of a conv with residual / tanh epilogue"
        x_base, x = _act(in5, ld["ldx"], offs["x"], x_dt, fill_in)
        rho = min(0.5, 4.0 / (cin * T))
        if tier == "Xs":     # sparse enough that sum y^2 per channel stays below 2^24 (E[a^2 w^2] <= 16 (x16 behind a prologue))
            rho = min(rho, 2.0 ** 22 / (M_out * cin * T * 16.0 * (16.0 if r["pro"] is not None else 1.0))) / thin
        x.copy_(O.data(in5, rho))
        pro = make_pro() if r["pro"] is not None else None
        bias = None
        if "bias" in offs:   # (zero in the sparse exact tier: M*|bias| alone would pass 2^24)
            bias = _into(torch.zeros(cout, device="cuda") if tier == "Xs" else O.data((cout,), 1.0), 0, "bias", offs)
        resid = None
        if "resid" in offs:
            _, resid = _act(out5, ld["ldr"], offs["resid"], f32, fill_in)
            resid.copy_(O.data(out5, 0.5))
        epi = None
        if e == "mpgan_conv_forward_act":
            epi = (_into(O.scale((cout,), False), 0, "escale", offs), _into(O.shift((cout,), False), 0, "eshift", offs),
                   _into(torch.full((cout,), 0.25, device="cuda") if O.exact else
                         torch.rand(cout, generator=O.gen, device="cuda") * 0.5, 0, "eslope", offs))
        y_base, y = _act(out5, ld["ldy"], offs["y"], y_dt, float("nan"))
        rows = 0
        part = None
        if has_stats:
            if e == "mpgan_conv_forward":
                rows = ops.conv_stats_rows(g, 0 if pro is None else (2 if pro.n_stride else 1))
            elif e == "mpgan_conv_forward_bf16":
                rows = ops.conv_stats_rows_bf16(g)
            else:
                rows = (M_out + 255) // 256
            assert rows > 0
            part_base, part = _flat(rows * 2 * cout, f32, offs["stats"], float("nan"))
        if e == "mpgan_conv_forward":
            ops.conv_forward(g, x, wp, bias, y, pro=pro, resid=resid, tanh_out=tanh, stats_partials=part)
        elif e == "mpgan_conv_forward_act":
            ops.conv_forward_act(g, x, wp, *epi, y, resid=resid, tanh_out=tanh)
        elif e == "mpgan_conv_forward_bf16":
            ops.conv_forward_bf16(g, x, wp, bias, y, stats_partials=part)
        else:
            ops.conv_forward_f32_to_bf16(g, x, wp, bias, y, stats_partials=part)
        torch.cuda.synchronize()
        got = y.clone()
        guard("y outside its view", y_base, y)
        L = Kred + 2 + (2 if pro is not None else 0) + (1 if resid is not None else 0) + (3 if epi is not None else 0)
        acc = R.RandomCheck(L, y_dt == bf, tanh)
        st, st_mag, st_extra = 0, 0, 0
        exact_ok, exact_msg, amax = True, "exact", 0.0
        for i in range(n):
            xi = x[i:i + 1].double()
            if pro is not None:
                ps = (pro.scale[i] if pro.n_stride else pro.scale).double()
                ph = (pro.shift[i] if pro.n_stride else pro.shift).double()
                ai = R.prologue(xi, ps, ph, 0, pro.act, pro.slope)
                aab = R.prologue(xi, ps, ph, 0, pro.act, pro.slope, absolute=True)
            else:
                ai, aab = xi, xi.abs()
            if served:
                ai = R.bf16_rne(ai)
                aab = torch.maximum(aab, ai.abs())
            ref = R.conv_forward(ai, w_ref.double(), k, s, p, g.out_dhw, tr)
            absr = R.conv_forward(aab, w_ref.double().abs(), k, s, p, g.out_dhw, tr)
            with R.no_tf32():
                ref32 = R.conv_forward(ai.float(), w_ref.float(), k, s, p, g.out_dhw, tr)
            if epi is not None:
                ref = R.act_epilogue(ref, *(v.double() for v in epi))
                absr = R.act_epilogue(absr, *(v.double() for v in epi), absolute=True)
                ref32 = R.act_epilogue(ref32, *epi)
            if bias is not None:
                ref, absr, ref32 = ref + bias.double(), absr + bias.double().abs(), ref32 + bias
            if resid is not None:
                ri = resid[i:i + 1]
                ref, absr, ref32 = ref + ri.double(), absr + ri.double().abs(), ref32 + ri
            gi = got[i:i + 1]
            if O.exact:
                amax = max(amax, absr.max().item())
                ok, msg = R.check_exact(gi, ref, y_dt == bf, tanh)
                if not ok and exact_ok:
                    exact_ok, exact_msg = False, f"sample {i}: {msg}"
            else:
                acc.add(gi, ref, absr, ref32)
            if has_stats:      # (no residual / tanh / epilogue here: ref is the pre-rounding output the sums are of)
                sm, mg, ex = R.stats_terms(ref, absr, 0 if O.exact else L)
                st, st_mag, st_extra = st + sm, st_mag + mg, st_extra + ex
            del ref, absr, ref32
        if O.exact:
            assert amax < R.EXACT_LIMIT, f"tier X operands too dense: magnitude sum {amax}"
            note("y", exact_ok, exact_msg)
        else:
            ok, re_, rn = acc.result()
            note("y", ok, f"elementwise {re_:.3g} norm-wise {rn:.3g}")
        if has_stats:
            exact = O.exact and R.exact_sums_ok(st_mag)
            if tier == "Xs" and not exact:
                return None
            sums_note("stats", R.stats_check(part.view(rows, 2, cout).double().sum(0), st, st_mag, st_extra, M_out, rows,
                                             exact), exact)
            guard("stats guard", part_base, part)

    elif kind == "dgrad":
        dy_dt = bf if e in ("mpgan_conv_backward_data_bf16", "mpgan_conv_backward_data_stats_bf16",
                            "mpgan_conv_backward_data_bf16_to_f32") else f32
        dx_dt = bf if e in ("mpgan_conv_backward_data_bf16", "mpgan_conv_backward_data_stats_bf16") else f32
        _, dy = _act(out5, ld["lddy"], offs["dy"], dy_dt, fill_in)
        rho = min(0.5, 4.0 / (cout * T))
        if tier == "Xs":     # sparse enough that the norm-backward sums (2 fractional bits) stay below 2^24
            rho = min(rho, 2.0 ** 20 / (M_in * cout * T * 12.0)) / thin
        dy.copy_(O.data(out5, rho))
        dx_base, dx = _act(in5, ld["lddx"], offs["dx"], dx_dt, float("nan"))
        resid = None
        if "resid" in offs:
            _, resid = _act(in5, ld["ldr"], offs["resid"], f32, fill_in)
            resid.copy_(O.data(in5, 0.5))
        stats = "partials" in offs
        if stats:
            bf_stats = e.endswith("_bf16")
            _, z = _act(in5, ld["ldz"], offs["z"], bf if bf_stats else f32, fill_in)
            z.copy_(O.data(in5, 0.5))
            nv = [_into(v, 0, nm, offs) for v, nm in ((O.scale((cin,), False), "scale"), (O.shift((cin,), False), "shift"),
                                                     (O.shift((cin,), False), "mean"),
                                                     (torch.ones(cin, device="cuda") if O.exact else
                                                      torch.rand(cin, generator=O.gen, device="cuda") + 0.5, "invstd"))]
            slope = 0.25 if O.exact else float(sc["slope"])
            gc_ = g.c()
            rows = lib().mpgan_conv_bwd_stats_rows_bf16(C.byref(gc_)) if bf_stats else ops.conv_bwd_stats_rows(g)
            assert rows > 0
            part_base, part = _flat(rows * 3 * cin, f32, offs["partials"], float("nan"))
            if bf_stats:
                check(lib().mpgan_conv_backward_data_stats_bf16(C.byref(gc_), dy.data_ptr(), ld["lddy"], wp.data_ptr(),
                                                                dx.data_ptr(), ld["lddx"], z.data_ptr(), ld["ldz"],
                                                                *(v.data_ptr() for v in nv), slope, part.data_ptr(), stream),
                      "backward_data_stats_bf16")
            else:
                assert ops.conv_backward_data_stats(g, dy, wp, dx, z, *nv, int(sc["act"]), slope, part) == rows
        elif e == "mpgan_conv_backward_data":
            ops.conv_backward_data(g, dy, wp, dx, resid=resid)
        elif e == "mpgan_conv_backward_data_bf16":
            ops.conv_backward_data_bf16(g, dy, wp, dx)
        else:
            ops.conv_backward_data_bf16_to_f32(g, dy, wp, dx)
        torch.cuda.synchronize()
        got = dx.clone()
        guard("dx outside its view", dx_base, dx)
        L = Kred + 2 + (1 if resid is not None else 0)
        acc, amax = R.RandomCheck(L, dx_dt == bf), 0.0
        exact_ok, exact_msg = True, "exact"
        for i in range(n):
            di = dy[i:i + 1].double()
            if served:
                di = R.bf16_rne(di)
            ref = R.conv_backward_data(di, w_ref.double(), k, s, p, g.in_dhw, tr)
            absr = R.conv_backward_data(di.abs(), w_ref.double().abs(), k, s, p, g.in_dhw, tr)
            with R.no_tf32():
                ref32 = R.conv_backward_data(di.float(), w_ref.float(), k, s, p, g.in_dhw, tr)
            if resid is not None:
                ri = resid[i:i + 1]
                ref, absr, ref32 = ref + ri.double(), absr + ri.double().abs(), ref32 + ri
            gi = got[i:i + 1]
            if O.exact:
                amax = max(amax, absr.max().item())
                ok, msg = R.check_exact(gi, ref, dx_dt == bf)
                if not ok and exact_ok:
                    exact_ok, exact_msg = False, f"sample {i}: {msg}"
            else:
                acc.add(gi, ref, absr, ref32)
            del ref, absr, ref32
        if O.exact:
            assert amax < R.EXACT_LIMIT, f"tier X operands too dense: magnitude sum {amax}"
            note("dx", exact_ok, exact_msg)
        else:
            ok, re_, rn = acc.result()
            note("dx", ok, f"elementwise {re_:.3g} norm-wise {rn:.3g}")
        if stats:       # from the STORED gradient and z, as the small-shape tests define them
            want, mag = R.norm_bwd_sums(got.double(), z.double(), *(v.double() for v in nv[:4]), slope, third=not bf_stats)
            exact = O.exact and R.exact_sums_ok(mag, 2)
            if tier == "Xs" and not exact:
                return None
            # a row adds at most row_chain terms; each term costs up to three roundings (zhat, gy * zhat)
            sums_note("norm-backward sums", R.check_sums(part.view(rows, 3, cin).double().sum(0), want, mag,
                                                         R.row_chain(M_in, rows) + 4, exact=exact), exact)
            guard("partials guard", part_base, part)

    else:   # wgrad
        x_dt = bf if e == "mpgan_conv_backward_weight_bf16" else f32
        dy_dt = f32 if e == "mpgan_conv_backward_weight" else bf
        Mred = M_in if tr else M_out
        rho = min(0.5, math.sqrt(2.0 ** 16 / (3.0 * Mred)))
        _, x = _act(in5, ld["ldx"], offs["x"], x_dt, fill_in)
        x.copy_(O.data(in5, rho))
        _, dy = _act(out5, ld["lddy"], offs["dy"], dy_dt, fill_in)
        dy.copy_(O.data(out5, rho))
        pro = make_pro() if r["pro"] is not None else None
        beta = float(sc["beta"])
        assert beta != 0.0, "the replay pre-fills dw with known values: beta = 0 would need a NaN-safe kernel"
        dw_base, dwf = _flat(cout * cin * T, f32, offs["dw"], float("nan"))
        old = O.data(wshape, 1.0)
        dw = dwf.view(wshape)
        dw.copy_(old)
        dbias = None
        if "dbias" in offs:
            db_base, dbias = _flat(cout, f32, offs["dbias"], float("nan"))
            old_b = O.data((cout,), 1.0)
            dbias.copy_(old_b)
        ws_bytes = int(sc["ws_bytes"])
        _, ws = _flat(max(ws_bytes // 4, 1), f32, offs.get("ws", 0), 0.0)
        if e == "mpgan_conv_backward_weight":
            ops.conv_backward_weight(g, x, dy, dw, ws, pro=pro, beta=beta, dbias=dbias)
        elif e == "mpgan_conv_backward_weight_bf16":
            ops.conv_backward_weight_bf16(g, x, dy, dw, ws, beta=beta)
        else:
            ops.conv_backward_weight_bf16dy(g, x, dy, dw, ws, beta=beta, dbias=dbias)
        torch.cuda.synchronize()
        got = dw.clone()
        guard("dw outside its view", dw_base, dwf)
        ref = beta * old.double()
        absr = (beta * old.double()).abs()
        ref32 = beta * old
        db_ref, db_mag = 0.0, 0.0
        for i in range(n):
            xi, di = x[i:i + 1].double(), dy[i:i + 1].double()
            if pro is not None:
                ps = (pro.scale[i] if pro.n_stride else pro.scale).double()
                ph = (pro.shift[i] if pro.n_stride else pro.shift).double()
                ai = R.prologue(xi, ps, ph, 0, pro.act, pro.slope)
                aab = R.prologue(xi, ps, ph, 0, pro.act, pro.slope, absolute=True)
            else:
                ai, aab = xi, xi.abs()
            if dbias is not None:
                db_ref, db_mag = db_ref + R.bias_grad(di), db_mag + R.bias_grad(di.abs())
            if served:
                ai, di = R.bf16_rne(ai), R.bf16_rne(di)
                aab = torch.maximum(aab, ai.abs())
            ref = ref + R.conv_backward_weight(ai, di, k, s, p, tr)
            absr = absr + R.conv_backward_weight(aab, di.abs(), k, s, p, tr)
            with R.no_tf32():
                ref32 = ref32 + R.conv_backward_weight(ai.float(), di.float(), k, s, p, tr)
        if O.exact:
            assert absr.max().item() < R.EXACT_LIMIT, f"tier X operands too dense: magnitude sum {absr.max().item()}"
            ok, msg = R.check_exact(got, ref)
            note("dw", ok, msg)
        else:
            L = Mred + 2 + (2 if pro is not None else 0) + 1
            ok, re_, rn = R.check_random(got, ref, absr, ref32, L)
            note("dw", ok, f"elementwise {re_:.3g} norm-wise {rn:.3g}")
        if dbias is not None:
            got_b = dbias.clone()
            want_b, mag_b = beta * old_b.double() + db_ref, db_mag + abs(beta) * old_b.double().abs()
            if O.exact:      # integer dy: exact in any order (the only tier that pins the slab structure of dbias)
                assert R.exact_sums_ok(mag_b), f"tier X operands too dense for an exact bias gradient: {mag_b.max().item()}"
                sums_note("dbias", R.check_sums(got_b, want_b, mag_b, 0, exact=True), True)
            else:            # the slab count is the library's own: L = all M pixels, a loose any-order bound
                sums_note("dbias", R.check_sums(got_b, want_b, mag_b, Mred), False)
            guard("dbias outside its view", db_base, dbias)

    torch.cuda.synchronize()
    print(f"  [{tier}] {r['label']:<44} {e[11:]:<26} {_dispatch(r, g):<14} {'; '.join(res)}  "
          f"({time.time() - t0:.1f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB)", flush=True)
    return fails


CONFIGS = ("c5-train", "c5-eval", "c3")
KINDS = {"c5-train": ("fwd", "dgrad", "wgrad"), "c5-eval": ("fwd",), "c3": ("fwd", "dgrad", "wgrad")}


def _launch_id(cfg, r):
    desc = r["label"].replace("->", "to").replace(" ", "-")
    return f"{cfg}-{desc}-{r['entry'][11:]}"


def pytest_generate_tests(metafunc):
    """One test per distinct launch, with a readable id (`-k c5-train-D-64to128` selects D.conv2's launches).  The
    inventory needs the GPU, so it is built while the module is collected on one; elsewhere (or if building it fails)
    the single placeholder case reports why."""
    if "launch" not in metafunc.fixturenames:
        return
    cases, ids = [], []
    if torch.cuda.is_available():
        try:
            for cfg in CONFIGS:
                for r in _inventory(cfg):
                    cases.append((cfg, r))
        except Exception as ex:         # surfaces as a failing test rather than a collection error
            cases = [("inventory", repr(ex))]
    else:
        cases = [("inventory", "no GPU: the launch inventory is built from plans on an MI355X")]
    seen = {}
    for cfg, r in cases:
        i = _launch_id(cfg, r) if cfg != "inventory" else "inventory"
        seen[i] = seen.get(i, 0) + 1
        ids.append(i if seen[i] == 1 else f"{i}-{seen[i]}")
    metafunc.parametrize("launch", cases, ids=ids)


def test_inventories_are_complete():
    """Every config has launches of every kind it runs (an empty or partial inventory fails)."""
    for cfg in CONFIGS:
        kinds = {r["kind"] for r in _inventory(cfg)}
        assert set(KINDS[cfg]) <= kinds, (cfg, kinds)


def test_step_launch_against_fp64_reference(launch):
    cfg, r = launch
    assert cfg != "inventory", r
    t0 = time.time()
    seed = 1000 + int.from_bytes(r["key"].encode()[-8:], "little") % 100000
    fails = _replay(r, "X", seed)
    if "stats" in r["off"] or "partials" in r["off"]:       # fused sums: a sparse exact pass as well
        for attempt in range(6):
            f = _replay(r, "Xs", seed + 3, thin=2 ** attempt)
            if f is not None:
                fails += f
                break
        else:
            fails.append("tier Xs: operands never sparse enough for exact sums")
    fails += _replay(r, "R", seed + 1)
    print(f"[{_launch_id(cfg, r)}] {time.time() - t0:.1f} s")
    assert not fails, "\n".join(fails)
