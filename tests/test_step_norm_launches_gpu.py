"""Every non-convolution launch of the headline steps, replayed at its exact production geometry against the fp64
reference of tests/norm_ref.py (the companion of tests/test_step_launches_gpu.py, which replays the convolutions).

Inventory: the same configs and plans as the conv replay (C5 train: 128^3, batch 4, bf16 storage in D; C5's generator in
eval mode at batch 1; C3: 256^2, batch 16).  Every call of every `engine.Program` whose C entry is not a convolution is
decoded through LAYOUT -- the geometry scalars (n, P, c, chunks, cstride, pitches, instance, eps, momentum, beta, slope,
g_f32, out_f32), which pointers are set and each one's offset mod 16, in-place aliasing, and the prologue fields -- and
launches equal in all of that are replayed once.  An entry without a replayer fails, and so does a non-null `peer`.
Python callables (`pack_if_stale`) are skipped by name.  The ops gan.py calls outside the plans (L1, BCE, Adam) are
recorded by wrapping `mpgan_amd.ops` during the inventory step.

Buffers: production shape, pitch and offset mod 16; channels outside a pitched slice hold other values; outputs and
partial-row buffers are pre-filled with NaN and a NaN guard sits behind each (behind the compact fold's scratch for a
finalize); accumulating outputs start from known values.  Finalize launches read synthetic partial rows of the
production row count and cstride: fp32 tile sums of an offset random (tier R) or sparse integer (tier X) tensor.
  * tier X: dyadic operands whose magnitude sums stay below 2^24 per channel: rows, sums and elementwise outputs must
    be bit-exact (after RNE for bf16 outputs); finalize outputs within 1 ulp (invstd) / 2 ulp (scale, shift, running
    statistics) of the fp64 formula on the kernel's own mean / invstd (norm_ref.finalize_check).
  * tier R: offset operands (|mean| / std = 10), production slope; sums within (L + 1) 2^-24 sum|terms| with L from
    norm_ref.chain_length; the variance's bound scales with E[z^2] and is propagated to invstd / scale / shift; elementwise
    outputs within a few ulp of their magnitude, plus 2^-8 relative for bf16 outputs.
Each launch prints its label, form, the worst error / bound ratio per output, its time and its peak memory."""
import ctypes as C
import gc
import math
import struct
import time

import pytest
import torch

import norm_ref as N
from test_step_launches_gpu import _programs

pytestmark = pytest.mark.gpu

LAYOUT = {
    "mpgan_channel_stats": "z ldz n P c partials",
    "mpgan_reduce_partials": "partials rows row_stride c out beta",
    "mpgan_norm_finalize": "partials n chunks c P instance gamma beta eps momentum rm rv nbt scale shift mean invstd",
    "mpgan_norm_finalize_strided": "partials n chunks c cstride P instance gamma beta eps momentum rm rv nbt scale shift "
                                   "mean invstd",
    "mpgan_norm_act_add": "z ldz pz r ldr pr n P c tanh out ldo",
    "mpgan_norm_bwd_reduce": "g ldg z ldz pro mean invstd peer n P c partials",
    "mpgan_norm_bwd_finalize": "partials n chunks c P instance dgamma dbeta dslope c1 c2",
    "mpgan_norm_bwd_apply": "g ldg z ldz pro mean invstd c1 c2 peer n P c dz lddz",
    "mpgan_norm_act_bf16": "z ldz scale shift slope rows c out ldo out_f32",
    "mpgan_norm_bwd_reduce_bf16": "g g_f32 ldg z ldz scale shift mean invstd slope rows c partials",
    "mpgan_norm_bwd_apply_bf16": "g g_f32 ldg z ldz scale shift mean invstd c1 c2 slope rows c dz lddz bias_partials",
    "mpgan_linear1_forward": "z pro n P c w bias partials logit prob",
    "mpgan_linear1_backward": "z pro n P c w dlogit g_a dw dbias beta",
    "mpgan_sigmoid_backward": "dprob prob n dlogit",
    "mpgan_tanh_backward": "g y numel dx",
    "mpgan_pack_weights_bf16": "src dst table n_entries max_elems",
    "mpgan_epi_vectors_multi": "table n_layers",
}
PRO = {"pro", "pz", "pr"}
SKIP = {"pack_if_stale"}                 # Python callables of a Program (the fp32 repack, skipped while weights are unchanged)
OUT_OF_PLAN = ("l1_loss", "bce_forward", "bce_backward", "adam_step")
GUARD = 1024
U = N.U
f32, bf = torch.float32, torch.bfloat16


def _val(a):
    return a.value if isinstance(a, C.c_void_p) else a


def _decode(entry, args, keep):
    names = LAYOUT[entry].split()
    assert len(args) == len(names), (entry, len(args), names)
    a = dict(zip(names, args))
    rec = {"entry": entry, "scal": {}, "off": {}, "pro": {}, "alias": [], "table": None}
    ptrs = {}
    for k, v in a.items():
        if k in PRO:
            if v is not None:
                p = v._obj
                rec["pro"][k] = (p.n_stride, p.act, round(float(p.slope), 6), bool(p.slope_ptr))
                rec["off"][k + ".scale"] = int(p.scale) % 16
            continue
        if k == "peer":
            assert v is None, f"{entry}: peer taps (variant B only) have no replayer here"
            continue
        if k == "table":
            t = [x for x in keep if isinstance(x, torch.Tensor) and x.dtype == torch.int64 and x.data_ptr() == int(v)]
            assert t, f"{entry}: table tensor not kept by the program"
            rec["table"] = t[0].cpu()
            continue
        if k in ("n", "P", "c", "chunks", "cstride", "instance", "rows", "row_stride", "numel", "tanh", "g_f32",
                 "out_f32", "n_entries", "max_elems", "n_layers") or k.startswith("ld"):
            rec["scal"][k] = int(v)
        elif k in ("eps", "momentum", "beta", "slope") and not isinstance(_val(v), (type(None),)) and \
                not (k == "beta" and entry.startswith("mpgan_norm_finalize")):
            rec["scal"][k] = round(float(v), 7)
        else:                            # a pointer
            v = _val(v)
            if v:
                rec["off"][k] = int(v) % 16
                ptrs[k] = int(v)
    inv = {}
    for k, v in ptrs.items():
        inv.setdefault(v, []).append(k)
    rec["alias"] = sorted(tuple(sorted(v)) for v in inv.values() if len(v) > 1)
    tkey = None
    if rec["table"] is not None:
        t = rec["table"]
        if entry == "mpgan_pack_weights_bf16":
            tkey = tuple(tuple(int(x) for x in r[2:7]) for r in t)
        else:
            tkey = tuple((tuple(bool(x) for x in r[:6]), int(r[9]), int(r[10]), int(r[11])) for r in t)
    rec["key"] = repr((entry, sorted(rec["scal"].items()), sorted(rec["off"].items()), sorted(rec["pro"].items()),
                       rec["alias"], tkey))
    return rec


def _collect(mods, recs):
    for label, mod in mods:
        for pool in mod._plans.values():
            for plan in pool:
                for prog in _programs(plan):
                    for i, (fn, args) in enumerate(prog.calls):
                        if fn is None:
                            continue
                        name = getattr(fn, "__name__", "")
                        if name in SKIP or name.startswith("mpgan_conv_"):
                            continue
                        assert name in LAYOUT, f"launch {name} has no replayer"
                        r = _decode(name, args, prog.keep[i] or ())
                        r["label"] = f"{label} {prog.descs[i]}".strip()
                        r["count"] = 1
                        if r["key"] in recs:
                            recs[r["key"]]["count"] += 1
                        else:
                            recs[r["key"]] = r
    return recs


_INV, _COUNTS = {}, {}


def _batch(n, S, dims, seed):
    gen = torch.Generator().manual_seed(seed)
    shp = (n, 1) + (S,) * dims
    return {"t1w": (torch.rand(*shp, generator=gen) * 2 - 1).cuda(), "t2w": (torch.rand(*shp, generator=gen) * 2 - 1).cuda()}


def _record_out_of_plan(recs):
    """Wrap the mpgan_amd.ops functions gan.py calls outside the plans; returns the restore callable."""
    from mpgan_amd import ops
    saved = {k: getattr(ops, k) for k in OUT_OF_PLAN}

    def wrap(name):
        def f(*a, **kw):
            if name == "l1_loss":
                scal = {"numel": a[0].numel(), "grad": (a[4] if len(a) > 4 else kw.get("grad_a")) is not None,
                        "grad_scale": float(a[5] if len(a) > 5 else kw.get("grad_scale", 1.0))}
            elif name == "adam_step":
                scal = {"numel": a[0].numel(), "lr": float(a[4]), "b1": float(a[5]), "b2": float(a[6]),
                        "eps": float(a[7]), "grad_scale": float(a[9] if len(a) > 9 else kw.get("grad_scale", 1.0))}
            else:
                scal = {"n": a[0].numel()}
            r = {"entry": name, "scal": scal, "off": {}, "pro": {}, "alias": [], "label": "out-of-plan", "count": 1,
                 "key": repr((name, sorted(scal.items())))}
            recs.setdefault(r["key"], r)
            return saved[name](*a, **kw)
        return f

    for k in OUT_OF_PLAN:
        setattr(ops, k, wrap(k))
    return lambda: [setattr(ops, k, v) for k, v in saved.items()]


def _entry_counts(mods):
    cnt = {}
    for _, mod in mods:
        for pool in mod._plans.values():
            for plan in pool:
                for prog in _programs(plan):
                    for fn, _ in prog.calls:
                        name = getattr(fn, "__name__", "") if fn is not None else ""
                        if name and name not in SKIP and not name.startswith("mpgan_conv_"):
                            cnt[name[6:]] = cnt.get(name[6:], 0) + 1
    return cnt


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
    oop = {}
    restore = _record_out_of_plan(oop)
    try:
        m.fit_batch(b, 0, opts)
    finally:
        restore()
    torch.cuda.synchronize()
    mods = [("G", m.generator), ("D", m.discriminator)]
    train = list(_collect(mods, {}).values()) + list(oop.values())
    counts = _entry_counts(mods)
    if cfg.startswith("c5"):
        _INV["c5-train"], _COUNTS["c5-train"] = train, counts
        g_train = _entry_counts([("G", m.generator)])
        m.generator.eval()
        with torch.no_grad():
            m.generator(b["t1w"][:1])
        torch.cuda.synchronize()
        keys = {r["key"] for r in train}
        allc = _entry_counts([("G", m.generator)])
        _COUNTS["c5-eval"] = {k: v - g_train.get(k, 0) for k, v in allc.items() if v != g_train.get(k, 0)}
        _INV["c5-eval"] = [r for r in _collect([("G", m.generator)], {}).values() if r["key"] not in keys]
    else:
        _INV["c3"], _COUNTS["c3"] = train, counts
    del m, opts, b
    gc.collect()
    torch.cuda.empty_cache()
    for c in [c for c in _INV if c.startswith(cfg[:2])]:
        print(f"\n[inventory {c}] {len(_INV[c])} distinct non-conv launches; calls per entry {_COUNTS[c]}")
        for r in _INV[c]:
            print(f"  {r['label']:<30} {r['entry']:<28} {r['scal']} off16 {r['off']} pro {r['pro']} alias {r['alias']}")
    return _INV[cfg]


# ------------------------------------------------------------------ buffers
def _flat(numel, dtype, off, fill):
    es = torch.empty((), dtype=dtype).element_size()
    assert off % es == 0, (off, dtype)
    base = torch.full((off // es + numel + GUARD,), fill, dtype=dtype, device="cuda")
    return base, base[off // es:off // es + numel]


def _rows(nrows, c, ld, off, dtype, fill):
    """A pitched [nrows][c] view (pitch ld) at byte offset `off`; the base is filled with `fill` everywhere."""
    base, flat = _flat(nrows * ld, dtype, off, fill)
    return base, flat.as_strided((nrows, c), (ld, 1))


def _untouched(base, view):
    view.fill_(float("nan"))
    return bool(torch.isnan(base.float()).all())


class _Ops:
    def __init__(self, tier, seed):
        self.exact = tier == "X"
        self.gen = torch.Generator(device="cuda").manual_seed(seed)

    def u(self, *shape):
        return torch.rand(shape, generator=self.gen, device="cuda") * 2 - 1

    def ints(self, shape, lo=-3, hi=3, density=1.0):
        v = torch.randint(lo, hi + 1, shape, generator=self.gen, device="cuda").float()
        if density < 1.0:
            v = v * (torch.rand(shape, generator=self.gen, device="cuda") < density)
        return v

    def sign(self, shape):
        return torch.where(torch.rand(shape, generator=self.gen, device="cuda") < 0.5, -1.0, 1.0)

    def offset(self, shape, ratio=10.0):
        """Offset random values: per-channel |mean| / std = ratio (channels last)."""
        c = shape[-1]
        std = torch.rand(c, generator=self.gen, device="cuda") + 0.5
        return (ratio * std * self.sign((c,)) + std * torch.randn(shape, generator=self.gen, device="cuda")).float()

    def data(self, shape, density=1.0):
        return self.ints(shape, density=density) if self.exact else self.offset(shape)

    def scale(self, shape):
        return self.sign(shape) * (torch.exp2(self.ints(shape, -1, 1)) if self.exact else
                                   torch.rand(shape, generator=self.gen, device="cuda") + 0.5)

    def shift(self, shape):
        return self.ints(shape, -2, 2) * 0.25 if self.exact else self.u(*shape) * 0.5

    def invstd(self, shape):
        return torch.exp2(self.ints(shape, -1, 1)) if self.exact else torch.rand(shape, generator=self.gen,
                                                                                  device="cuda") + 0.5


def _vec(t, off=0):
    """A copy of vector t at byte offset `off` mod 16."""
    _, v = _flat(t.numel(), t.dtype, off, 0)
    v.copy_(t.reshape(-1))
    return v


class _Run:
    def __init__(self, r, tier):
        self.r, self.tier, self.res, self.fails, self.form = r, tier, [], [], ""

    def note(self, what, ok, txt):
        self.res.append(f"{what} {txt}")
        if not ok:
            self.fails.append(f"{self.r['label']} [{self.r['entry']}] tier {self.tier}: {what} {txt}")

    def ratio(self, what, ok_r):
        ok, r = ok_r
        self.note(what, ok, "exact" if (ok and r == 0) else ("NOT exact" if (not ok and math.isinf(r)) else f"{r:.3g}"))

    def exact(self, what, got, want):
        g = got.double()
        ok = bool((g == want).all())
        if ok:
            self.note(what, True, "exact")
        else:
            bad = (g != want).reshape(-1)
            i = int(bad.nonzero()[0].item())
            self.note(what, False, f"{int(bad.sum())}/{bad.numel()} differ; first at {i}: got {g.reshape(-1)[i].item()!r} "
                                   f"want {want.reshape(-1)[i].item()!r}")

    def guard(self, what, base, view):
        ok = _untouched(base, view)
        self.note(what, ok, "untouched" if ok else "WRITTEN")


def _pro_vectors(O, p, n, c, offs, name):
    """A mpgan_prologue like production's: per-channel or per-(sample, channel) scale / shift, act, slope (host or
    device).  Returns (PrologueC, scale (n or 1, 1, c), shift, slope value, keepalive)."""
    from mpgan_amd._lib import PrologueC
    ns, act, slope, sp = p
    rows = n if ns else 1
    sc = O.scale((rows, c))
    sh = O.shift((rows, c))
    s = 0.25 if O.exact else (0.2 if sp else slope)
    vs, vh = _vec(sc, offs.get(name + ".scale", 0)), _vec(sh, offs.get(name + ".scale", 0))
    st = _vec(torch.full((1,), s, device="cuda")) if sp else None
    pc = PrologueC()
    pc.scale, pc.shift, pc.n_stride, pc.act, pc.slope = vs.data_ptr(), vh.data_ptr(), ns, act, s
    pc.slope_ptr = st.data_ptr() if sp else None
    s32 = float(torch.tensor(s, dtype=f32))
    return pc, sc.double().reshape(rows, 1, c), sh.double().reshape(rows, 1, c), s32, (vs, vh, st, pc)


def _synthetic_rows(O, n, P, c, chunks, W, exact):
    """Partial rows [n*chunks][2][W] of a tensor (n, P, c): fp32 chunk sums (self-consistent); columns c..W hold the
    rows of another tensor.  Returns (rows fp32 on the device, fp64 sums (2, c), magnitude sums, per-sample pairs)."""
    nq = 2
    rows = torch.empty(n * chunks, nq, W, device="cuda")
    s = torch.zeros(nq, c, dtype=torch.float64, device="cuda")
    mag = torch.zeros(nq, c, dtype=torch.float64, device="cuda")
    per_n = []
    for i in range(n):
        if exact:
            z = O.ints((1, P, c), density=min(1.0, 2.0 ** 22 / (9.0 * n * P)))
        else:
            z = O.offset((1, P, c))
        t = torch.cat([z, z * z], -1)
        rows[i * chunks:(i + 1) * chunks, :, :c] = N.chunk_rows(t, chunks).reshape(chunks, nq, c)
        t64 = t.double()
        si = t64.reshape(P, nq, c).sum(0)
        mi = t64.abs().reshape(P, nq, c).sum(0)
        s += si
        mag += mi
        per_n.append((si, mi))
        if W > c:
            o = O.offset((1, P, W - c), ratio=30.0)
            rows[i * chunks:(i + 1) * chunks, :, c:] = N.chunk_rows(torch.cat([o] * nq, -1), chunks).reshape(chunks, nq, W - c)
    return rows, s, mag, per_n


# ------------------------------------------------------------------ replayers
def _replay(r, tier, seed):
    from mpgan_amd._lib import lib
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    e, sc, offs = r["entry"], r["scal"], r["off"]
    O = _Ops(tier, seed)
    X = O.exact
    run = _Run(r, tier)
    L_ = lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E = e[6:] if e.startswith("mpgan_") else e

    if E == "channel_stats":
        n, P, c, ldz = sc["n"], sc["P"], sc["c"], sc["ldz"]
        vec = c % 4 == 0 and ldz % 4 == 0 and offs["z"] == 0
        run.form = "Vec<4>" if vec else "Vec<1>"
        chunks = N.stats_chunks(P, c)
        _, z = _rows(n * P, c, ldz, offs["z"], f32, 7.0)
        z.copy_(O.data((n * P, c), density=min(1.0, 2.0 ** 22 / (9.0 * n * P))))
        pb, part = _flat(n * chunks * 2 * c, f32, offs["partials"], float("nan"))
        assert L_.mpgan_channel_stats(z.data_ptr(), ldz, n, P, c, part.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        want, mag = N.channel_stats_rows(z.double().reshape(n, P, c), chunks)
        L = N.chain_length("reduce", P=P, C=c, vec=vec)
        got = part.view(-1, 2, c)
        run.ratio("rows", N.check_sums(got, want, mag, 0 if X else L + 1, exact=X))
        run.guard("partials guard", pb, part)

    elif E in ("norm_finalize", "norm_finalize_strided"):
        n, chunks, c, P, inst = sc["n"], sc["chunks"], sc["c"], sc["P"], sc["instance"]
        W = sc.get("cstride", c)
        form, _ = N.finalize_form(n, chunks, inst)
        run.form = form + (f" cstride {W}" if W != c else "")
        nrows = n * chunks
        rows, s, mag, per_n = _synthetic_rows(O, n, P, c, chunks, W, X)
        cap = (nrows + N.COMPACT_ROWS) * 2 * W
        pb, part = _flat(cap, f32, offs["partials"], float("nan"))
        part[:nrows * 2 * W].copy_(rows.reshape(-1))
        m = n * c if inst else c
        gamma = O.scale((c,)) if "gamma" in offs else None
        beta = O.shift((c,)) if "beta" in offs else None
        gv = _vec(gamma, offs["gamma"]) if gamma is not None else None
        bv = _vec(beta, offs["beta"]) if beta is not None else None
        rm0 = O.shift((c,)) if "rm" in offs else None
        rv0 = (O.invstd((c,)) if "rv" in offs else None)
        rmv = _vec(rm0, offs["rm"]) if rm0 is not None else None
        rvv = _vec(rv0, offs["rv"]) if rv0 is not None else None
        nbt = None
        if "nbt" in offs:
            _, nbt = _flat(1, torch.int64, offs["nbt"], 0)
            nbt.fill_(5)
        outs = {k: _flat(m, f32, offs[k], float("nan")) for k in ("scale", "shift", "mean", "invstd")}
        eps, mom = sc["eps"], sc["momentum"]
        args = [part.data_ptr(), n, chunks, c] + ([W] if E.endswith("strided") else []) + [
            P, inst, gv.data_ptr() if gv is not None else None, bv.data_ptr() if bv is not None else None, eps, mom,
            rmv.data_ptr() if rmv is not None else None, rvv.data_ptr() if rvv is not None else None,
            nbt.data_ptr() if nbt is not None else None] + [outs[k][1].data_ptr() for k in ("scale", "shift", "mean",
                                                                                            "invstd")]
        assert getattr(L_, e)(*args, stream) == 0
        torch.cuda.synchronize()
        L = 0 if X else -(-P // chunks) + N.chain_length("finalize", n=n, chunks=chunks, instance=inst)
        g64 = gamma.double() if gamma is not None else torch.ones(c, dtype=torch.float64, device="cuda")
        b64 = beta.double() if beta is not None else torch.zeros(c, dtype=torch.float64, device="cuda")
        groups = [(slice(i * c, (i + 1) * c), per_n[i][0], per_n[i][1], P) for i in range(n)] if inst else \
            [(slice(0, c), s, mag, n * P)]
        worst = {}
        for sl, si, mi, cnt in groups:
            got = {k: outs[k][1][sl] for k in outs}
            track = rm0 is not None and not inst
            if track:
                got["running_mean"], got["running_var"] = rmv, rvv
            res = N.finalize_check(got, si[0], mi[0], si[1], cnt, eps, g64, b64, L, exact=X,
                                   rm=rm0.double() if track else None, rv=rv0.double() if track else None,
                                   momentum=mom)
            for k, v in res.items():
                if k not in worst or not v[0] or v[1] > worst[k][1]:
                    worst[k] = v if (k not in worst or worst[k][0]) else worst[k]
        for k, v in worst.items():
            run.ratio(k, v)
        if nbt is not None:
            run.note("num_batches_tracked", int(nbt.item()) == 6, f"{int(nbt.item())} (5 before)")
        run.guard("partials guard (behind the compact scratch)", pb, part)
        for k, (b_, v_) in outs.items():
            run.guard(f"{k} guard", b_, v_)

    elif E == "norm_act_add":
        n, P, c = sc["n"], sc["P"], sc["c"]
        vec = c % 4 == 0 and all(sc[k] % 4 == 0 for k in ("ldz", "ldo")) and offs["z"] == 0 and offs["out"] == 0 and \
            ("r" not in offs or (sc["ldr"] % 4 == 0 and offs["r"] == 0))
        run.form = "Vec<4>" if vec else "Vec<1>"
        _, z = _rows(n * P, c, sc["ldz"], offs["z"], f32, 7.0)
        z.copy_(O.data((n * P, c)))
        rt = None
        if "r" in offs:
            _, rt = _rows(n * P, c, sc["ldr"], offs["r"], f32, 7.0)
            rt.copy_(O.data((n * P, c)))
        ob, out = _rows(n * P, c, sc["ldo"], offs["out"], f32, float("nan"))
        keep, pz, pr = [], None, None
        zz = z.double().reshape(n, P, c)
        rr = rt.double().reshape(n, P, c) if rt is not None else None
        sz = hz = sr = hr = None
        slz = slr = 1.0
        actz = actr = N.ACT_NONE
        if "pz" in r["pro"]:
            pz, sz, hz, slz, k_ = _pro_vectors(O, r["pro"]["pz"], n, c, offs, "pz")
            actz = r["pro"]["pz"][1]
            keep.append(k_)
        if "pr" in r["pro"]:
            pr, sr, hr, slr, k_ = _pro_vectors(O, r["pro"]["pr"], n, c, offs, "pr")
            actr = r["pro"]["pr"][1]
            keep.append(k_)
        assert L_.mpgan_norm_act_add(z.data_ptr(), sc["ldz"], C.byref(pz) if pz else None,
                                     rt.data_ptr() if rt is not None else None, sc.get("ldr", 0),
                                     C.byref(pr) if pr else None, n, P, c, sc["tanh"], out.data_ptr(), sc["ldo"],
                                     stream) == 0
        torch.cuda.synchronize()
        want, mag = N.norm_act_add(zz, sz, hz, actz, slz, rr, sr, hr, actr, slr)
        got = out.double().reshape(n, P, c)
        if sc["tanh"]:
            ok, rr_ = N.within(got, torch.tanh(want), 4 * U * mag + 2.0 ** -21)
            run.ratio("out (tanh)", (ok, rr_))
        elif X:
            run.exact("out", got, want)
        else:
            run.ratio("out", N.within(got, want, 4 * U * mag))
        run.guard("out outside its view", ob, out)

    elif E in ("norm_bwd_reduce", "norm_bwd_apply"):
        n, P, c = sc["n"], sc["P"], sc["c"]
        p = r["pro"]["pro"]
        pitches = [sc["ldg"], sc["ldz"]] + ([sc["lddz"]] if E == "norm_bwd_apply" else [])
        ptr_names = ["g", "z"] + (["dz"] if E == "norm_bwd_apply" else [])
        vec = c % 4 == 0 and all(x % 4 == 0 for x in pitches) and all(offs[k] == 0 for k in ptr_names)
        run.form = "Vec<4>" if vec else "Vec<1>"
        inplace = ("dz", "g") in r["alias"]
        density = min(1.0, 2.0 ** 13 / (n * P)) if X else 1.0
        gb, g = _rows(n * P, c, sc["ldg"], offs["g"], f32, 7.0)
        g.copy_(O.data((n * P, c), density))
        _, z = _rows(n * P, c, sc["ldz"], offs["z"], f32, 7.0)
        z.copy_(O.ints((n * P, c)) if X else O.offset((n * P, c)))
        pc, s_, h_, sl, k_ = _pro_vectors(O, p, n, c, offs, "pro")
        rows_v = n if p[0] else 1
        mean = O.shift((rows_v, c)) if X else O.u(rows_v, c) * 10
        inv = O.invstd((rows_v, c))
        mv, iv = _vec(mean, offs["mean"]), _vec(inv, offs["invstd"])
        g64, z64 = g.double().reshape(n, P, c), z.double().reshape(n, P, c)
        m64, i64 = mean.double().reshape(rows_v, 1, c), inv.double().reshape(rows_v, 1, c)
        if E == "norm_bwd_reduce":
            chunks = N.stats_chunks(P, c)
            pb, part = _flat(n * chunks * (3 * c + 1), f32, offs["partials"], float("nan"))
            assert L_.mpgan_norm_bwd_reduce(g.data_ptr(), sc["ldg"], z.data_ptr(), sc["ldz"], C.byref(pc), mv.data_ptr(),
                                            iv.data_ptr(), None, n, P, c, part.data_ptr(), stream) == 0
            torch.cuda.synchronize()
            want, mag, slopes = N.norm_bwd_reduce_rows(g64, z64, s_, h_, m64, i64, p[1], sl, chunks)
            L = N.chain_length("reduce3", P=P, C=c, vec=vec)
            got = part[:n * chunks * 3 * c].view(-1, 3, c)
            run.ratio("rows", N.check_sums(got, want, mag, 0 if X else L + 4, exact=X))
            smag = mag[:, 2].sum(-1)
            run.ratio("slope scalars", N.check_sums(part[n * chunks * 3 * c:], slopes, smag,
                                                    0 if X else L + 4 + -(-c // 64) + 7, exact=X))
            run.guard("partials guard", pb, part)
        else:
            c1 = O.shift((rows_v, c)) if X else O.u(rows_v, c)
            c2 = O.shift((rows_v, c)) if X else O.u(rows_v, c)
            c1v, c2v = _vec(c1, offs["c1"]), _vec(c2, offs["c2"])
            if inplace:
                db, dz = gb, g
            else:
                db, dz = _rows(n * P, c, sc["lddz"], offs["dz"], f32, float("nan"))
            assert L_.mpgan_norm_bwd_apply(g.data_ptr(), sc["ldg"], z.data_ptr(), sc["ldz"], C.byref(pc), mv.data_ptr(),
                                           iv.data_ptr(), c1v.data_ptr(), c2v.data_ptr(), None, n, P, c, dz.data_ptr(),
                                           sc["lddz"], stream) == 0
            torch.cuda.synchronize()
            want, mag = N.norm_bwd_apply(g64, z64, s_, h_, m64, i64, c1.double().reshape(rows_v, 1, c),
                                         c2.double().reshape(rows_v, 1, c), p[1], sl)
            got = dz.double().reshape(n, P, c)
            if X:
                run.exact("dz" + (" (in place)" if inplace else ""), got, want)
            else:
                run.ratio("dz" + (" (in place)" if inplace else ""), N.within(got, want, 6 * U * mag))
            if not inplace:
                run.guard("dz outside its view", db, dz)

    elif E == "norm_bwd_finalize":
        n, chunks, c, P, inst = sc["n"], sc["chunks"], sc["c"], sc["P"], sc["instance"]
        nrows = n * chunks
        run.form = "wide" if (not inst and nrows >= N.WIDE_BWD_FINALIZE) else "narrow"
        has_slope = "dslope" in offs
        vals = O.ints((nrows, 3, c)) if X else O.u(nrows, 3, c)
        sc_rows = O.ints((nrows,)) if X else O.u(nrows)
        pb, part = _flat(nrows * 3 * c + (nrows if has_slope else 0), f32, offs["partials"], float("nan"))
        part[:nrows * 3 * c].copy_(vals.reshape(-1))
        if has_slope:
            part[nrows * 3 * c:].copy_(sc_rows)
        m = n * c if inst else c
        olds = {}
        for k, sz in (("dgamma", c), ("dbeta", c), ("dslope", 1)):
            if k in offs:
                ob, ov = _flat(sz, f32, offs[k], float("nan"))
                o = O.ints((sz,)) if X else O.u(sz)
                ov.copy_(o)
                olds[k] = (o.double(), ob, ov)
        c1b, c1 = _flat(m, f32, offs["c1"], float("nan"))
        c2b, c2 = _flat(m, f32, offs["c2"], float("nan"))
        p_ = lambda k: olds[k][2].data_ptr() if k in olds else None
        assert L_.mpgan_norm_bwd_finalize(part.data_ptr(), n, chunks, c, P, inst, p_("dgamma"), p_("dbeta"),
                                          p_("dslope"), c1.data_ptr(), c2.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        v64 = vals.double()
        if inst:
            per = v64.reshape(n, chunks, 3, c).sum(1)          # (n, 3, c)
            c1w, c2w = (per[:, 0] / P).reshape(-1), (per[:, 1] / P).reshape(-1)
            tot = per.sum(0)
        else:
            tot = v64.sum(0)
            c1w, c2w = tot[0] / (n * P), tot[1] / (n * P)
        run.ratio("c1", N.within_ulps(c1, c1w, c1w, 0.51))
        run.ratio("c2", N.within_ulps(c2, c2w, c2w, 0.51))
        for k, q in (("dgamma", tot[1]), ("dbeta", tot[0]), ("dslope", sc_rows.double().sum().reshape(1))):
            if k in olds:
                o, ob, ov = olds[k]
                want = o + q
                if X:
                    run.exact(k + " (accumulated)", ov, want)
                else:
                    run.ratio(k + " (accumulated)", N.within_ulps(ov, want, o.abs() + q.abs(), 1.0))
                run.guard(k + " guard", ob, ov)
        run.guard("c1 guard", c1b, c1)
        run.guard("c2 guard", c2b, c2)

    elif E in ("norm_act_bf16", "norm_bwd_reduce_bf16", "norm_bwd_apply_bf16"):
        rows, c = sc["rows"], sc["c"]
        slope = 0.25 if X else sc["slope"]
        s32 = float(torch.tensor(slope, dtype=f32))
        _, z = _rows(rows, c, sc["ldz"], offs["z"], bf, 7.0)
        if E == "norm_act_bf16":
            z.copy_(O.ints((rows, c), -100, 100) if X else O.offset((rows, c)))
        else:
            z.copy_(O.ints((rows, c)) if X else O.offset((rows, c)))
        scl = O.scale((c,))
        sh = (O.ints((c,), -8, 8) * 0.125) if X else O.shift((c,))
        vs, vh = _vec(scl, offs["scale"]), _vec(sh, offs["shift"])
        z64 = z.double()
        if E == "norm_act_bf16":
            out_f32 = sc["out_f32"]
            odt = f32 if out_f32 else bf
            run.form = "fp32 out" if out_f32 else "bf16 out"
            ob, out = _rows(rows, c, sc["ldo"], offs["out"], odt, float("nan"))
            assert L_.mpgan_norm_act_bf16(z.data_ptr(), sc["ldz"], vs.data_ptr(), vh.data_ptr(), slope, rows, c,
                                          out.data_ptr(), sc["ldo"], out_f32, stream) == 0
            torch.cuda.synchronize()
            want = N.norm_act_bf16(z64, scl.double(), sh.double(), s32)
            mag = (z64.abs() * scl.double().abs() + sh.double().abs())
            if X:
                run.exact("out", out, want if out_f32 else N.bf16_rne(want))
            else:
                acc = 3 * U * mag
                run.ratio("out", N.within(out, want, (0 if out_f32 else 2.0 ** -8) * (want.abs() + acc) + acc))
            run.guard("out outside its view", ob, out)
        else:
            g_f32 = sc["g_f32"]
            gdt = f32 if g_f32 else bf
            run.form = "g fp32" if g_f32 else "g bf16"
            density = min(1.0, 2.0 ** 14 / rows) if X else 1.0
            gb, g = _rows(rows, c, sc["ldg"], offs["g"], gdt, 7.0)
            g.copy_(O.ints((rows, c), density=density) if X else O.u(rows, c))
            mean = O.shift((c,)) if X else O.u(c) * 10
            inv = O.invstd((c,))
            mv, iv = _vec(mean, offs["mean"]), _vec(inv, offs["invstd"])
            g64 = g.double()
            nb_ = N.bwd_rows_bf16(rows, c)
            if E == "norm_bwd_reduce_bf16":
                pb, part = _flat(nb_ * 3 * c, f32, offs["partials"], float("nan"))
                assert L_.mpgan_norm_bwd_reduce_bf16(g.data_ptr(), g_f32, sc["ldg"], z.data_ptr(), sc["ldz"], vs.data_ptr(),
                                                     vh.data_ptr(), mv.data_ptr(), iv.data_ptr(), slope, rows, c,
                                                     part.data_ptr(), stream) == 0
                torch.cuda.synchronize()
                want, mag, _ = N.norm_bwd_reduce_rows(g64[None], z64[None], scl.double(), sh.double(), mean.double(),
                                                      inv.double(), N.ACT_LEAKY, s32, nb_, third=False)
                L = N.chain_length("reduce_bf16", C=c, rows=rows)
                run.ratio("rows", N.check_sums(part.view(-1, 3, c), want, mag, 0 if X else L + 4, exact=X))
                run.guard("partials guard", pb, part)
            else:
                c1 = O.shift((c,)) if X else O.u(c)
                c2 = O.shift((c,)) if X else O.u(c)
                c1v, c2v = _vec(c1, offs["c1"]), _vec(c2, offs["c2"])
                inplace = ("dz", "g") in r["alias"]
                if inplace:
                    db, dz = gb, g
                else:
                    db, dz = _rows(rows, c, sc["lddz"], offs["dz"], bf, float("nan"))
                bp = None
                if "bias_partials" in offs:
                    bpb, bp = _flat(nb_ * c, f32, offs["bias_partials"], float("nan"))
                assert L_.mpgan_norm_bwd_apply_bf16(g.data_ptr(), g_f32, sc["ldg"], z.data_ptr(), sc["ldz"], vs.data_ptr(),
                                                    vh.data_ptr(), mv.data_ptr(), iv.data_ptr(), c1v.data_ptr(),
                                                    c2v.data_ptr(), slope, rows, c, dz.data_ptr(), sc["lddz"],
                                                    bp.data_ptr() if bp is not None else None, stream) == 0
                torch.cuda.synchronize()
                want, mag = N.norm_bwd_apply(g64, z64, scl.double(), sh.double(), mean.double(), inv.double(),
                                             c1.double(), c2.double(), N.ACT_LEAKY, s32)
                if X:
                    run.exact("dz (bf16)", dz, N.bf16_rne(want))
                else:
                    acc = 6 * U * mag
                    run.ratio("dz (bf16)", N.within(dz, want, 2.0 ** -8 * (want.abs() + acc) + acc))
                if bp is not None:
                    R_ = 256 // (c // 8)
                    bw, bm = N.bias_partials_bf16(dz.double(), nb_, R_)
                    L = N.chain_length("bias_bf16", C=c, rows=rows)
                    ex = X and N.exact_sums_ok(bm, 8)
                    run.ratio("bias partials", N.check_sums(bp.view(nb_, c), bw, bm, 0 if ex else L, exact=ex))
                    run.guard("bias partials guard", bpb, bp)
                if not inplace:
                    run.guard("dz outside its view", db, dz)

    elif E == "reduce_partials":
        rows, rs, c, beta = sc["rows"], sc["row_stride"], sc["c"], sc["beta"]
        vals = O.ints((rows * rs,)) if X else O.u(rows * rs)
        _, part = _flat(rows * rs, f32, offs["partials"], 0)
        part.copy_(vals)
        ob, out = _flat(c, f32, offs["out"], float("nan"))
        old = O.ints((c,)) if X else O.u(c)
        out.copy_(old)
        assert L_.mpgan_reduce_partials(part.data_ptr(), rows, rs, c, out.data_ptr(), beta, stream) == 0
        torch.cuda.synchronize()
        want, mag = N.reduce_partials(old.double(), beta, vals.double(), rows, rs, c)
        if X:
            run.exact("out = beta old + sum", out, want)
        else:
            run.ratio("out = beta old + sum", N.within_ulps(out, want, mag, 1.5))
        run.guard("out guard", ob, out)

    elif E in ("linear1_forward", "linear1_backward"):
        n, P, c = sc["n"], sc["P"], sc["c"]
        F_ = P * c
        _, z = _flat(n * F_, f32, offs["z"], 7.0)
        z.copy_((O.ints((n * F_,)) if X else O.offset((n * P, c)).reshape(-1)))
        _, w = _flat(F_, f32, offs["w"], 7.0)
        w.copy_(O.ints((F_,), density=min(1.0, 2.0 ** 14 / F_)) if X else O.u(F_) / math.sqrt(F_))
        a64 = z.double().reshape(n, P, c)
        keep = None
        run.form = "prologue" if "pro" in r["pro"] else "plain"
        pcref = None
        if "pro" in r["pro"]:
            pc, s_, h_, sl, keep = _pro_vectors(O, r["pro"]["pro"], n, c, offs, "pro")
            pcref = C.byref(pc)
            amag = (a64.abs() * s_.abs() + h_.abs()) * max(sl, 1.0)
            a64 = N.act(a64 * s_ + h_, r["pro"]["pro"][1], sl)
        else:
            amag = a64.abs()
        a64, amag = a64.reshape(n, F_), amag.reshape(n, F_)
        w64 = w.double()
        if E == "linear1_forward":
            bias = O.ints((1,)) if X else O.u(1)
            bv = _vec(bias, offs.get("bias", 0)) if "bias" in offs else None
            _, part = _flat(n * 64, f32, offs["partials"], float("nan"))
            lb, logit = _flat(n, f32, offs["logit"], float("nan"))
            pb = prob = None
            if "prob" in offs:
                pb, prob = _flat(n, f32, offs["prob"], float("nan"))
            assert L_.mpgan_linear1_forward(z.data_ptr(), pcref, n, P, c, w.data_ptr(),
                                            bv.data_ptr() if bv is not None else None, part.data_ptr(), logit.data_ptr(),
                                            prob.data_ptr() if prob is not None else None, stream) == 0
            torch.cuda.synchronize()
            want, mag = N.linear1_forward(a64, w64)
            if bv is not None:
                want, mag = want + bias.double(), mag + bias.double().abs()
            per = -(-(F_ // 4) // 64) * 4
            L = 4 * -(-per // 1024) + 9 + 64 + 1 + (3 if keep is not None else 0)
            if X:
                run.exact("logit", logit, want)
            else:
                run.ratio("logit", N.within(logit, want, (L + 1) * U * (w64.abs() * amag).sum(1)))
            if prob is not None:
                pw = torch.sigmoid(logit.double())
                run.ratio("prob = sigmoid(logit)", N.within(prob, pw, 4 * U * pw + 2.0 ** -30))
                run.guard("prob guard", pb, prob)
            run.guard("logit guard", lb, logit)
        else:
            beta = sc["beta"]
            dl = O.ints((n,)) * 0.5 if X else O.u(n)
            dlv = _vec(dl, offs["dlogit"])
            gab = ga = dwb = dw = dbb = db = None
            if "g_a" in offs:
                gab, ga = _flat(n * F_, f32, offs["g_a"], float("nan"))
            old_w = O.ints((F_,)) if X else O.u(F_)
            old_b = O.ints((1,)) if X else O.u(1)
            if "dw" in offs:
                dwb, dw = _flat(F_, f32, offs["dw"], float("nan"))
                dw.copy_(old_w)
            if "dbias" in offs:
                dbb, db = _flat(1, f32, offs["dbias"], float("nan"))
                db.copy_(old_b)
            pp = lambda t: t.data_ptr() if t is not None else None
            assert L_.mpgan_linear1_backward(z.data_ptr(), pcref, n, P, c, w.data_ptr(), dlv.data_ptr(), pp(ga), pp(dw),
                                             pp(db), beta, stream) == 0
            torch.cuda.synchronize()
            g_a, dww, dwm, dbw, dbm, _ = N.linear1_backward(a64, w64, dl.double(), old_w.double(), old_b.double(), beta,
                                                            P, c)
            if ga is not None:
                if X:
                    run.exact("g_a", ga.view(n, F_), g_a)
                else:
                    run.ratio("g_a", N.within(ga.view(n, F_), g_a, U * g_a.abs()))
                run.guard("g_a guard", gab, ga)
            if dw is not None:
                mag = abs(beta) * old_w.double().abs() + (dl.double().abs()[:, None] * amag).sum(0).reshape(P, c).t().reshape(-1)
                if X:
                    run.exact("dW (beta = 1 onto known values)", dw, dww)
                else:
                    run.ratio("dW (beta = 1 onto known values)", N.within(dw, dww, (n + 2 + (3 if keep else 0)) * U * mag))
                run.guard("dW guard", dwb, dw)
            if db is not None:
                if X:
                    run.exact("dbias", db, dbw)
                else:
                    run.ratio("dbias", N.within(db, dbw, (n + 2) * U * dbm))
                run.guard("dbias guard", dbb, db)

    elif E in ("sigmoid_backward", "tanh_backward"):
        n = sc.get("n", sc.get("numel"))
        a_name, b_name, o_name = ("dprob", "prob", "dlogit") if E == "sigmoid_backward" else ("g", "y", "dx")
        _, a = _flat(n, f32, offs[a_name], 0)
        a.copy_(O.ints((n,)) if X else O.u(n))
        _, b = _flat(n, f32, offs[b_name], 0)
        b.copy_((O.ints((n,), 0, 4) * 0.25) if X else (torch.rand(n, generator=O.gen, device="cuda") if
                                                      E == "sigmoid_backward" else O.u(n)))
        ob, o = _flat(n, f32, offs[o_name], float("nan"))
        assert getattr(L_, e)(a.data_ptr(), b.data_ptr(), n, o.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        A, B = a.double(), b.double()
        want = N.sigmoid_backward(A, B) if E == "sigmoid_backward" else N.tanh_backward(A, B)
        mag = A.abs() * (1 + B.abs()) * (B.abs() + (1 if E == "tanh_backward" else 0))
        if X:
            run.exact(o_name, o, want)
        else:
            run.ratio(o_name, N.within(o, want, 4 * U * mag))
        run.guard(o_name + " guard", ob, o)

    elif E == "pack_weights_bf16":
        t = r["table"].clone()
        src_need = int(max(int(x[0]) + int(x[2]) * int(x[3]) * int(x[4]) for x in t))
        dst_need = int(max(int(x[1]) + int(x[2]) * int(x[3]) * int(x[4]) for x in t))
        _, src = _flat(src_need, f32, offs["src"], 0)
        src.copy_(O.u(src_need) * (1 if X else 3) + (2.0 ** -12 if X else 0))
        db_, dst = _flat(dst_need, bf, offs["dst"], float("nan"))
        tv = _vec(t.cuda(), offs.get("table", 0))
        assert L_.mpgan_pack_weights_bf16(src.data_ptr(), dst.data_ptr(), tv.data_ptr(), t.shape[0], sc["max_elems"],
                                          stream) == 0
        torch.cuda.synchronize()
        want = torch.full((dst_need,), float("nan"), dtype=bf, device="cuda")
        for x in t.tolist():
            so, do, co, ci, T, tr, lay = x[:7]
            wt = src[so:so + co * ci * T].view((ci, co, T) if tr else (co, ci, T))
            wt = wt.permute(1, 0, 2) if tr else wt
            want[do:do + co * ci * T] = N.pack_weights_bf16(wt, lay)
        ok = torch.equal(dst.view(torch.int16), want.view(torch.int16)) or bool(
            ((dst.float() == want.float()) | (torch.isnan(dst.float()) & torch.isnan(want.float()))).all())
        run.note("packed (bit-exact RNE, gaps untouched)", ok, "exact" if ok else "DIFFERS")
        run.form = "layouts " + ",".join(sorted({str(int(x[6])) for x in t}))
        run.guard("dst guard", db_, dst)

    elif E == "epi_vectors_multi":
        t = r["table"]
        rows_t, keep, chk = [], [], []
        for x in t.tolist():
            c_norm, c_total, eps_bits = int(x[9]), int(x[10]), int(x[11])
            eps = struct.unpack("<f", struct.pack("<I", eps_bits & 0xFFFFFFFF))[0]
            mk = lambda present, v: (_vec(v) if present else None)
            gamma = mk(x[0], O.scale((c_total,)))
            beta = mk(x[1], O.shift((c_total,)))
            rm = mk(x[2], O.shift((c_total,)) * 4)
            rv = mk(x[3], O.invstd((c_total,)) + (0 if X else 0.1))
            bias = mk(x[4], O.shift((c_total,)))
            alpha = mk(x[5], torch.full((1,), 0.25, device="cuda"))
            outs = [_flat(-(-c_total // 4) * 4, f32, 0, float("nan")) for _ in range(3)]
            p = lambda v: v.data_ptr() if v is not None else 0
            rows_t.append([p(gamma), p(beta), p(rm), p(rv), p(bias), p(alpha)] + [o[1].data_ptr() for o in outs] +
                          [c_norm, c_total, eps_bits])
            keep += [gamma, beta, rm, rv, bias, alpha, outs]
            chk.append((gamma, beta, rm, rv, bias, alpha, outs, c_norm, c_total, eps))
        tab = torch.tensor(rows_t, dtype=torch.int64, device="cuda")
        assert L_.mpgan_epi_vectors_multi(tab.data_ptr(), tab.shape[0], stream) == 0
        torch.cuda.synchronize()
        worst, lin_ok = {"scale": (True, 0.0), "shift": (True, 0.0)}, True
        for gamma, beta, rm, rv, bias, alpha, outs, c_norm, c_total, eps in chk:
            cpu = lambda v: v.cpu() if v is not None else None
            sc_w, sh_w, sl_w = N.epi_vectors(cpu(gamma), cpu(beta), cpu(rm), cpu(rv), cpu(bias),
                                             float(alpha.item()) if alpha is not None else None, c_norm, c_total, eps)
            got = [o[1][:c_total].double().cpu() for o in outs]
            lin_ok &= torch.equal(got[0][c_norm:], sc_w[c_norm:]) and torch.equal(got[1][c_norm:], sh_w[c_norm:]) and \
                torch.equal(got[2][c_norm:], sl_w[c_norm:]) and torch.equal(got[2][:c_norm], sl_w[:c_norm])
            if c_norm:
                r1 = N.within_ulps(got[0][:c_norm], sc_w[:c_norm], sc_w[:c_norm], 3)
                bi = (bias.double().cpu() if bias is not None else torch.zeros(c_total, dtype=torch.float64))[:c_norm]
                be = (beta.double().cpu() if beta is not None else torch.zeros(c_total, dtype=torch.float64))[:c_norm]
                d = bi - rm.double().cpu()[:c_norm]
                yw = be + d * got[0][:c_norm]
                r2 = N.within_ulps(got[1][:c_norm], yw, be.abs() + (d * got[0][:c_norm]).abs(), 2)
                for k, v in (("scale", r1), ("shift", r2)):
                    if not v[0] or v[1] > worst[k][1]:
                        worst[k] = v if worst[k][0] else worst[k]
            for b_, v_ in outs:
                if not _untouched(b_, v_[:c_total]):
                    lin_ok = False
        run.note("channels >= c_norm: (1, bias, 1); slope; guards", lin_ok, "exact" if lin_ok else "WRONG")
        for k, v in worst.items():
            run.ratio(k + " (c < c_norm)", v)
        run.form = f"{t.shape[0]} table rows"

    elif E == "l1_loss":
        from mpgan_amd import ops
        nel, gsc = sc["numel"], sc["grad_scale"]
        a = O.ints((nel,)) * 0.25 if X else O.u(nel)
        b = O.ints((nel,)) * 0.25 if X else O.u(nel)
        part = torch.full((ops.l1_partials() + GUARD,), float("nan"), device="cuda")
        loss = torch.full((1,), float("nan"), device="cuda")
        grad = torch.full((nel,), float("nan"), device="cuda") if sc["grad"] else None
        ops.l1_loss(a, b, part, loss, grad, gsc)
        torch.cuda.synchronize()
        lw, gw = N.l1_loss(a.double(), b.double(), gsc)
        mag = (a.double() - b.double()).abs().mean()
        blocks = min(-(-nel // 256), 1024)
        L = -(-nel // (blocks * 256)) + 10
        run.ratio("loss", N.within(loss, lw.reshape(1), (L + 2) * U * mag.reshape(1) + 0.5 * N.ulp(lw.reshape(1))))
        if grad is not None:
            g32 = torch.sign(a.double() - b.double()) * float(torch.tensor(gsc, dtype=f32) / torch.tensor(float(nel),
                                                                                                          dtype=f32))
            run.exact("grad (sign * scale / numel)", grad, g32)
        run.note("partials guard", bool(torch.isnan(part[blocks:]).all()), "untouched")

    elif E in ("bce_forward", "bce_backward"):
        from mpgan_amd import ops
        n = sc["n"]
        p = torch.rand(n, generator=O.gen, device="cuda")
        p[0] = 0.0                                              # log(0) and log(1 - 1): the -100 clamp
        if n > 1:
            p[1] = 1.0
        t = (torch.rand(n, generator=O.gen, device="cuda") < 0.5).float()
        if E == "bce_forward":
            loss = torch.full((1,), float("nan"), device="cuda")
            ops.bce_forward(p, t, loss)
            torch.cuda.synchronize()
            want = N.bce_forward(p.double(), t.double())
            lp = torch.clamp(torch.log(p.double()), min=-100).abs() + torch.clamp(torch.log1p(-p.double()), min=-100).abs()
            run.ratio("loss (log clamped at -100)", N.within(loss, want.reshape(1), ((12 + 8) * U * lp.mean()).reshape(1)))
        else:
            gout = _vec(torch.tensor([0.75], device="cuda"))
            dp = torch.full((n,), float("nan"), device="cuda")
            ops.bce_backward(p, t, gout, dp)
            torch.cuda.synchronize()
            want = N.bce_backward(p.double(), t.double(), 0.75)
            run.ratio("dprob", N.within(dp, want, 6 * U * want.abs() + 1e-30))

    elif E == "adam_step":
        from mpgan_amd import ops
        nel = sc["numel"]
        for step in (1, 1000):
            p = O.u(nel)
            g = O.u(nel) * 1e-2
            m = O.u(nel) * 1e-3 if step > 1 else torch.zeros(nel, device="cuda")
            v = torch.rand(nel, generator=O.gen, device="cuda") * 1e-4 if step > 1 else torch.zeros(nel, device="cuda")
            P64, M64, V64 = p.double(), m.double(), v.double()
            ops.adam_step(p, g, m, v, sc["lr"], sc["b1"], sc["b2"], sc["eps"], step, sc["grad_scale"])
            torch.cuda.synchronize()
            pw, mw, vw = N.adam_step(P64, g.double(), M64, V64, sc["lr"], sc["b1"], sc["b2"], sc["eps"], step,
                                     sc["grad_scale"])
            upd = (P64 - pw).abs()
            run.ratio(f"p (step {step})", N.within(p, pw, 2 * U * P64.abs() + 16 * U * upd))
            run.ratio(f"m (step {step})", N.within(m, mw, 4 * U * (M64.abs() + g.double().abs())))
            run.ratio(f"v (step {step})", N.within(v, vw, 4 * U * (V64.abs() + g.double() ** 2)))
    else:
        raise AssertionError(f"no replayer for {e}")

    torch.cuda.synchronize()
    print(f"  [{tier}] {r['label']:<30} {E:<24} {run.form:<18} {'; '.join(run.res)}  "
          f"({time.time() - t0:.1f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB)", flush=True)
    return run.fails


CONFIGS = ("c5-train", "c5-eval", "c3")
# calls per entry in one step (the plans only; the out-of-plan ops are checked for presence)
EXPECTED = {
    "c3": {"norm_finalize_strided": 321, "norm_finalize": 3, "norm_act_add": 168, "norm_bwd_reduce": 159,
           "norm_bwd_finalize": 168, "norm_bwd_apply": 168, "channel_stats": 39, "reduce_partials": 36,
           "linear1_forward": 3, "linear1_backward": 3, "sigmoid_backward": 3, "tanh_backward": 1},
    "c5-train": {"norm_finalize_strided": 288, "norm_finalize": 36, "norm_act_add": 168, "norm_bwd_reduce": 156,
                 "norm_bwd_finalize": 168, "norm_bwd_apply": 156, "channel_stats": 60, "reduce_partials": 42,
                 "norm_act_bf16": 12, "norm_bwd_reduce_bf16": 12, "norm_bwd_apply_bf16": 12, "linear1_forward": 3,
                 "linear1_backward": 3, "sigmoid_backward": 3, "tanh_backward": 1, "pack_weights_bf16": 3},
    "c5-eval": {"epi_vectors_multi": 1},
}


def _launch_id(cfg, r):
    desc = r["label"].replace("->", "to").replace(" ", "-")
    return f"{cfg}-{desc}-{r['entry'].replace('mpgan_', '')}"


def pytest_generate_tests(metafunc):
    if "launch" not in metafunc.fixturenames:
        return
    cases, ids = [], []
    if torch.cuda.is_available():
        try:
            for cfg in CONFIGS:
                for r in _inventory(cfg):
                    cases.append((cfg, r))
        except Exception as ex:
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
    """Each config's non-conv entries and their call counts per step are the expected ones, and the out-of-plan
    ops were recorded."""
    for cfg in CONFIGS:
        inv = _inventory(cfg)
        assert _COUNTS[cfg] == EXPECTED[cfg], (cfg, _COUNTS[cfg])
        if cfg != "c5-eval":
            assert set(OUT_OF_PLAN) <= {r["entry"] for r in inv}, cfg


def test_step_norm_launch_against_fp64_reference(launch):
    cfg, r = launch
    assert cfg != "inventory", r
    t0 = time.time()
    seed = 2000 + int.from_bytes(r["key"].encode()[-8:], "little") % 100000
    fails = _replay(r, "X", seed) + _replay(r, "R", seed + 1)
    print(f"[{_launch_id(cfg, r)}] {time.time() - t0:.1f} s")
    assert not fails, "\n".join(fails)
