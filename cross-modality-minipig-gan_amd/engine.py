"""Execution plans for the GAN hot path: pre-bound sequences of C-ABI calls.

A *plan* owns every activation / gradient buffer one forward (+ backward) of a
network needs for a fixed (batch, spatial) shape, and two *programs*: lists of
(C function, argument tuple) built once.  Running a network is a tight loop of
ctypes calls on the current stream -- no per-op Python logic, no per-op
allocation, graph-capturable.  Data layout in HBM: channels-last
(N, D, H, W, C) fp32; concatenations are channel slices of one buffer that the
producers write directly; only RAW conv outputs + per-channel norm vectors are
kept (BatchNorm/InstanceNorm + PReLU/LeakyReLU are applied by the consumer's
load prologue).

Graph of one U-Net follows MONAI 0.4.0 `UNet(num_res_units=2)` as the reference
instantiates it (code/GAN/GAN_final.py:106-114); the
discriminator follows code/GAN/GAN_final.py:159-209.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import struct
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops
from ._lib import lib
from .ops import ACT_LEAKY, ACT_NONE, ConvGeom, Prologue


# --------------------------------------------------------------------------
# programs
# --------------------------------------------------------------------------
class KernelProbe:
    """HIP-event timing of tagged launches (bench.py's live roofline figure):
    events are recorded on the stream the kernels are launched on."""

    def __init__(self, want=None, detail=False, min_flops=0.0):
        self.want = want            # None = every tagged call, else a set of kernel names
        self.detail = detail        # True: time EVERY call, keyed "<c entry point> <geometry>" (tools/profile_step.py)
        self.min_flops = min_flops  # only launches with at least this much algorithmic work (the dense families)
        self.samples = []           # (kernel, flops, ev0, ev1, algorithmic bytes)

    def summary(self):
        """kernel -> dict(calls, ms, flops): durations read after a synchronize."""
        out = {}
        for k, fl, e0, e1, by in self.samples:
            d = out.setdefault(k, dict(calls=0, ms=0.0, flops=0.0, bytes=0.0))
            d["calls"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += by
        return out


_PROBE: Optional[KernelProbe] = None


def set_probe(p: Optional[KernelProbe]):
    global _PROBE
    _PROBE = p


_SIDE = {}


def side_stream(device) -> "torch.cuda.Stream":
    """The second HIP stream of this device: weight-gradient kernels of the generator run here,
    next to the (latency-bound) norm-backward / backward-data chain on the caller's stream."""
    key = torch.device(device).index or 0
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


_SINGLE_STREAM = bool(os.environ.get("MPGAN_SINGLE_STREAM"))
_ALWAYS_PACK = bool(os.environ.get("MPGAN_DBG_ALWAYS_PACK"))
# BatchNorm statistics through integer accumulators + fold-on-load in the first consumer (csrc/norm_fold.h) instead of
# partial rows + a finalize launch.  Built, tested and MEASURED: the 66 finalize launches it
# removes from a generator forward (4.7-6.3 us each + a ~1.5 us boundary) are paid back in full by what it adds to
# every block of the neighbouring kernels -- the fold's load -> barrier -> double-precision finalize -> barrier sits on
# each consumer block's critical path (+3.6-5 us per launch) and the atomics on the producer's tail (+1-4 us) -- and
# same-address atomics make a 1-channel layer 8x slower (convt_quad: 28 -> 225 us).  Off unless MPGAN_ACC_STATS=1.
_ACC_STATS = bool(os.environ.get("MPGAN_ACC_STATS"))
_FUSE_DOWN = not os.environ.get("MPGAN_DBG_NO_FUSE_DOWN")   # ResidualUnit: first conv + residual conv as one launch
# The discriminator's weight gradients run on the caller's stream, one after the other with the backward-data
# launches (lane 0).  Both families are matrix-bound: side by side on two streams each only gets half the chip --
# A/B on one box, 20-step benches: 55.25 / 55.27 ms (second stream) vs 55.18 / 55.35 ms (one stream) -- and the
# per-launch figures the bench line reports are then contention-free.  MPGAN_D_WGRAD_SIDE=1 puts them back on lane 1.
_D_WGRAD_LANE = 1 if os.environ.get("MPGAN_D_WGRAD_SIDE") else 0


def same_geom(a, b) -> bool:
    return (a.n, a.in_dhw, a.cin, a.k, a.stride, a.pad, a.transposed) == (b.n, b.in_dhw, b.cin, b.k, b.stride, b.pad,
                                                                         b.transposed)


class Mark:
    """A point on the side stream another program section can wait for."""
    __slots__ = ("event", "armed")

    def __init__(self):
        self.event = torch.cuda.Event()
        self.armed = False


class Program:
    """A frozen list of C calls; `run` appends the stream and checks status.

    Calls carry a lane: 0 = the caller's stream, 1 = the side stream.  A lane-1 call first makes
    the side stream wait for everything enqueued so far on the caller's stream (event), so it
    may read anything produced before it; `join()` makes the caller's stream wait for the side
    stream.  The emitter must place a join before any buffer a lane-1 call reads is rewritten
    and before its results are consumed."""
    __slots__ = ("calls", "keep", "names", "tags", "descs", "lanes", "events")

    def __init__(self):
        self.calls = []
        self.keep = []
        self.names = []
        self.tags = []
        self.descs = []
        self.lanes = []
        self.events = {}

    def add(self, name, fn, *args, keep=(), tag=None, desc="", lane=0):
        self.calls.append((fn, args))
        self.names.append(name)
        self.keep.append(keep)
        self.tags.append(tag)
        self.descs.append(desc)
        self.lanes.append(lane)

    def join(self):
        """The caller's stream waits for everything enqueued so far on the side stream."""
        if self.calls and self.calls[-1] == (None, ("join",)):
            return
        self.add("join", None, "join")

    def mark(self, m: "Mark"):
        """Record `m` on the side stream here (a later `wait(m)` orders the caller's stream after it)."""
        self.add("mark", None, "mark", m)

    def wait(self, m: "Mark"):
        self.add("wait", None, "wait", m)

    def extend(self, other: "Program"):
        self.calls += other.calls
        self.names += other.names
        self.keep += other.keep
        self.tags += other.tags
        self.descs += other.descs
        self.lanes += other.lanes

    def rebind(self, ptr: int, slot: "C.c_void_p") -> int:
        """Replace every pointer argument equal to `ptr` by the mutable `slot` (a ctypes pointer object whose
        .value the caller sets before `run`): the caller's own tensor is then read / written in place instead
        of a plan-owned staging buffer.  Returns the number of calls touched."""
        hits = 0
        for i, (fn, args) in enumerate(self.calls):
            if fn is None or not any(type(a) is int and a == ptr for a in args):
                continue
            self.calls[i] = (fn, tuple(slot if (type(a) is int and a == ptr) else a for a in args))
            hits += 1
        return hits

    def _event(self, i):
        ev = self.events.get(i)
        if ev is None:
            ev = self.events[i] = torch.cuda.Event()
        return ev

    def run(self, stream=None):
        main = torch.cuda.current_stream()
        s = main.cuda_stream if stream is None else stream
        probe = _PROBE
        lanes = self.lanes
        multi = (stream is None and not _SINGLE_STREAM and not (probe is not None and probe.detail)
                 and 1 in lanes)
        if probe is None and not multi:            # plain program on one stream: the tight loop
            for i, (fn, args) in enumerate(self.calls):
                if fn is not None:
                    rc = fn(*args, s)
                    if rc:
                        raise RuntimeError(f"{self.names[i]} failed (status {rc}): {lib().mpgan_last_error().decode()}")
            return
        side = side_stream(main.device) if multi else None
        s1 = side.cuda_stream if multi else s
        side_busy = False
        main_dirty = True                          # the caller's stream has work the side stream has not waited for
        for i, (fn, args) in enumerate(self.calls):
            if fn is None:                         # stream bookkeeping
                kind = args[0]
                if not multi:
                    continue
                if kind == "join":
                    if side_busy:
                        ev = self._event(i)
                        ev.record(side)
                        main.wait_event(ev)
                        side_busy = False
                elif kind == "mark":
                    args[1].event.record(side)
                    args[1].armed = True
                elif args[1].armed:                # wait
                    main.wait_event(args[1].event)
                continue
            on_side = multi and lanes[i] == 1
            if on_side:
                if main_dirty:
                    ev = self._event(i)
                    ev.record(main)
                    side.wait_event(ev)
                    main_dirty = False
                side_busy = True
            else:
                main_dirty = True
            tag = self.tags[i]
            timed = False
            if probe is not None:
                if probe.detail:
                    tag = (f"{self.names[i]} {self.descs[i]}".strip(), tag[1] if tag else 0.0,
                           tag[2] if tag and len(tag) > 2 else 0.0)
                timed = (tag is not None and (probe.want is None or tag[0] in probe.want)
                         and tag[1] >= probe.min_flops)
            if timed:                              # events go on the stream the kernel is launched on
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side if on_side else main)
            rc = fn(*args, s1 if on_side else s)
            if rc:
                raise RuntimeError(f"{self.names[i]} failed (status {rc}): {lib().mpgan_last_error().decode()}")
            if timed:
                e1.record(side if on_side else main)
                probe.samples.append((tag[0], tag[1], e0, e1, tag[2] if len(tag) > 2 else 0.0))
        if side_busy:                              # never leave work un-joined behind a program
            ev = self._event(-1)
            ev.record(side)
            main.wait_event(ev)

    def __len__(self):
        return len(self.calls)


def conv_macs(g: ConvGeom) -> int:
    """Algorithmic multiply-accumulates of one conv (transposed conv counted input-side)."""
    grid = g.in_dhw if g.transposed else g.out_dhw
    return g.n * grid[0] * grid[1] * grid[2] * g.cin * g.cout * g.taps


def conv_bytes(g: ConvGeom, esize: int = 4) -> int:
    """Algorithmic HBM bytes of one conv in any direction: the gathered side read or written once
    plus the dense side read or written once; weights and norm vectors are not counted."""
    i, o = g.in_dhw, g.out_dhw
    return g.n * (i[0] * i[1] * i[2] * g.cin + o[0] * o[1] * o[2] * g.cout) * esize


def gather_kernel_name(g: ConvGeom, backward_data: bool, has_pro: bool, per_sample_norm: bool = False,
                       fast_leaky: bool = False) -> str:
    """The kernel symbol (as rocprofv3 prints it, minus `void mpgan::` and the argument list) of the instance the
    C dispatcher runs for this conv, from the same choice the launch makes (mpgan_conv_kernel_name)."""
    gc = g.c()
    pro = (2 if per_sample_norm else (3 if fast_leaky else 1)) if has_pro else 0
    return kernel_label(lib().mpgan_conv_kernel_name, C.byref(gc), int(backward_data), pro)


def wgrad_kernel_name(g: ConvGeom, pro=None, bf16_dy: bool = False) -> str:
    """rocprofv3's name of the weight-gradient instance the C dispatcher runs for this conv (bf16_dy: the entry with a
    bf16 dy), from the same choice the launch makes (mpgan_conv_wgrad_kernel_name)."""
    gc = g.c()
    code = (2 if pro.n_stride else (3 if _fast_leaky(pro) else 1)) if pro is not None else 0
    return kernel_label(lib().mpgan_conv_wgrad_kernel_name, C.byref(gc), code, int(bf16_dy))


def wgrad_kernel_name_at(g: ConvGeom, x, dy, pro=None) -> str:
    """The same label for these very operands (mpgan_conv_wgrad_kernel_name_at): the pitches, base alignment and
    prologue of x and dy decide as they do in the launch; a bf16 dy names the bf16-dy entry's instance."""
    gc = g.c()
    bf16_dy = dy.dtype == torch.bfloat16
    lddy = ops._clx(dy, dy.dtype, "wgrad_kernel_name_at dy")[2]
    return kernel_label(lib().mpgan_conv_wgrad_kernel_name_at, C.byref(gc), x.data_ptr(), _ld(x), ops._pro(pro),
                        dy.data_ptr(), lddy, int(bf16_dy))


def kernel_label(entry, *args) -> str:
    """The label a mpgan_conv_kernel_name* entry writes for these arguments."""
    buf = C.create_string_buffer(160)
    if entry(*args, buf, len(buf)):
        raise RuntimeError(lib().mpgan_last_error().decode())
    return buf.value.decode()


def _ld(t):
    return 0 if t is None else ops._cl(t, "plan tensor")[2]


def _p(t):
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------
# parameter storage
# --------------------------------------------------------------------------
class ConvRec:
    """One conv / transposed conv / linear-as-conv weight in the flat store."""
    __slots__ = ("mod", "transposed", "cout", "cin", "taps", "w_off", "fwd_off", "bwd_off", "tco", "tco_off", "plane0_bwd")


class FusedRec:
    """Two ConvNd of one geometry reading the same input (a ResidualUnit's first conv and its strided
    residual conv), packed as ONE conv over their concatenated output channels: forward weights
    [CoutA + CoutB][tap][Cin] and the concatenated biases, both in the packed buffer."""
    __slots__ = ("a", "b", "w_off", "b_off", "cout", "cin", "taps")


class ParamStore:
    """All parameters of a network as views of ONE flat fp32 buffer (+ a flat
    gradient buffer the kernels accumulate into, the buffer RCCL all-reduces and
    the fused Adam steps over) and the packed [Cout][tap][Cin] conv weights."""

    def __init__(self, module: nn.Module):
        self.module = module
        self.convs: List[ConvRec] = []
        self.fused: List[FusedRec] = []
        self._by_mod = {}
        self.flat = None
        self.flat_grad = None
        self.packed = None
        self.table = None
        self.version = 0
        self.frozen = False
        self._touched = 0
        self._pack_state = {}
        self.flatten()
        for m in module.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv3d, nn.ConvTranspose2d, nn.ConvTranspose3d)):
                tr = isinstance(m, (nn.ConvTranspose2d, nn.ConvTranspose3d))
                self.register_conv(m, cout=m.out_channels, cin=m.in_channels, taps=math.prod(m.kernel_size), transposed=tr)

    def flatten(self):
        params = list(self.module.parameters())
        dev = params[0].device
        offs, total = [], 0
        for p in params:
            total = (total + 3) // 4 * 4  # keep every tensor 16-byte aligned
            offs.append(total)
            total += p.numel()
        total = (total + 3) // 4 * 4
        flat = torch.zeros(total, dtype=torch.float32, device=dev)
        grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self._off = {}
        with torch.no_grad():
            for p, o in zip(params, offs):
                flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
                p.data = flat[o:o + p.numel()].view(p.shape)
                p.grad = grad[o:o + p.numel()].view(p.shape)
                self._off[id(p)] = o
        self.flat, self.flat_grad = flat, grad
        self._params = params
        self.version += 1
        self._build_pack_table()

    def attach_grads(self):
        """Re-point .grad at the flat gradient views (an optimizer's
        zero_grad(set_to_none=True) detaches them)."""
        lost = [p for p in self._params
                if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * self._off[id(p)]]
        if not lost:
            return
        # A gradient that was set to None (torch.optim's zero_grad default) counts as zeroed: the kernels ACCUMULATE
        # into the flat buffer, so its slice must not keep the previous step's values.
        all_none = len(lost) == len(self._params) and all(p.grad is None for p in lost)
        if all_none:
            self.flat_grad.zero_()
        for p in lost:
            o = self._off[id(p)]
            view = self.flat_grad[o:o + p.numel()].view(p.shape)
            if p.grad is None:
                if not all_none:
                    view.zero_()
            else:
                view.copy_(p.grad)                 # a foreign gradient tensor: adopt its values
            p.grad = view

    def offset(self, p) -> int:
        return self._off[id(p)]

    def grad_view(self, p) -> Optional[torch.Tensor]:
        if p is None:                            # e.g. the gamma / beta of a non-affine instance norm
            return None
        o = self._off[id(p)]
        return self.flat_grad[o:o + p.numel()].view(p.shape)

    def register_conv(self, mod, *, cout, cin, taps, transposed=False, tco=False):
        """Register a weight for packing.  All weights must be registered before
        the first plan is built (packed offsets are baked into the programs)."""
        if id(mod) in self._by_mod:
            r = self._by_mod[id(mod)]
            assert (r.cout, r.cin, r.taps, r.transposed) == (cout, cin, taps, transposed)
            return r
        if self.frozen:
            raise RuntimeError("ParamStore: conv registered after plans were built")
        r = ConvRec()
        r.mod, r.transposed, r.cout, r.cin, r.taps = mod, transposed, cout, cin, taps
        r.tco, r.tco_off, r.plane0_bwd = tco, -1, False
        self.convs.append(r)
        self._by_mod[id(mod)] = r
        if self.flat is not None:
            self._build_pack_table()
        return r

    def pack_plane0_bwd(self, mod):
        """The backward-data pack of this registered ConvNd holds input channel 0 alone, [tap][cout] (layout 3 of
        mpgan_pack_weights): the conditional discriminator's first conv, whose second input plane is data."""
        r = self._by_mod[id(mod)]
        if r.plane0_bwd:
            return r
        if self.frozen:
            raise RuntimeError("ParamStore: pack layout changed after plans were built")
        assert not r.transposed
        r.plane0_bwd = True
        self._build_pack_table()
        return r

    def register_fused(self, conv_a, conv_b) -> FusedRec:
        """The concatenated forward pack of two registered ConvNd with equal input channels and kernel."""
        for f in self.fused:
            if f.a.mod is conv_a and f.b.mod is conv_b:
                return f
        if self.frozen:
            raise RuntimeError("ParamStore: fused pair registered after plans were built")
        ra, rb = self._by_mod[id(conv_a)], self._by_mod[id(conv_b)]
        assert (ra.cin, ra.taps, ra.transposed, rb.transposed) == (rb.cin, rb.taps, False, False)
        assert conv_a.bias is not None and conv_b.bias is not None
        f = FusedRec()
        f.a, f.b, f.cout, f.cin, f.taps = ra, rb, ra.cout + rb.cout, ra.cin, ra.taps
        self.fused.append(f)
        self._build_pack_table()
        return f

    def wp_fused(self, f: FusedRec) -> torch.Tensor:
        return self.packed[f.w_off:f.w_off + f.cout * f.cin * f.taps]

    def bias_fused(self, f: FusedRec) -> torch.Tensor:
        return self.packed[f.b_off:f.b_off + f.cout]

    def _build_pack_table(self):
        if not self.convs:
            return
        rows, off = [], 0
        for r in self.convs:
            n = r.cout * r.cin * r.taps
            assert r.mod.weight.numel() == n, (r.mod, n)
            r.w_off = self.offset(r.mod.weight)
            r.fwd_off = off
            off += (n + 3) // 4 * 4
            r.bwd_off = off
            off += (n + 3) // 4 * 4
            rows.append([r.w_off, r.fwd_off, r.cout, r.cin, r.taps, int(r.transposed), 0, 0])
            rows.append([r.w_off, r.bwd_off, r.cout, r.cin, r.taps, int(r.transposed), 3 if r.plane0_bwd else 1, 0])
            if r.tco:
                r.tco_off = off
                off += (n + 3) // 4 * 4
                rows.append([r.w_off, r.tco_off, r.cout, r.cin, r.taps, int(r.transposed), 2, 0])
        for f in self.fused:
            na, nb_ = f.a.cout * f.cin * f.taps, f.b.cout * f.cin * f.taps
            f.w_off = off
            rows.append([f.a.w_off, off, f.a.cout, f.cin, f.taps, 0, 0, 0])
            rows.append([f.b.w_off, off + na, f.b.cout, f.cin, f.taps, 0, 0, 0])
            off += (na + nb_ + 3) // 4 * 4
            f.b_off = off                      # biases: a "conv" with one tap and one input channel copies them
            rows.append([self.offset(f.a.mod.bias), off, f.a.cout, 1, 1, 0, 0, 0])
            rows.append([self.offset(f.b.mod.bias), off + f.a.cout, f.b.cout, 1, 1, 0, 0, 0])
            off += (f.cout + 3) // 4 * 4
        dev = self.flat.device
        self.packed = torch.empty(off, dtype=torch.float32, device=dev)
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self._max_elems = max(r.cout * r.cin * r.taps for r in self.convs)
        self._pack_state.clear()               # a new packed buffer holds nothing yet

    def emit_pack(self, prog: Program):
        """The repack launch, skipped while the parameters are known to be unchanged since the last pack.
        Every Parameter keeps its OWN version counter (`p.data = flat[...]` aliases the storage, not the counter),
        so the key holds the counters of all packed parameters -- `load_state_dict`, `nn.init.*`, `weight.mul_()`
        and a stock `torch.optim.Adam` bump those -- next to the flat buffer's counter (writes through `store.flat`)
        and `touch()` (the fused Adam writes through a raw pointer).  Back-to-back forwards on constant weights
        (inference, the discriminator's real/fake pair of one step) then pack once."""
        self.frozen = True
        fn = lib().mpgan_pack_weights
        args = (self.flat.data_ptr(), self.packed.data_ptr(), self.table.data_ptr(), self.table.shape[0], self._max_elems)
        state = self._pack_state
        packed_params = [r.mod.weight for r in self.convs]
        for f in self.fused:
            packed_params += [f.a.mod.bias, f.b.mod.bias]

        def pack_if_stale(stream):
            key = (self.flat._version, self.version, self._touched, sum(p._version for p in packed_params))
            if state.get("key") == key and not _ALWAYS_PACK:
                return 0
            rc = fn(*args, stream)
            if rc == 0:
                state["key"] = key
            return rc

        prog.add("pack_weights", pack_if_stale, keep=(self.flat, self.packed, self.table))

    def touch(self):
        """Parameters were written behind torch's back (raw-pointer kernel)."""
        self._touched += 1

    def wp(self, rec: ConvRec) -> torch.Tensor:
        return self.packed[rec.fwd_off:rec.fwd_off + rec.cout * rec.cin * rec.taps]

    def wp_bwd(self, rec: ConvRec) -> torch.Tensor:
        return self.packed[rec.bwd_off:rec.bwd_off + rec.cout * rec.cin * rec.taps]

    def wp_tco(self, rec: ConvRec) -> torch.Tensor:
        return self.packed[rec.tco_off:rec.tco_off + rec.cout * rec.cin * rec.taps]


# --------------------------------------------------------------------------
# emit helpers
# --------------------------------------------------------------------------
class NormBuf:
    """Device vectors of one norm layer in one plan."""

    def __init__(self, n, c, instance, dev):
        m = n * c if instance else c
        mm = (m + 3) // 4 * 4
        buf = torch.zeros(6, mm, device=dev)
        self.scale, self.shift, self.mean, self.invstd, self.c1, self.c2 = (buf[i, :m] for i in range(6))
        self.n, self.c, self.instance = n, c, instance
        # accumulator statistics (csrc/norm_fold.h): set by the plan for layers whose producer and first consumer
        # both support it; `folded` flips when the first consumer has been emitted
        self.acc = None            # int64 view [replicas][4][cstride]
        self.acc_cstride = 0
        self.acc_count = 0
        self.norm_mod = None
        self.folded = False

    def fold(self):
        """The mpgan_norm_fold the FIRST consumer of these statistics passes; None once they are published."""
        if self.acc is None or self.folded:
            return None
        self.folded = True
        return ops.make_fold(self.acc, ops.ACC_REPLICAS, self.acc_cstride, self.acc_count, self.norm_mod, self.scale,
                             self.shift, self.mean, self.invstd)

    def prologue(self, act, slope=1.0, slope_t=None) -> Prologue:
        return Prologue(self.scale, self.shift, self.c if self.instance else 0, act, slope, slope_t)


def _fast_leaky(pro) -> bool:
    """launch_pipe_pro's rule for the max(y, slope*y) form: per-channel norm + LeakyReLU whose slope the
    host knows (no device PReLU weight) to lie in [0, 1]."""
    return bool(pro is not None and not pro.n_stride and pro.act == ACT_LEAKY and pro.slope_t is None
                and 0.0 <= pro.slope <= 1.0)


def _gdesc(g: ConvGeom) -> str:
    return (f"{g.cin}->{g.cout} k{'x'.join(map(str, g.k))} s{g.stride[-1]}{'T' if g.transposed else ''} "
            f"in{'x'.join(map(str, g.in_dhw))}")


def emit_conv_fwd(prog, g: ConvGeom, x, wp, bias, y, pro=None, resid=None, tanh=False, stats=None, lane=0, fold=None,
                  stats_acc=None):
    """fold: mpgan_norm_fold of the producer of x (its statistics are finalised by this launch);
    stats_acc: int64 accumulators that receive this conv's own statistics instead of partial rows."""
    ops._check_in_out(g, x, y, "plan conv_forward")
    gc = g.c()
    pc = pro.c() if pro is not None else None
    tag = (gather_kernel_name(g, False, pro is not None, bool(pro is not None and pro.n_stride), _fast_leaky(pro)),
           2.0 * conv_macs(g), conv_bytes(g))
    if fold is None and stats_acc is None:
        prog.add("conv_forward", lib().mpgan_conv_forward, C.byref(gc), x.data_ptr(), _ld(x), wp.data_ptr(), _p(bias),
                 C.byref(pc) if pc is not None else None, _p(resid), _ld(resid), int(tanh), _p(stats), y.data_ptr(),
                 _ld(y), keep=(gc, pc, x, wp, bias, y, resid, pro), desc=_gdesc(g), tag=tag, lane=lane)
        return
    assert stats is None or stats_acc is None
    prog.add("conv_forward_fold", lib().mpgan_conv_forward_fold, C.byref(gc), x.data_ptr(), _ld(x), wp.data_ptr(),
             _p(bias), C.byref(pc) if pc is not None else None, C.byref(fold) if fold is not None else None, _p(resid),
             _ld(resid), int(tanh), _p(stats), _p(stats_acc), ops.ACC_REPLICAS if stats_acc is not None else 0,
             y.data_ptr(), _ld(y), keep=(gc, pc, fold, x, wp, bias, y, resid, pro, stats_acc), desc=_gdesc(g), tag=tag,
             lane=lane)


def emit_conv_dgrad(prog, g: ConvGeom, dy, wp_bwd, dx, resid=None):
    ops._check_in_out(g, dx, dy, "plan conv_backward_data")
    gc = g.c()
    prog.add("conv_backward_data", lib().mpgan_conv_backward_data, C.byref(gc), dy.data_ptr(), _ld(dy),
             wp_bwd.data_ptr(), _p(resid), _ld(resid), dx.data_ptr(), _ld(dx), keep=(gc, dy, wp_bwd, dx, resid),
             desc=_gdesc(g), tag=("dgrad:" + gather_kernel_name(g, True, False), 2.0 * conv_macs(g), conv_bytes(g)))


_FUSE_BWD_STATS = not os.environ.get("MPGAN_DBG_NO_FUSE_BWD_STATS")
# The bf16 path's counterpart (mpgan_conv_backward_data_stats_bf16) is OFF by default: measured at config C5 on one box
# (tools/phase_times.py, round 4), D's backward passes take 57.9 ms per step with the sums fused into the backward-data
# epilogues and 57.2 ms with the separate norm_bwd_reduce_bf16 launches -- the bf16 kernels run one block per CU, so the
# epilogue's extra 16-byte z loads are exposed, while the separate pass streams g and z with the whole chip at the HBM rate.
_FUSE_BWD_STATS_BF16 = bool(os.environ.get("MPGAN_FUSE_BWD_STATS_BF16"))


def emit_conv_dgrad_stats(prog, g: ConvGeom, dy, wp_bwd, dx, z, nb: "NormBuf", slope: float, partials) -> int:
    """Backward-data whose epilogue also leaves the norm-backward partial sums of dx against z (the raw output of
    the layer in front, BatchNorm + LeakyReLU(slope)): returns the number of rows, 0 when this geometry has no
    fused sums (then the plain launch is emitted and the caller runs the reduce pass)."""
    rows = ops.conv_bwd_stats_rows(g) if _FUSE_BWD_STATS and not nb.instance else 0
    if not rows or partials.numel() < rows * 3 * g.cin:
        emit_conv_dgrad(prog, g, dy, wp_bwd, dx)
        return 0
    ops._check_in_out(g, dx, dy, "plan conv_backward_data_stats")
    gc = g.c()
    prog.add("conv_backward_data", lib().mpgan_conv_backward_data_stats, C.byref(gc), dy.data_ptr(), _ld(dy),
             wp_bwd.data_ptr(), dx.data_ptr(), _ld(dx), z.data_ptr(), _ld(z), nb.scale.data_ptr(), nb.shift.data_ptr(),
             nb.mean.data_ptr(), nb.invstd.data_ptr(), ACT_LEAKY, float(slope), partials.data_ptr(),
             keep=(gc, dy, wp_bwd, dx, z, nb, partials), desc=_gdesc(g),
             tag=("dgrad:" + gather_kernel_name(g, True, False), 2.0 * conv_macs(g), conv_bytes(g)))
    return rows


def emit_conv_wgrad(prog, g: ConvGeom, x, dy, dw, ws, pro=None, dbias=None, lane=0):
    """dW += wgrad; for a ConvNd, dbias += colsum(dy) rides along in the same kernel."""
    ops._check_in_out(g, x, dy, "plan conv_backward_weight")
    gc = g.c()
    pc = pro.c() if pro is not None else None
    need = ops.conv_wgrad_workspace(g)
    assert ws.numel() * 4 >= need, "wgrad workspace too small"
    prog.add("conv_backward_weight", lib().mpgan_conv_backward_weight, C.byref(gc), x.data_ptr(), _ld(x),
             C.byref(pc) if pc is not None else None, dy.data_ptr(), _ld(dy), dw.data_ptr(), _p(dbias), 1.0,
             ws.data_ptr(), ws.numel() * 4, keep=(gc, pc, x, dy, dw, dbias, ws, pro), desc=_gdesc(g),
             tag=(wgrad_kernel_name(g, pro), 2.0 * conv_macs(g), conv_bytes(g)), lane=lane)


def emit_bias_grad(prog, dy, db, partials):
    """db += column sums of dy (two-stage, deterministic)."""
    n, P, ld = ops._cl(dy, "bias grad")
    c = dy.shape[-1]
    chunks = ops.stats_chunks(P, c)
    assert partials.numel() >= n * chunks * 2 * c
    L = lib()
    prog.add("channel_stats", L.mpgan_channel_stats, dy.data_ptr(), ld, n, P, c, partials.data_ptr(),
             keep=(dy, partials))
    prog.add("reduce_partials", L.mpgan_reduce_partials, partials.data_ptr(), n * chunks, 2 * c, c, db.data_ptr(), 1.0,
             keep=(db,))


def emit_norm_stats(prog, z, nb: NormBuf, norm_mod, partials, eps=1e-5, momentum=0.1):
    """channel_stats + finalize: scale/shift for the consumer's prologue; running
    stats updated in place (BatchNorm, train mode)."""
    n, P, ld = ops._cl(z, "norm stats")
    c = z.shape[-1]
    chunks = ops.stats_chunks(P, c)
    assert partials.numel() >= n * chunks * 2 * c
    L = lib()
    rm = getattr(norm_mod, "running_mean", None)
    rv = getattr(norm_mod, "running_var", None)
    nbt = getattr(norm_mod, "num_batches_tracked", None)
    eps = getattr(norm_mod, "eps", eps)
    momentum = getattr(norm_mod, "momentum", momentum)
    if nb.instance:
        rm = rv = nbt = None
    prog.add("channel_stats", L.mpgan_channel_stats, z.data_ptr(), ld, n, P, c, partials.data_ptr(),
             keep=(z, partials))
    prog.add("norm_finalize", L.mpgan_norm_finalize, partials.data_ptr(), n, chunks, c, P, int(nb.instance),
             _p(norm_mod.weight), _p(norm_mod.bias), float(eps), float(momentum), _p(rm), _p(rv), _p(nbt),
             nb.scale.data_ptr(), nb.shift.data_ptr(), nb.mean.data_ptr(), nb.invstd.data_ptr(),
             keep=(norm_mod.weight, norm_mod.bias, rm, rv, nbt, nb))


def emit_conv_fwd_norm(prog, g: ConvGeom, x, wp, bias, y, nb: NormBuf, norm_mod, partials, pro=None, training=True,
                       eval_norms=None, c_norm=None, fold=None):
    """Conv whose raw output feeds a norm layer: BatchNorm statistics come out of the
    conv's own epilogue (one finalize launch follows); so do InstanceNorm's when the partial rows
    fall into per-sample groups; otherwise a separate statistics pass runs.  In eval
    mode BatchNorm's scale/shift come from the running statistics instead.
    c_norm: the norm covers only the first c_norm output channels (a conv fused with its
    ResidualUnit's residual conv: the trailing channels are the un-normalised residual branch)."""
    c = g.cout if c_norm is None else c_norm
    y_norm = y if c_norm is None else y[..., :c]
    if training and nb.acc is not None:
        # accumulator statistics: no finalize launch; the first consumer of `nb` folds them (NormBuf.fold)
        nb.norm_mod = norm_mod
        nb.acc_cstride = g.cout
        n_, P_, _ = ops._cl(y, "conv+norm")
        nb.acc_count = n_ * P_
        emit_conv_fwd(prog, g, x, wp, bias, y, pro=pro, fold=fold, stats_acc=nb.acc)
        return
    if not training and not nb.instance:
        emit_conv_fwd(prog, g, x, wp, bias, y, pro=pro)
        if eval_norms is not None:       # input-independent: the plan folds all of them into one launch up front
            eval_norms.append((norm_mod, nb, c))
            return
        prog.add("norm_from_running", lib().mpgan_norm_from_running, _p(norm_mod.weight), _p(norm_mod.bias),
                 norm_mod.running_mean.data_ptr(), norm_mod.running_var.data_ptr(), float(norm_mod.eps), c,
                 nb.scale.data_ptr(), nb.shift.data_ptr(), nb.mean.data_ptr(), nb.invstd.data_ptr(),
                 keep=(norm_mod.weight, norm_mod.bias, norm_mod.running_mean, norm_mod.running_var, nb))
        return
    code = 0 if pro is None else (2 if pro.n_stride else 1)
    rows = ops.conv_stats_rows(g, code)
    n, P, _ = ops._cl(y, "conv+norm")
    if nb.instance and rows:
        # InstanceNorm needs the partial rows grouped by sample: true for the patch kernel (sample is the
        # slowest block index), for 128-pixel tiles of a non-transposed conv when 128 | P, and for the
        # thin kernel's 256-pixel blocks when 256 | P
        v = ops.conv_variant(g, False, code)
        v = v - 3000 if v >= 3000 else v
        v = v - 2000 if v >= 2000 else v
        grouped = (v in (16, 17) or (v == 1 and P % 256 == 0)
                   or (v in (32, 64, 128) and not g.transposed and P % 128 == 0))
        if not grouped or rows % n:
            rows = 0
    if rows == 0:
        emit_conv_fwd(prog, g, x, wp, bias, y, pro=pro, fold=fold)
        emit_norm_stats(prog, y_norm, nb, norm_mod, partials)
        return
    W = g.cout                                  # partial rows are [2][W] wide
    assert partials.numel() >= (rows + 32) * 2 * W
    emit_conv_fwd(prog, g, x, wp, bias, y, pro=pro, stats=partials, fold=fold)
    if nb.instance:
        prog.add("norm_finalize", lib().mpgan_norm_finalize_strided, partials.data_ptr(), n, rows // n, c, W, P, 1,
                 _p(norm_mod.weight), _p(norm_mod.bias), float(norm_mod.eps), 0.0, None, None, None,
                 nb.scale.data_ptr(), nb.shift.data_ptr(), nb.mean.data_ptr(), nb.invstd.data_ptr(),
                 keep=(norm_mod.weight, norm_mod.bias, nb, partials))
        return
    rm = getattr(norm_mod, "running_mean", None)
    rv = getattr(norm_mod, "running_var", None)
    nbt = getattr(norm_mod, "num_batches_tracked", None)
    prog.add("norm_finalize", lib().mpgan_norm_finalize_strided, partials.data_ptr(), 1, rows, c, W, n * P, 0,
             _p(norm_mod.weight), _p(norm_mod.bias), float(norm_mod.eps), float(norm_mod.momentum), _p(rm), _p(rv),
             _p(nbt), nb.scale.data_ptr(), nb.shift.data_ptr(), nb.mean.data_ptr(), nb.invstd.data_ptr(),
             keep=(norm_mod.weight, norm_mod.bias, rm, rv, nbt, nb, partials), desc=f"C{c} rows{rows}")


def _f32_bits(v: float) -> int:
    """The bit pattern of a float32, as the int64 tables of the `_multi` launches carry one."""
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def emit_eval_norms(prog, eval_norms, dev):
    """One launch computing scale/shift of every eval-mode BatchNorm layer of a plan (they depend on
    parameters and running statistics only, not on the input)."""
    if not eval_norms:
        return
    rows = []
    for norm_mod, nb, c in eval_norms:
        rows.append([_p(norm_mod.weight) or 0, _p(norm_mod.bias) or 0, norm_mod.running_mean.data_ptr(),
                     norm_mod.running_var.data_ptr(), nb.scale.data_ptr(), nb.shift.data_ptr(), nb.mean.data_ptr(),
                     nb.invstd.data_ptr(), c, _f32_bits(norm_mod.eps)])
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    prog.add("norm_from_running_multi", lib().mpgan_norm_from_running_multi, table.data_ptr(), len(rows),
             keep=(table, eval_norms))


def emit_conv_fwd_act(prog, rows, g: ConvGeom, x, wp, bias, y, norm_mod=None, act_mod=None, c_norm=None, resid=None,
                      tanh=False):
    """Eval-mode inference conv (code/GAN/inferrence.py:97-110,169-170): running-statistics BatchNorm, PReLU, the conv's
    bias and the residual add all in the conv's epilogue (mpgan_conv_forward_act); `rows` collects the plan's table rows
    for the one up-front mpgan_epi_vectors_multi launch that fills this conv's scale / shift / slope vectors.
    c_norm: the norm + activation cover only the first c_norm output channels (a conv fused with its unit's residual conv)."""
    ops._check_in_out(g, x, y, "plan conv_forward_act")
    if act_mod is not None:
        assert act_mod.weight.numel() == 1, "eval plan: PReLU with one parameter (MONAI 0.4.0's default)"
    vec = epi_row(rows, g.cout, bias, norm_mod, act_mod, x.device, c_norm=c_norm)
    gc = g.c()
    tag = (gather_kernel_name(g, False, False), 2.0 * conv_macs(g), conv_bytes(g))
    prog.add("conv_forward", lib().mpgan_conv_forward_act, C.byref(gc), x.data_ptr(), _ld(x), wp.data_ptr(),
             vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), _p(resid), _ld(resid), int(tanh), y.data_ptr(), _ld(y),
             keep=(gc, x, wp, bias, y, resid, vec, norm_mod, act_mod), desc=_gdesc(g), tag=tag)


def emit_epi_vectors(prog, rows, dev):
    """One launch filling the epilogue-activation vectors of every conv of an eval-mode plan (they depend on parameters
    and running statistics only, not on the input)."""
    if not rows:
        return
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    prog.add("epi_vectors_multi", lib().mpgan_epi_vectors_multi, table.data_ptr(), len(rows), keep=(table,))


class _ConstSlope:
    """A LeakyReLU's slope as emit_conv_fwd_act / mpgan_epi_vectors_multi take an activation: a one-element device
    tensor in the PReLU column of the table."""

    def __init__(self, slope: float, dev):
        self.weight = torch.full((1,), float(slope), device=dev)


def epi_row(rows, cout, bias, norm_mod, act_mod, dev, c_norm=None):
    """Table row of mpgan_epi_vectors_multi for one eval-mode conv with `cout` output channels: running-statistics
    BatchNorm over the first c_norm of them (default: all; none without a norm_mod), then the activation (none without
    an act_mod).  Returns the (3, cpad) tensor whose rows the launch fills with scale / shift / slope (each 16-byte
    aligned)."""
    nm = norm_mod
    if nm is not None:
        assert getattr(nm, "running_mean", None) is not None, "eval plan: BatchNorm layers with running statistics only"
    c = 0 if nm is None else (cout if c_norm is None else c_norm)
    vec = torch.empty(3, (cout + 3) // 4 * 4, device=dev)
    rows.append([(_p(nm.weight) or 0) if nm is not None else 0, (_p(nm.bias) or 0) if nm is not None else 0,
                 nm.running_mean.data_ptr() if nm is not None else 0, nm.running_var.data_ptr() if nm is not None else 0,
                 _p(bias) or 0, _p(act_mod.weight) if act_mod is not None else 0, vec[0].data_ptr(), vec[1].data_ptr(),
                 vec[2].data_ptr(), c, cout, _f32_bits(nm.eps if nm is not None else 0.0)])
    return vec


def emit_conv_fwd_act_bf16(prog, rows, g: ConvGeom, x, wp, bias, y, norm_mod, act_mod):
    """Eval-mode conv of the bf16-storage discriminators: running-statistics BatchNorm + LeakyReLU in the epilogue of the
    bf16 forward (mpgan_conv_forward_act_bf16; mpgan_conv_forward_act_f32_to_bf16 for the 1-input-channel layer), the
    activated tensor stored once -- bf16, or fp32 when `y` is (the layer the fp32 head reads)."""
    vec = epi_row(rows, g.cout, bias, norm_mod, act_mod, x.device)
    gc = g.c()
    if g.cin == 1:
        prog.add("conv_forward_act_f32_to_bf16", lib().mpgan_conv_forward_act_f32_to_bf16, C.byref(gc), x.data_ptr(), 1,
                 wp.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), None, y.data_ptr(), g.cout,
                 keep=(gc, x, wp, y, vec, norm_mod, act_mod, bias), desc=_gdesc(g),
                 tag=_thin_cin1_tag(g, x))
        return
    prog.add("conv_forward_act_bf16", lib().mpgan_conv_forward_act_bf16, C.byref(gc), x.data_ptr(), g.cin, wp.data_ptr(),
             vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), None, y.data_ptr(), g.cout,
             int(y.dtype == torch.float32), keep=(gc, x, wp, y, vec, norm_mod, act_mod, bias), desc=_gdesc(g),
             tag=(_bf16_kernel_name(g, False), 2.0 * conv_macs(g), conv_bytes(g, 2)))


def emit_norm_act_add(prog, z, pz, r, pr, out, tanh=False, fold=None):
    """fold: mpgan_norm_fold of z's producer (this launch finalises its statistics)."""
    n, P, ldz = ops._cl(z, "norm_act_add z")
    assert out.shape == z.shape and (r is None or r.shape == z.shape)
    pzc = pz.c() if pz is not None else None
    prc = pr.c() if pr is not None else None
    if fold is None:
        prog.add("norm_act_add", lib().mpgan_norm_act_add, z.data_ptr(), ldz, C.byref(pzc) if pzc else None, _p(r),
                 _ld(r), C.byref(prc) if prc else None, n, P, z.shape[-1], int(tanh), out.data_ptr(), _ld(out),
                 keep=(z, pzc, pz, r, prc, pr, out), desc=f"C{z.shape[-1]} n{n} P{P}")
        return
    prog.add("norm_act_add_fold", lib().mpgan_norm_act_add_fold, z.data_ptr(), ldz, C.byref(pzc), C.byref(fold), _p(r),
             _ld(r), C.byref(prc) if prc else None, n, P, z.shape[-1], int(tanh), out.data_ptr(), _ld(out),
             keep=(z, pzc, pz, fold, r, prc, pr, out))


def emit_norm_bwd(prog, g, z, nb: NormBuf, pro: Prologue, dz, partials, dgamma, dbeta, dslope, peer=None, reduced_rows=0):
    """reduce -> finalize -> apply.  dgamma/dbeta/dslope are gradient views
    (accumulated into) or None when the owner's parameters are frozen.
    reduced_rows > 0: `partials` already holds that many [3][C] rows, left by the backward-data launch that
    produced g (emit_conv_dgrad_stats) -- no reduce pass."""
    n, P, ldz = ops._cl(z, "norm_bwd z")
    assert g.shape == z.shape and dz.shape == z.shape
    c = z.shape[-1]
    chunks = ops.stats_chunks(P, c)
    assert partials.numel() >= n * chunks * (3 * c + 1)              # [3][C] rows + one slope scalar per row (ops.norm_bwd_reduce)
    L = lib()
    pc = pro.c()
    pe = peer.c() if peer is not None else None
    pe_ref = C.byref(pe) if pe is not None else None
    if reduced_rows:
        assert peer is None and not nb.instance and partials.numel() >= reduced_rows * 3 * c
        # rows left by mpgan_conv_backward_data_stats carry no per-row slope scalars (include/mpgan_hip.h): a learnable
        # PReLU slope needs the stand-alone reduce pass
        assert dslope is None, "fused norm-backward rows cannot feed a slope gradient"
        prog.add("norm_bwd_finalize", L.mpgan_norm_bwd_finalize, partials.data_ptr(), 1, reduced_rows, c, n * P, 0,
                 _p(dgamma), _p(dbeta), _p(dslope), nb.c1.data_ptr(), nb.c2.data_ptr(), keep=(dgamma, dbeta, dslope))
        prog.add("norm_bwd_apply", L.mpgan_norm_bwd_apply, g.data_ptr(), _ld(g), z.data_ptr(), ldz, C.byref(pc),
                 nb.mean.data_ptr(), nb.invstd.data_ptr(), nb.c1.data_ptr(), nb.c2.data_ptr(), pe_ref, n, P, c,
                 dz.data_ptr(), _ld(dz), keep=(dz, g, z, pc, pro, nb, partials), desc=f"C{c} n{n} P{P}")
        return
    prog.add("norm_bwd_reduce", L.mpgan_norm_bwd_reduce, g.data_ptr(), _ld(g), z.data_ptr(), ldz, C.byref(pc),
             nb.mean.data_ptr(), nb.invstd.data_ptr(), pe_ref, n, P, c, partials.data_ptr(),
             keep=(g, z, pc, pro, nb, partials, pe, peer), desc=f"C{c} n{n} P{P}")
    prog.add("norm_bwd_finalize", L.mpgan_norm_bwd_finalize, partials.data_ptr(), n, chunks, c, P, int(nb.instance),
             _p(dgamma), _p(dbeta), _p(dslope), nb.c1.data_ptr(), nb.c2.data_ptr(), keep=(dgamma, dbeta, dslope),
             desc=f"C{c} rows{n * chunks}")
    prog.add("norm_bwd_apply", L.mpgan_norm_bwd_apply, g.data_ptr(), _ld(g), z.data_ptr(), ldz, C.byref(pc),
             nb.mean.data_ptr(), nb.invstd.data_ptr(), nb.c1.data_ptr(), nb.c2.data_ptr(), pe_ref, n, P, c,
             dz.data_ptr(), _ld(dz), keep=(dz,), desc=f"C{c} n{n} P{P}")


# ---- bf16 storage: the single description of a bf16 layer's launches, for both discriminators ----
def _bf16_kernel_name(g: ConvGeom, backward_data: bool) -> str:
    """rocprofv3's name of the bf16 kernel that serves this layer (labels of bench.py's probe), from the same choice
    the launch makes (mpgan_conv_kernel_name_bf16; the forward is the one with statistics)."""
    gc = g.c()
    return kernel_label(lib().mpgan_conv_kernel_name_bf16, C.byref(gc), int(backward_data))


def _bf16_wgrad_kernel_name(g: ConvGeom) -> str:
    """rocprofv3's name of the bf16 weight-gradient kernel of this layer, asked of the library that makes the choice."""
    gc = g.c()
    return "wgrad_bf16_wide_kernel" if lib().mpgan_conv_wgrad_variant_bf16(C.byref(gc)) == 1 else "wgrad_bf16_kernel<8>"


def _thin_cin1_tag(g: ConvGeom, x):
    """Probe tag of the 1-input-channel layer's forward (fp32 image in, bf16 out)."""
    return ("thin_cin1_full_kernel<16, true>", 2.0 * conv_macs(g), conv_bytes(g, 2) + 2 * x.numel())


def _rows(g: ConvGeom) -> int:
    """Rows (pixels of all samples) of a conv's channels-last output."""
    return g.n * math.prod(g.out_dhw)


class PacksBF16:
    """bf16 packs of a plan's dense convs, from their ConvRecs: [Cout][tap][Cin] (forward) and [Cin][tap][Cout]
    (backward-data) in one buffer, each pack 16-byte aligned, refreshed from the flat fp32 store by one launch."""

    def __init__(self, recs, dev):
        rows, off, self._at = [], 0, {}
        for r in recs:
            nel = r.cout * r.cin * r.taps
            pad = (nel + 7) // 8 * 8
            self._at[id(r)] = (off, off + pad, nel)
            rows.append([r.w_off, off, r.cout, r.cin, r.taps, 0, 0, 0])
            rows.append([r.w_off, off + pad, r.cout, r.cin, r.taps, 0, 1, 0])
            off += 2 * pad
        self.packed = torch.empty(off, device=dev, dtype=torch.bfloat16)
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.max_elems = max(r.cout * r.cin * r.taps for r in recs)

    def emit(self, prog, store: ParamStore):
        prog.add("pack_weights_bf16", lib().mpgan_pack_weights_bf16, store.flat.data_ptr(), self.packed.data_ptr(),
                 self.table.data_ptr(), self.table.shape[0], self.max_elems, keep=(self.packed, self.table))

    def fwd(self, rec: ConvRec) -> torch.Tensor:
        o, _, nel = self._at[id(rec)]
        return self.packed[o:o + nel]

    def bwd(self, rec: ConvRec) -> torch.Tensor:
        _, o, nel = self._at[id(rec)]
        return self.packed[o:o + nel]


def emit_conv_fwd_bf16(prog, g: ConvGeom, x, wp, bias, z, stats=None) -> int:
    """Raw conv output z (bf16) with the fp32 BatchNorm statistics out of the epilogue (`stats`: the partials, None
    for none); the 1-input-channel layer reads the fp32 image and fp32 weights.  Returns the statistics rows written."""
    gc = g.c()
    thin = g.cin == 1
    name = "conv_forward_f32_to_bf16" if thin else "conv_forward_bf16"
    prog.add(name, getattr(lib(), "mpgan_" + name), C.byref(gc), x.data_ptr(), g.cin, wp.data_ptr(), bias.data_ptr(),
             _p(stats), z.data_ptr(), g.cout, keep=(gc, x, wp, bias, z, stats), desc=_gdesc(g),
             tag=_thin_cin1_tag(g, x) if thin else (_bf16_kernel_name(g, False), 2.0 * conv_macs(g), conv_bytes(g, 2)))
    return (_rows(g) + 255) // 256 if thin else ops.conv_stats_rows_bf16(g)


def emit_norm_act_bf16(prog, z, nb: NormBuf, slope: float, a, norm_mod=None, partials=None, stat_rows=0):
    """a = LeakyReLU(z*scale + shift), stored once (bf16, or fp32 when `a` is).  norm_mod: first finalize the
    `stat_rows` statistics rows the conv left in `partials` (train mode: running statistics updated); None: scale /
    shift are already there (emit_eval_norms)."""
    rows, c = z.numel() // z.shape[-1], z.shape[-1]
    if norm_mod is not None:
        prog.add("norm_finalize", lib().mpgan_norm_finalize, partials.data_ptr(), 1, stat_rows, c, rows, 0,
                 _p(norm_mod.weight), _p(norm_mod.bias), float(norm_mod.eps), float(norm_mod.momentum),
                 _p(norm_mod.running_mean), _p(norm_mod.running_var), _p(norm_mod.num_batches_tracked),
                 nb.scale.data_ptr(), nb.shift.data_ptr(), nb.mean.data_ptr(), nb.invstd.data_ptr(),
                 keep=(norm_mod, nb, partials))
    prog.add("norm_act_bf16", lib().mpgan_norm_act_bf16, z.data_ptr(), c, nb.scale.data_ptr(), nb.shift.data_ptr(),
             float(slope), rows, c, a.data_ptr(), c, int(a.dtype == torch.float32), keep=(z, nb, a))


def emit_norm_bwd_bf16(prog, g, z, nb: NormBuf, slope: float, dz, partials, dgamma, dbeta, peer=None, reduced_rows=0,
                       bias_part=False):
    """emit_norm_bwd on bf16 z: reduce -> finalize -> apply, dz stored as bf16 (g: bf16 or fp32).
    peer: ops.PeerTapsBF16 of the other pass (the `_peer` entries).  reduced_rows > 0: `partials` already holds that
    many [3][C] rows, left by the backward-data launch that produced g (emit_conv_dgrad_bf16) -- no reduce pass.
    bias_part: apply also leaves per-block column sums of the stored dz (the conv's bias gradient); they sit behind
    the rows finalize reads, and their view of `partials` is returned."""
    rows, c = z.numel() // z.shape[-1], z.shape[-1]
    brow = ops.norm_bwd_rows_bf16(rows, c)
    base = max(brow, reduced_rows) * 3 * c + c
    assert partials.numel() >= base + (brow * c if bias_part else 0)
    bias_part = partials[base:base + brow * c] if bias_part else None
    L = lib()
    g32 = int(g.dtype == torch.float32)
    norm = (nb.scale.data_ptr(), nb.shift.data_ptr(), nb.mean.data_ptr(), nb.invstd.data_ptr())
    pc = peer.c() if peer is not None else None
    pe, sfx = ((C.byref(pc),), "_peer") if peer is not None else ((), "")
    assert peer is None or not reduced_rows
    if not reduced_rows:
        prog.add("norm_bwd_reduce_bf16" + sfx, getattr(L, "mpgan_norm_bwd_reduce_bf16" + sfx), g.data_ptr(), g32, c,
                 z.data_ptr(), c, *norm, *pe, float(slope), rows, c, partials.data_ptr(),
                 keep=(g, z, nb, partials, peer, pc))
    prog.add("norm_bwd_finalize", L.mpgan_norm_bwd_finalize, partials.data_ptr(), 1, reduced_rows or brow, c, rows, 0,
             _p(dgamma), _p(dbeta), None, nb.c1.data_ptr(), nb.c2.data_ptr(), keep=(dgamma, dbeta))
    prog.add("norm_bwd_apply_bf16" + sfx, getattr(L, "mpgan_norm_bwd_apply_bf16" + sfx), g.data_ptr(), g32, c,
             z.data_ptr(), c, *norm, nb.c1.data_ptr(), nb.c2.data_ptr(), *pe, float(slope), rows, c, dz.data_ptr(), c,
             _p(bias_part), keep=(g, z, nb, dz, bias_part, peer, pc))
    return bias_part


def emit_conv_wgrad_bf16(prog, g: ConvGeom, x, dy, dw, dbias, ws, bias_part=None):
    """dW += wgrad on bf16 dy.  Dense layers (bf16 x): dbias += the column sums emit_norm_bwd_bf16 left in `bias_part`;
    the 1-input-channel layer (fp32 x): the bias gradient rides along in the kernel."""
    gc = g.c()
    if g.cin == 1:
        assert ws.numel() * 4 >= ops.conv_wgrad_workspace_bf16dy(g), "wgrad workspace too small"
        prog.add("conv_backward_weight_bf16dy", lib().mpgan_conv_backward_weight_bf16dy, C.byref(gc), x.data_ptr(), 1,
                 dy.data_ptr(), g.cout, dw.data_ptr(), dbias.data_ptr(), 1.0, ws.data_ptr(), ws.numel() * 4,
                 keep=(gc, x, dy, dw, dbias, ws), desc=_gdesc(g),
                 tag=(wgrad_kernel_name(g, bf16_dy=True), 2.0 * conv_macs(g), conv_bytes(g, 2) + 2 * x.numel()))
        return
    assert ws.numel() * 4 >= ops.conv_wgrad_workspace_bf16(g), "wgrad workspace too small"
    prog.add("reduce_partials", lib().mpgan_reduce_partials, bias_part.data_ptr(), bias_part.numel() // g.cout, g.cout,
             g.cout, dbias.data_ptr(), 1.0, keep=(bias_part, dbias))
    prog.add("conv_backward_weight_bf16", lib().mpgan_conv_backward_weight_bf16, C.byref(gc), x.data_ptr(), g.cin,
             dy.data_ptr(), g.cout, dw.data_ptr(), 1.0, ws.data_ptr(), ws.numel() * 4, keep=(gc, x, dy, dw, ws),
             desc=_gdesc(g), tag=(_bf16_wgrad_kernel_name(g), 2.0 * conv_macs(g), conv_bytes(g, 2)))


def bwd_stats_rows_bf16(g: ConvGeom) -> int:
    """Rows of norm-backward sums the fused backward-data form leaves for this geometry (0: it has none)."""
    gc = g.c()
    return max(0, int(lib().mpgan_conv_bwd_stats_rows_bf16(C.byref(gc))))


def emit_conv_dgrad_bf16(prog, g: ConvGeom, dy, wp_bwd, dx, stats=None) -> int:
    """Backward-data on bf16 dy; dx is bf16, or fp32 for the 1-input-channel layer (fp32 weights).
    stats = (z, nb, slope, partials) of the layer in front: where this geometry has the fused form, the epilogue also
    leaves that layer's norm-backward sums of dx against z in `partials` -- returns their number of rows, else 0 (the
    caller runs the reduce pass)."""
    gc = g.c()
    thin = g.cin == 1
    tag = None if thin else ("dgrad:" + _bf16_kernel_name(g, True), 2.0 * conv_macs(g), conv_bytes(g, 2))
    rows = bwd_stats_rows_bf16(g) if stats is not None and not thin else 0
    if not rows:
        name = "conv_backward_data_bf16_to_f32" if thin else "conv_backward_data_bf16"
        prog.add(name, getattr(lib(), "mpgan_" + name), C.byref(gc), dy.data_ptr(), g.cout, wp_bwd.data_ptr(),
                 dx.data_ptr(), g.cin, keep=(gc, dy, wp_bwd, dx), desc=_gdesc(g), tag=tag)
        return 0
    z, nb, slope, partials = stats
    assert partials.numel() >= rows * 3 * g.cin
    prog.add("conv_backward_data_bf16", lib().mpgan_conv_backward_data_stats_bf16, C.byref(gc), dy.data_ptr(), g.cout,
             wp_bwd.data_ptr(), dx.data_ptr(), g.cin, z.data_ptr(), g.cin, nb.scale.data_ptr(), nb.shift.data_ptr(),
             nb.mean.data_ptr(), nb.invstd.data_ptr(), float(slope), partials.data_ptr(),
             keep=(gc, dy, wp_bwd, dx, z, nb, partials), desc=_gdesc(g), tag=tag)
    return rows


# ---- the conditional discriminator's first conv: two 1-channel input planes (image, condition), mpgan_conv2p_* ----
def _conv2p_tag(name: str, g: ConvGeom, dense):
    """Probe tag of a two-plane launch: both fp32 planes read once, the 64-channel tensor read or written once."""
    return (name, 2.0 * conv_macs(g), 4 * g.n * math.prod(g.in_dhw) * 2 + dense.numel() * dense.element_size())


def _check_conv2p(g: ConvGeom, x, cond, dense, what: str):
    if cond is None or tuple(cond.shape) != tuple(x.shape) or tuple(x.shape) != (g.n, *g.in_dhw, 1):
        raise ValueError(f"{what}: the image and the condition must both be {(g.n, *g.in_dhw, 1)}")
    if tuple(dense.shape) != (g.n, *g.out_dhw, g.cout):
        raise ValueError(f"{what}: output shape {tuple(dense.shape)} != {(g.n, *g.out_dhw, g.cout)}")


def emit_conv2p_fwd(prog, g: ConvGeom, x, cond, wp, bias, z, stats=None) -> int:
    """Raw output z (fp32 or bf16, as `z` is) of the two-plane conv; `stats`: the partials that receive the fused
    statistics rows (bf16 z only).  Returns the rows written (0: none, run a statistics pass)."""
    _check_conv2p(g, x, cond, z, "plan conv2p_forward")
    bf = z.dtype == torch.bfloat16
    rows = ops.conv2p_stats_rows(g, bf) if stats is not None else 0
    name = "conv2p_forward_f32_to_bf16" if bf else "conv2p_forward"
    gc = g.c()
    prog.add(name, getattr(lib(), "mpgan_" + name), C.byref(gc), x.data_ptr(), cond.data_ptr(), wp.data_ptr(),
             bias.data_ptr(), _p(stats) if rows else None, z.data_ptr(), g.cout, keep=(gc, x, cond, wp, bias, z, stats),
             desc=_gdesc(g), tag=_conv2p_tag(ops.conv2p_kernel_name(g, bf), g, z))
    return rows


def emit_conv2p_fwd_act(prog, rows, g: ConvGeom, x, cond, wp, bias, y, norm_mod, act_mod):
    """Eval mode: running-statistics BatchNorm + LeakyReLU in the two-plane conv's epilogue, the activated tensor stored
    once as fp32 or bf16 (as `y` is); `rows`: see emit_conv_fwd_act."""
    _check_conv2p(g, x, cond, y, "plan conv2p_forward_act")
    vec = epi_row(rows, g.cout, bias, norm_mod, act_mod, x.device)
    bf = y.dtype == torch.bfloat16
    gc = g.c()
    head = (C.byref(gc), x.data_ptr(), cond.data_ptr(), wp.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr())
    kw = dict(keep=(gc, x, cond, wp, bias, y, vec, norm_mod, act_mod), desc=_gdesc(g),
              tag=_conv2p_tag(ops.conv2p_kernel_name(g, bf), g, y))
    if bf:
        prog.add("conv2p_forward_act_f32_to_bf16", lib().mpgan_conv2p_forward_act_f32_to_bf16, *head, None, y.data_ptr(),
                 g.cout, **kw)
    else:
        prog.add("conv2p_forward_act", lib().mpgan_conv2p_forward_act, *head, y.data_ptr(), g.cout, **kw)


def emit_conv2p_wgrad(prog, g: ConvGeom, x, cond, dy, dw, dbias, ws, lane=0):
    """dW (64, 2, k...) += the weight gradient over both planes from one pass over dy (fp32 or bf16); dbias rides along."""
    _check_conv2p(g, x, cond, dy, "plan conv2p_backward_weight")
    bf = dy.dtype == torch.bfloat16
    assert ws.numel() * 4 >= ops.conv2p_wgrad_workspace(g), "wgrad workspace too small"
    gc = g.c()
    prog.add("conv2p_backward_weight", lib().mpgan_conv2p_backward_weight, C.byref(gc), x.data_ptr(), cond.data_ptr(),
             dy.data_ptr(), g.cout, int(bf), dw.data_ptr(), _p(dbias), 1.0, ws.data_ptr(), ws.numel() * 4,
             keep=(gc, x, cond, dy, dw, dbias, ws), desc=_gdesc(g),
             tag=_conv2p_tag(ops.conv2p_wgrad_kernel_name(g, bf), g, dy), lane=lane)


def image_plane_geom(g: ConvGeom) -> ConvGeom:
    """The two-plane conv seen from its image plane alone: what its backward-data runs as (a C -> 1 gather over the
    layout-3 pack); the condition is data and gets no gradient."""
    return dataclasses.replace(g, cin=1)


def _t3(v, dims, fill):
    v = (v,) * dims if isinstance(v, int) else tuple(v)
    return (fill,) * (3 - dims) + tuple(v)


_GEOM_DEFAULTS = dict(mm_bf16=False)


class geom_defaults:
    """Plan-wide geometry flags while a plan is being built: `with geom_defaults(mm_bf16=True):` makes every
    conv_geom_of inside carry MPGAN_CONV_MM_BF16 (the C5 generator: bf16 matrix operands, fp32 storage)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = dict(_GEOM_DEFAULTS)
        _GEOM_DEFAULTS.update(self.kw)

    def __exit__(self, *a):
        _GEOM_DEFAULTS.clear()
        _GEOM_DEFAULTS.update(self.saved)
        return False


def conv_geom_of(mod, n, in_dhw, dims) -> ConvGeom:
    """Geometry of an nn.ConvNd / nn.ConvTransposeNd module at a given input size."""
    tr = isinstance(mod, (nn.ConvTranspose2d, nn.ConvTranspose3d))
    k, s, p = _t3(mod.kernel_size, dims, 1), _t3(mod.stride, dims, 1), _t3(mod.padding, dims, 0)
    op = _t3(mod.output_padding, dims, 0) if tr else (0, 0, 0)
    return ConvGeom(n, tuple(in_dhw), mod.in_channels, mod.out_channels, k, s, p, tr, op, **_GEOM_DEFAULTS)


class Scratch:
    """Grow-only scratch shared by the plans of one network (partials, wgrad slabs)."""

    def __init__(self, dev):
        self.dev = dev
        self.partials_need = 0
        self.ws_need = 0
        self.partials = None
        self.ws = None

    def want_partials(self, n, P, c):
        self.partials_need = max(self.partials_need, (n * ops.stats_chunks(P, c) + 32) * (3 * c + 1) + c)

    def want_ws(self, g: ConvGeom):
        self.ws_need = max(self.ws_need, ops.conv_wgrad_workspace(g) // 4)
        # fused-statistics partial rows of the forward conv (with or without prologue: same count)
        rows = max(ops.conv_stats_rows(g, code) for code in (0, 1, 2))
        self.partials_need = max(self.partials_need, (rows + 32) * 2 * g.cout)   # + finalize's fold scratch

    def want_bf16_layer(self, g: ConvGeom, fused_rows=0, two_plane=False):
        """One conv -> BN layer in bf16 storage: the forward's statistics rows (+ finalize's fold scratch), the norm
        backward's [3][C] rows (`fused_rows`: those the next layer's backward-data launch leaves instead, if more) +
        one vector + the bias partials behind them (emit_norm_bwd_bf16), and the weight gradient's workspace."""
        c, rows = g.cout, _rows(g)
        if two_plane:                      # the two-plane first layer: fp32 planes in, its own rows and slabs
            fwd_rows, ws = ops.conv2p_stats_rows(g, True), ops.conv2p_wgrad_workspace(g)
        else:
            fwd_rows = (rows + 255) // 256 if g.cin == 1 else ops.conv_stats_rows_bf16(g)
            ws = ops.conv_wgrad_workspace_bf16dy(g) if g.cin == 1 else ops.conv_wgrad_workspace_bf16(g)
        bwd_rows = max(ops.norm_bwd_rows_bf16(rows, c), fused_rows)
        self.partials_need = max(self.partials_need, (fwd_rows + 32) * 2 * c, (bwd_rows * 4 + 1) * c)
        self.ws_need = max(self.ws_need, ws // 4)

    def alloc(self):
        self.partials = torch.empty(max(self.partials_need, 4), device=self.dev)
        self.ws = torch.empty(max(self.ws_need, 4), device=self.dev)


# --------------------------------------------------------------------------
# residual U-Net
# --------------------------------------------------------------------------
class ConvUnit:
    """One `conv [+ norm + PReLU]` of a U-Net plan: the modules, the conv's pack record and geometry, its raw output `z`
    and the norm layer's device vectors, and the launches that touch them (the emit_* helpers with this unit's operands
    filled in).  `p` is the UNetPlan that carries the programs, the store, the scratch and the mode."""

    def __init__(self, p: "UNetPlan", conv, adn, in_dhw, z=None):
        self.p, self.conv = p, conv
        self.N, self.A = (adn.N, adn.A) if adn is not None else (None, None)
        self.g = g = conv_geom_of(conv, p.n, in_dhw, p.dims)
        self.rec = p.store.register_conv(conv, cout=g.cout, cin=g.cin, taps=math.prod(conv.kernel_size),
                                         transposed=g.transposed)
        self.z = z                         # None: alloc() gives it a buffer of its own, unless fuse() has by then
        self.fused = self.gf = self.zf = None
        self.nb = None
        if self.N is not None:
            self.nb = NormBuf(p.n, g.cout, p.instance, p.dev)
            p.scratch.want_partials(p.n, math.prod(g.out_dhw), g.cout)
        p.scratch.want_ws(g)

    def alloc(self) -> "ConvUnit":
        if self.z is None:
            self.z = self.p.E(self.p.n, *self.g.out_dhw, self.g.cout)
        return self

    def fuse(self, other: "ConvUnit"):
        """This conv and `other` read the same input with the same geometry: ONE forward conv over their concatenated
        output channels writes [z | other.z] (one launch, the input read once)."""
        p, c = self.p, self.g.cout
        self.fused = p.store.register_fused(self.conv, other.conv)       # before any packed offset is taken (emit)
        self.gf = dataclasses.replace(self.g, cout=c + other.g.cout)
        self.zf = p.E(p.n, *self.g.out_dhw, self.gf.cout)
        self.z, other.z = self.zf[..., :c], self.zf[..., c:]
        p.scratch.want_ws(self.gf)

    def acc_want(self, code, consumer_ok):
        """[(NormBuf, accumulator row width)] when the producing kernel (prologue `code`) can leave accumulator
        statistics and the first consumer can fold them, else []."""
        g = self.g if self.fused is None else self.gf
        return [(self.nb, g.cout)] if consumer_ok and ops.conv_acc_supported(g, code) else []

    def prologue(self) -> Prologue:
        return self.nb.prologue(ACT_LEAKY, 1.0, self.A.weight)

    def _fwd_operands(self):
        """Geometry, packed weights, bias, output and normed channel count of the forward launch: the fused pair's,
        whose first `cout` channels alone are normed, when there is one."""
        st = self.p.store
        if self.fused is not None:
            return self.gf, st.wp_fused(self.fused), st.bias_fused(self.fused), self.zf, self.g.cout
        return self.g, st.wp(self.rec), self.conv.bias, self.z, None

    def fwd_norm(self, x, pre: Optional["ConvUnit"] = None):
        """Raw output and the norm's statistics (train, and eval outside the fused path); `pre`: the unit in front,
        whose norm + PReLU is applied to x on load."""
        p = self.p
        g, w, bias, y, c_norm = self._fwd_operands()
        emit_conv_fwd_norm(p.fwd, g, x, w, bias, y, self.nb, self.N, p.scratch.partials,
                           pro=pre.prologue() if pre is not None else None, training=p.training,
                           eval_norms=p.eval_norms, c_norm=c_norm, fold=pre.nb.fold() if pre is not None else None)

    def fwd_act(self, x, y=None, resid=None, tanh=False):
        """Fused eval forward: the ACTIVATED output (running-statistics norm, PReLU, bias, `resid`) into y (default z)."""
        p = self.p
        g, w, bias, z, c_norm = self._fwd_operands()
        emit_conv_fwd_act(p.fwd, p.epi_rows, g, x, w, bias, z if y is None else y, self.N, self.A, c_norm=c_norm,
                          resid=resid, tanh=tanh)

    def fwd(self, x, resid=None, tanh=False):
        """Plain conv into z (a residual branch, the top level's conv-only unit)."""
        emit_conv_fwd(self.p.fwd, self.g, x, self.p.store.wp(self.rec), self.conv.bias, self.z, resid=resid, tanh=tanh)

    def norm_bwd(self, g, dz):
        p, gv = self.p, self.p.store.grad_view
        emit_norm_bwd(p.bwd, g, self.z, self.nb, self.prologue(), dz, p.scratch.partials, gv(self.N.weight),
                      gv(self.N.bias), gv(self.A.weight))

    def wgrad(self, x, dy, pre: Optional["ConvUnit"] = None):
        """Weight (and, for a ConvNd, bias) gradient, onto the side program."""
        p, gv = self.p, self.p.store.grad_view
        emit_conv_wgrad(p.side, self.g, x, dy, gv(self.conv.weight), p.scratch.ws,
                        pro=pre.prologue() if pre is not None else None,
                        dbias=None if self.g.transposed else gv(self.conv.bias), lane=1)

    def dgrad(self, dy, dx, resid=None):
        emit_conv_dgrad(self.p.bwd, self.g, dy, self.p.store.wp_bwd(self.rec), dx, resid=resid)


class ResidualUnit:
    """MONAI's two-subunit ResidualUnit, every down level and the bottom of the U:
    out = act(norm(conv1(act(norm(conv0(x)))))) + residual(x).  `out` is set by the plan once the unit's geometry has
    sized the buffer it is a slice of."""

    def __init__(self, p: "UNetPlan", ru, x, out=None):
        self.p, self.x, self.out = p, x, out
        m0, m1 = ru.conv
        in_dhw = tuple(x.shape[1:4])
        # MONAI's ResidualUnit has a residual conv only when the stride or the channel count changes: a bottom
        # layer with chans[-2] == chans[-1] (generator_test.py's (…, 512, 512)) adds its input unchanged.
        identity = isinstance(ru.residual, nn.Identity)
        self.u0 = ConvUnit(p, m0.conv, m0.adn, in_dhw)
        self.res = None if identity else ConvUnit(p, ru.residual, None, in_dhw)
        if not identity and _FUSE_DOWN and same_geom(self.u0.g, self.res.g):    # (never the bottom: its residual is 1x1)
            self.u0.fuse(self.res)
        self.u0.alloc()
        self.u1 = ConvUnit(p, m1.conv, m1.adn, self.u0.g.out_dhw).alloc()
        self.r = x if identity else self.res.alloc().z

    def acc_wants(self):
        # (the consumer of conv1's statistics is the residual-sum pass)
        return self.u0.acc_want(0, ops.conv_fold_supported(self.u1.g)) + self.u1.acc_want(1, True)

    def emit_forward(self):
        u0, u1 = self.u0, self.u1
        u0.fwd_norm(self.x)
        if self.res is not None and u0.fused is None:
            # (the residual conv could run on the side stream; measured: the event hand-offs cost more
            #  than the ~20 us kernels they would overlap -- G forward 4.42 -> 4.56 ms)
            self.res.fwd(self.x)
        u1.fwd_norm(u0.z, pre=u0)
        emit_norm_act_add(self.p.fwd, u1.z, u1.prologue(), self.r, None, self.out, fold=u1.nb.fold())

    def emit_forward_eval(self):
        """The fused eval path: conv1's epilogue adds the residual and writes `out`."""
        self.u0.fwd_act(self.x)                    # fused with the residual conv: its own channels alone are normed + activated
        if self.res is not None and self.u0.fused is None:
            self.res.fwd(self.x)
        self.u1.fwd_act(self.u0.z, y=self.out, resid=self.r)

    def emit_backward(self, g_out, dz1, ga0, dx, accumulate_first=True):
        """g_out = dL/d(out); dz1, ga0: scratch of conv1's output shape.  dL/dx goes to `dx`: both backward-data launches
        accumulate into it, or the first writes it (accumulate_first=False: nothing is there yet), or, with dx None,
        neither runs."""
        u0, u1, res = self.u0, self.u1, self.res
        u1.norm_bwd(g_out, dz1)
        u1.wgrad(u0.z, dz1, pre=u0)
        u1.dgrad(dz1, ga0)
        u0.norm_bwd(ga0, ga0)
        u0.wgrad(self.x, ga0)
        if res is not None:
            res.wgrad(self.x, g_out)
        if dx is None:
            return
        u0.dgrad(ga0, dx, resid=dx if accumulate_first else None)
        if res is not None:
            res.dgrad(g_out, dx, resid=dx)
        else:
            emit_norm_act_add(self.p.bwd, g_out, None, dx, None, dx)           # identity residual: dx += g_out


class UpLevel:
    """One up level: transposed conv + norm + PReLU on the concatenation `cat`, then the one-subunit ResidualUnit on its
    output -- normed, its residual act(norm(zt)) applied through the prologue pair, or, at the top of the U, conv-only
    on the materialised activation `ua`."""

    def __init__(self, p: "UNetPlan", up, cat, out, tanh):
        self.p, self.cat, self.out, self.tanh = p, cat, out, tanh
        unit = up[1].conv[0]
        adn = getattr(unit, "adn", None)
        self.top = adn is None
        self.t = t = ConvUnit(p, up[0].conv, up[0].adn, tuple(cat.shape[1:4])).alloc()
        assert t.g.out_dhw == tuple(out.shape[1:4]), (t.g.out_dhw, out.shape)
        self.u = ConvUnit(p, unit.conv, adn, t.g.out_dhw, z=out if self.top else None).alloc()
        self.ua = torch.empty_like(t.z) if self.top else None

    def acc_wants(self):
        if self.top:                               # materialised by the residual-sum pass
            return self.t.acc_want(0, True)
        return self.t.acc_want(0, ops.conv_fold_supported(self.u.g)) + self.u.acc_want(1, True)

    def emit_forward(self):
        t, u, f = self.t, self.u, self.p.fwd
        t.fwd_norm(self.cat)
        if self.top:
            emit_norm_act_add(f, t.z, t.prologue(), None, None, self.ua, fold=t.nb.fold())
            u.fwd(self.ua, resid=self.ua, tanh=self.tanh)
        else:
            u.fwd_norm(t.z, pre=t)
            emit_norm_act_add(f, u.z, u.prologue(), t.z, t.prologue(), self.out, tanh=self.tanh, fold=u.nb.fold())

    def emit_forward_eval(self):
        """The fused eval path: the transposed conv leaves act(norm(.)) itself (in `ua` at the top, else in zt)."""
        t, u = self.t, self.u
        t.fwd_act(self.cat, y=self.ua)
        if self.top:
            u.fwd(self.ua, resid=self.ua, tanh=self.tanh)
        else:
            u.fwd_act(t.z, y=self.out, resid=t.z, tanh=self.tanh)

    def emit_backward(self, g_out, dzu, gta, gcat):
        """g_out = dL/d(out); dzu, gta: scratch of zt's shape; dL/d(cat) is written to gcat."""
        t, u, p = self.t, self.u, self.p
        if self.top:
            u.wgrad(self.ua, g_out)
            u.dgrad(g_out, gta, resid=g_out)
        else:
            u.norm_bwd(g_out, dzu)
            u.wgrad(t.z, dzu, pre=t)
            u.dgrad(dzu, gta, resid=g_out)
        t.norm_bwd(gta, gta)
        emit_bias_grad(p.bwd, gta, p.store.grad_view(t.conv.bias), p.scratch.partials)
        t.wgrad(self.cat, gta)
        t.dgrad(gta, gcat)


class GradScratch(NamedTuple):
    """The gradient buffers one U-Net's backward works in."""
    gcat: list          # per level: dL/d(cat_l)
    up: list            # per up level: (dzu, gta)
    ru: list            # per down level, then the bottom: (dz1, ga0)


class UNetPlan:
    """Forward/backward programs of one residual U-Net for a fixed input shape: [down units] + bottom + [up levels]."""

    def __init__(self, unet, store: ParamStore, n: int, spatial: Sequence[int], x_in, y_out, *, tanh_out: bool,
                 instance: bool, want_backward: bool, scratch: Scratch, training: bool = True,
                 own_mark: Optional[Mark] = None, wait_mark: Optional[Mark] = None):
        self.unet, self.store, self.n, self.scratch = unet, store, n, scratch
        self.training, self.instance, self.want_backward = training, instance, want_backward
        self.dims, self.dev = unet.dimensions, x_in.device
        self.chans = chans = list(unet.channels)
        L = len(chans)                      # levels incl. bottom
        dhw0 = _t3(spatial, self.dims, 1)
        for d in range(3 - self.dims, 3):
            if dhw0[d] % (2 ** (L - 1)) != 0:
                raise ValueError(f"U-Net input extent {dhw0[d]} is not divisible by {2 ** (L - 1)}")
        self.fwd, self.bwd, self.side = Program(), Program(), Program()      # side: the weight gradients (lane 1)
        self._marks = (own_mark, wait_mark)
        self.eval_norms = [] if not training else None   # eval mode: (norm module, NormBuf, C) of every layer
        self.epi_rows = []                                # eval mode, BatchNorm: table rows of emit_conv_fwd_act
        self.eval_fused = (not training) and (not instance) and (not want_backward)
        # walk the module tree: level l = (down ResidualUnit, SkipConnection, up Sequential), the innermost submodule
        # the bottom unit.  cat_l = [down l's output | what the submodule appends] is the up level's input.
        self.downs, self.cats, up_mods = [], [], []
        x, blk = x_in, unet.model
        for l in range(L - 1):
            ru, skip, up = blk
            down = ResidualUnit(self, ru, x)
            cat = self.E(n, *down.u1.g.out_dhw, up[0].conv.in_channels)
            x = down.out = cat[..., :chans[l]]
            self.downs.append(down)
            self.cats.append(cat)
            up_mods.append(up)
            blk = skip.submodule
        assert not isinstance(blk, nn.Sequential), "U-Net depth and its channel list disagree"
        self.bottom = ResidualUnit(self, blk, x, self.cats[-1][..., chans[L - 2]:])
        self.ups = [UpLevel(self, up_mods[l], self.cats[l], self.cats[l - 1][..., chans[l - 1]:] if l > 0 else y_out,
                            tanh=tanh_out and l == 0) for l in range(L - 1)]
        # Accumulator statistics (csrc/norm_fold.h) for the norm layers whose producing kernel can leave them and
        # whose first consumer can fold them: no finalize launch for those.  (nb, accumulator row width)
        self.acc_wants = []
        if training and not instance and _ACC_STATS:
            self.acc_wants = [w for unit in self.downs + [self.bottom] + self.ups for w in unit.acc_wants()]

    def E(self, *shape):
        return torch.empty(*shape, device=self.dev)

    def grad_scratch(self) -> GradScratch:
        """One set of gradient buffers for emit(): their shapes follow from the architecture and the input shape alone,
        so the U-Nets of a generator share sets (GeneratorPlan)."""
        like = torch.empty_like
        return GradScratch(gcat=[like(c) for c in self.cats], up=[(like(u.t.z), like(u.t.z)) for u in self.ups],
                           ru=[(like(r.u1.z), like(r.u1.z)) for r in self.downs + [self.bottom]])

    # programs are emitted after the shared scratch has been sized and allocated
    def emit(self, gs: Optional[GradScratch] = None, g_out=None, g_x=None):
        """gs: the gradient scratch set of this backward; g_out = dL/dy; g_x: where dL/dx goes, None if unwanted."""
        units, chans = self.downs + [self.bottom], self.chans
        if self.eval_fused:
            # Eval-mode inference program (code/GAN/inferrence.py:97-110): every conv emits
            # its ACTIVATED output -- running-statistics BatchNorm, PReLU, bias and the unit's residual add in its
            # epilogue -- so no norm_act_add launch and no normalise-on-load prologue remain: 15 launches per U-Net
            # instead of 22, all of them convs.  Same buffers as the training plan (a raw-output buffer now holds the
            # activation).
            for unit in units + self.ups[::-1]:
                unit.emit_forward_eval()
            return
        for unit in units + self.ups[::-1]:
            unit.emit_forward()
        if not self.want_backward:
            return
        # Weight gradients run on the side stream (lane 1), all of them AFTER this U-Net's norm-backward /
        # backward-data chain has been enqueued: they only read (activation, dz) pairs that nothing
        # rewrites inside this U-Net's backward, and write parameter gradients / the split-K workspace
        # that only lane 1 touches.  One event hands the whole batch over; it then runs next to the
        # NEXT U-Net's chain, which works in the other set of gradient scratch (GeneratorPlan keeps two
        # and rotates).  `wait_mark` orders this U-Net after the side-stream work of the U-Net that
        # used the same set last.
        own_mark, wait_mark = self._marks
        b = self.bwd
        if wait_mark is not None:
            b.wait(wait_mark)
        gskip = [g[..., :c] for g, c in zip(gs.gcat, chans)]      # dL/d(down level l's output), cat_l's first half
        gsub = [g[..., c:] for g, c in zip(gs.gcat, chans)]       # dL/d(what the submodule appended to cat_l)
        for l, up in enumerate(self.ups):                         # up path, top to bottom of the U
            up.emit_backward(g_out if l == 0 else gsub[l - 1], *gs.up[l], gs.gcat[l])
        self.bottom.emit_backward(gsub[-1], *gs.ru[-1], gskip[-1])
        for l in range(len(self.downs) - 1, -1, -1):              # down path, bottom to top
            self.downs[l].emit_backward(gskip[l], *gs.ru[l], gskip[l - 1] if l > 0 else g_x, accumulate_first=l > 0)
        b.extend(self.side)
        if own_mark is not None:
            b.mark(own_mark)
        else:
            b.join()


class GeneratorPlan:
    """CasNet: chain of U-Nets + Tanh (code/GAN/GAN_final.py:92-122)."""

    def __init__(self, gen, store: ParamStore, n: int, spatial: Sequence[int], *, want_backward: bool,
                 want_input_grad: bool, instance: bool, training: bool = True, mm_bf16: bool = False):
        # mm_bf16: every MFMA-served conv of this plan rounds its matrix operands to bf16 (MPGAN_CONV_MM_BF16;
        # config C5's generator): activations, weights, statistics and gradients in HBM stay fp32
        self.mm_bf16 = mm_bf16
        unets = [m for m in gen.model if not isinstance(m, nn.Tanh)]
        dims = unets[0].dimensions
        dev = store.flat.device
        dhw = _t3(spatial, dims, 1)
        self.n, self.dhw, self.dims = n, dhw, dims
        self.store = store
        E = lambda *shape: torch.empty(*shape, device=dev)
        nU = len(unets)
        self.acts = [E(n, *dhw, 1) for _ in range(nU + 1)]   # x0 .. y
        self.x_in, self.y = self.acts[0], self.acts[-1]
        self.scratch = Scratch(dev)
        self.want_backward = want_backward
        marks = [Mark() for _ in range(nU)]
        with geom_defaults(mm_bf16=mm_bf16):
            self.unet_plans: List[UNetPlan] = [
                UNetPlan(unet, store, n, spatial, self.acts[u], self.acts[u + 1], tanh_out=(u == nU - 1),
                         instance=instance, want_backward=want_backward, scratch=self.scratch, training=training,
                         own_mark=marks[u], wait_mark=marks[u + 2] if u + 2 < nU else None)
                for u, unet in enumerate(unets)]
        self.scratch.alloc()
        wants = [w for p in self.unet_plans for w in p.acc_wants]
        self.acc_all = None
        if wants:
            total = sum(ops.ACC_REPLICAS * ops.ACC_WORDS * cw for _, cw in wants)
            self.acc_all = torch.zeros(total, dtype=torch.int64, device=dev)
            off = 0
            for nb, cw in wants:
                sz = ops.ACC_REPLICAS * ops.ACC_WORDS * cw
                nb.acc = self.acc_all[off:off + sz]
                off += sz
        if want_backward:
            # gradient scratch shared by all U-Nets (their backwards run one after another); two sets, rotated:
            # U-Net u's weight gradients (side stream) still read set u % 2 while U-Net u-1's chain fills the other one
            gsets = [self.unet_plans[0].grad_scratch(), self.unet_plans[0].grad_scratch()]
            self.g_acts = [E(n, *dhw, 1) for _ in range(nU + 1)]   # dL/d(acts[u]); never shared
            self.g_y = E(n, *dhw, 1)          # upstream gradient dL/dy is copied here
            for u, p in enumerate(self.unet_plans):
                p.emit(gsets[u % 2], self.g_acts[u + 1], self.g_acts[u] if (u > 0 or want_input_grad) else None)
        else:
            for p in self.unet_plans:
                p.emit()
        self.fwd = Program()
        store.emit_pack(self.fwd)
        if self.acc_all is not None:      # one memset for every norm layer of the forward
            self.fwd.add("zero_bytes", lib().mpgan_zero_bytes, self.acc_all.data_ptr(), self.acc_all.numel() * 8,
                         keep=(self.acc_all,))
        if not training:
            emit_eval_norms(self.fwd, [e for p in self.unet_plans for e in p.eval_norms], dev)
            emit_epi_vectors(self.fwd, [r for p in self.unet_plans for r in p.epi_rows], dev)
        for p in self.unet_plans:
            self.fwd.extend(p.fwd)
        self.bwd = Program()
        if want_backward:
            L_ = lib()
            last = self.g_acts[nU]            # = g_out of the last U-Net
            self.bwd.add("tanh_backward", L_.mpgan_tanh_backward, self.g_y.data_ptr(), self.y.data_ptr(),
                         self.y.numel(), last.data_ptr(), keep=(self.g_y, self.y, last))
            for p in reversed(self.unet_plans):
                self.bwd.extend(p.bwd)
            self.bwd.join()                   # parameter gradients are complete when the program returns
            self.g_x = self.g_acts[0] if want_input_grad else None
        self.busy = False


class IoSlots:
    """The plan's boundary tensors (network input, output, upstream gradient, input gradient) as rebindable pointer
    slots: `bind` points the programs at the caller's tensors for one pass, `reset` returns them to the plan's own
    buffers (which tools and tests that drive `plan.fwd.run()` directly keep using)."""

    def __init__(self, programs, **tensors):
        self.home, self.slot = {}, {}
        for name, t in tensors.items():
            if t is None:
                continue
            sl = C.c_void_p(t.data_ptr())
            if sum(pr.rebind(t.data_ptr(), sl) for pr in programs) == 0:
                continue
            self.home[name], self.slot[name] = t, sl

    @staticmethod
    def usable(t: torch.Tensor) -> bool:
        return t.is_contiguous() and t.dtype == torch.float32 and t.data_ptr() % 256 == 0

    def bind(self, name, t: torch.Tensor) -> bool:
        sl = self.slot.get(name)
        if sl is None or not self.usable(t) or t.numel() != self.home[name].numel():
            return False
        sl.value = t.data_ptr()
        return True

    def reset(self):
        for name, sl in self.slot.items():
            sl.value = self.home[name].data_ptr()


def plan_io(plan) -> IoSlots:
    io = getattr(plan, "io", None)
    if io is None:
        io = plan.io = IoSlots((plan.fwd, plan.bwd), x=plan.x_in, y=getattr(plan, "y", None),
                               g_y=getattr(plan, "g_y", None), g_x=getattr(plan, "g_x", None),
                               c=getattr(plan, "c_in", None))
    return io


# --------------------------------------------------------------------------
# discriminators: the conv stack and the two heads, as the plans of both variants and both storage modes hold them
# (every launch of a layer and of a head is described in one place)
# --------------------------------------------------------------------------
def _lrelu(nb: NormBuf) -> Prologue:
    return nb.prologue(ACT_LEAKY, 0.2, None)


class ConvStack:
    """The four conv -> BN -> LeakyReLU(0.2) layers of a discriminator in fp32 storage: geometries, weight records, norm
    vectors and the raw conv outputs z_i, which every consumer normalises on load (`raw_z` off, the fused eval program:
    the activated tensors are stored there instead)."""
    PEER = ops.PeerTaps                # the other pass's taps of one layer, as emit_backward's `peers` takes them
    FUSE_BWD_STATS = True              # variant A: backward-data leaves the norm-backward sums of the layer in front
    SIDE_WGRAD = True                  # emit_backward takes `wgrad_lane`: the backward program then ends in a join

    def __init__(self, disc, store: ParamStore, n: int, dhw, dims: int, *, raw_z: bool, what: str):
        dev, self.raw_z = store.flat.device, raw_z
        self.cond = None                   # the plan's condition plane, set before emitting when geoms[0].cin == 2
        self.convs = [disc.model_conv[i] for i in (0, 3, 6, 9)]
        self.bns = [disc.model_conv[i] for i in (1, 4, 7, 10)]
        self.geoms, self.zs, self.nbs, self.recs = [], [], [], []
        size = dhw
        for i, cv in enumerate(self.convs):
            g = conv_geom_of(cv, n, size, dims)
            self.geoms.append(g)
            size, c = g.out_dhw, cv.out_channels
            if min(size) < 1:
                raise ValueError(f"{what} too small")
            self._alloc_layer(i, (n, *size, c), dev)
            self.nbs.append(NormBuf(n, c, False, dev))
            self.recs.append(store.register_conv(cv, cout=c, cin=cv.in_channels, taps=math.prod(cv.kernel_size)))
        if self.two_plane:                 # backward-data of layer 0 reaches the image plane alone
            store.pack_plane0_bwd(self.convs[0])

    @property
    def two_plane(self) -> bool:
        """Layer 0 reads two 1-channel planes, the image and `cond` (the conditional discriminator)."""
        return self.geoms[0].cin == 2

    def _alloc_layer(self, i, shape, dev):
        self.zs.append(torch.empty(shape, device=dev))

    def want_scratch(self, scratch: Scratch, fuse_stats: bool):
        """Statistics partials and weight-gradient workspace of a training plan; fuse_stats: also the rows a
        backward-data launch leaves for the norm backward of the layer in front (emit_conv_dgrad_stats)."""
        for i, g in enumerate(self.geoms):
            scratch.want_partials(g.n, math.prod(g.out_dhw), g.cout)
            if i == 0 and self.two_plane:      # its own weight-gradient slabs; statistics by the separate pass
                scratch.ws_need = max(scratch.ws_need, ops.conv2p_wgrad_workspace(g) // 4)
                continue
            scratch.want_ws(g)
            if fuse_stats and g.cin > 1:
                scratch.partials_need = max(scratch.partials_need, ops.conv_bwd_stats_rows(g) * 3 * g.cin)

    def alloc_grads(self, disc):
        """(gas, dzs): the gradients w.r.t. the activations, and the dz the BatchNorm backward makes of them in place."""
        gas = [torch.empty_like(z) for z in self.zs]
        return gas, gas

    def _emit_fused_eval(self, prog, emit_layer, x, wp, outs):
        """Eval without raw z: outs[i] = LeakyReLU(BN_running(conv_i)) straight from each conv's epilogue, the epilogue
        vectors of all layers from one launch up front."""
        dev = x.device
        leaky, rows, body = _ConstSlope(0.2, dev), [], Program()
        for i, cv in enumerate(self.convs):
            if i == 0 and self.two_plane:
                emit_conv2p_fwd_act(body, rows, self.geoms[0], x, self.cond, wp(0), cv.bias, outs[0], self.bns[0], leaky)
            else:
                emit_layer(body, rows, self.geoms[i], x, wp(i), cv.bias, outs[i], self.bns[i], leaky)
            x = outs[i]
        emit_epi_vectors(prog, rows, dev)
        prog.extend(body)

    def emit_forward(self, prog, store: ParamStore, x, partials, training: bool):
        """x -> the (tensor, prologue or None) the head reads.  Training: statistics out of each conv, finalize; eval with
        raw z: scale / shift of every layer from the running statistics in one launch up front instead; eval without:
        zs[i] holds the ACTIVATED tensor."""
        wp = lambda i: store.wp(self.recs[i])
        if not self.raw_z:
            self._emit_fused_eval(prog, emit_conv_fwd_act, x, wp, self.zs)
            return self.zs[-1], None
        eval_norms, body, pro = [], Program(), None
        for i, cv in enumerate(self.convs):
            if i == 0 and self.two_plane:      # as the one-plane conv1: no fused statistics in fp32, a statistics pass
                emit_conv2p_fwd(body, self.geoms[0], x, self.cond, wp(0), cv.bias, self.zs[0])
                if training:
                    emit_norm_stats(body, self.zs[0], self.nbs[0], self.bns[0], partials)
                else:
                    eval_norms.append((self.bns[0], self.nbs[0], self.geoms[0].cout))
            else:
                emit_conv_fwd_norm(body, self.geoms[i], x, wp(i), cv.bias, self.zs[i], self.nbs[i], self.bns[i], partials,
                                   pro=pro, training=training, eval_norms=eval_norms)
            x, pro = self.zs[i], _lrelu(self.nbs[i])
        emit_eval_norms(prog, eval_norms, x.device)
        prog.extend(body)
        return x, pro

    def emit_backward(self, prog, store: ParamStore, x, gas, dzs, partials, ws, *, want_param_grads: bool, g_x,
                      peers=None, fuse_stats: bool = False, ext=None, wgrad_lane: int = 0):
        """Per layer, last to first: norm backward (in place) -> weight gradient -> backward data.
        peers: per layer, the other pass's taps (variant B's fused perceptual loss).  fuse_stats: the backward-data
        launch also leaves the norm-backward sums of the layer in front, which then needs no reduce pass (variant A).
        ext: per layer, the gradients (gz, gy, ga) deposited into the materialised taps (conv out, norm out, activation):
            g_a += G_a;  dz = BNbwd_act(g_a) + BNbwd_identity(G_y) + G_z
        (BatchNorm's backward is linear in the gradient of its output, so the y-tap's gradient goes through a second
        norm backward with an identity activation; both add into dgamma / dbeta) -- three more element-wise passes."""
        gv = store.grad_view if want_param_grads else (lambda p: None)
        add = lambda dst, src: prog.add("axpby", lib().mpgan_axpby, dst.data_ptr(), 1.0, src.data_ptr(), 1.0, dst.numel(),
                                        dst.data_ptr(), keep=(dst, src))
        reduced = 0                                  # rows the previous backward-data launch left in `partials`
        for i in range(len(self.convs) - 1, -1, -1):
            g, z, nb, bn, cv = gas[i], self.zs[i], self.nbs[i], self.bns[i], self.convs[i]
            if ext is not None:
                add(g, ext[i][2])
            emit_norm_bwd(prog, g, z, nb, _lrelu(nb), g, partials, gv(bn.weight), gv(bn.bias), None,
                          peer=peers[i] if peers is not None else None, reduced_rows=reduced)
            if ext is not None:
                gz, gy, _ = ext[i]
                emit_norm_bwd(prog, gy, z, nb, nb.prologue(ACT_NONE), gy, partials, gv(bn.weight), gv(bn.bias), None)
                add(g, gy)
                add(g, gz)
            if want_param_grads and i == 0 and self.two_plane:
                emit_conv2p_wgrad(prog, self.geoms[0], x, self.cond, g, gv(cv.weight), gv(cv.bias), ws, lane=wgrad_lane)
            elif want_param_grads:
                emit_conv_wgrad(prog, self.geoms[i], self.zs[i - 1] if i > 0 else x, g, gv(cv.weight), ws,
                                pro=_lrelu(self.nbs[i - 1]) if i > 0 else None, dbias=gv(cv.bias), lane=wgrad_lane)
            if i > 0 and fuse_stats:
                reduced = emit_conv_dgrad_stats(prog, self.geoms[i], g, store.wp_bwd(self.recs[i]), gas[i - 1],
                                                self.zs[i - 1], self.nbs[i - 1], 0.2, partials)
            elif i > 0:
                emit_conv_dgrad(prog, self.geoms[i], g, store.wp_bwd(self.recs[i]), gas[i - 1])
            elif g_x is not None:    # (two planes: the image plane's gradient alone, over the layout-3 pack)
                emit_conv_dgrad(prog, image_plane_geom(self.geoms[0]), g, store.wp_bwd(self.recs[0]), g_x)


class ConvStackBF16(ConvStack):
    """The same layers in bf16 storage: bf16 packs of the three dense convs, the raw conv outputs z_i
    (bf16; none where `raw_z` is off: the fused eval program) and the activations a_i (bf16; fp32 for the last layer,
    which the fp32 head reads)."""
    PEER = ops.PeerTapsBF16
    FUSE_BWD_STATS = _FUSE_BWD_STATS_BF16
    SIDE_WGRAD = False

    def __init__(self, disc, store: ParamStore, n: int, dhw, dims: int, *, raw_z: bool, what: str):
        self.acts = []
        super().__init__(disc, store, n, dhw, dims, raw_z=raw_z, what=what)
        self.packs = PacksBF16(self.recs[1:], store.flat.device)

    def _alloc_layer(self, i, shape, dev):
        if self.raw_z:
            self.zs.append(torch.empty(shape, device=dev, dtype=torch.bfloat16))
        self.acts.append(torch.empty(shape, device=dev, dtype=torch.float32 if i == 3 else torch.bfloat16))

    def want_scratch(self, scratch: Scratch, fuse_stats: bool):
        for i, g in enumerate(self.geoms):
            # (rows of the fused norm-backward sums the NEXT layer's backward-data launch leaves for this layer's norm)
            scratch.want_bf16_layer(g, bwd_stats_rows_bf16(self.geoms[i + 1]) if fuse_stats and i < 3 else 0,
                                    two_plane=i == 0 and self.two_plane)

    def alloc_grads(self, disc):
        """(gas, dzs): the gradients w.r.t. the activations (bf16; fp32 for a_3, which the fp32 head writes) and the
        dz the BatchNorm backward makes of them -- in place, but for the last layer's bf16 dz and under
        disc.debug_keep_intermediates (separate dz buffers, so that tests can check every layer of the backward
        against the CPU restatement on the SAME inputs)."""
        gas = [torch.empty_like(z) for z in self.zs[:3]] + [torch.empty_like(self.acts[3])]
        keep_all = bool(getattr(disc, "debug_keep_intermediates", False))
        return gas, [torch.empty_like(z) if keep_all or i == 3 else gas[i] for i, z in enumerate(self.zs)]

    def emit_forward(self, prog, store: ParamStore, x, partials, training: bool):
        """The bf16 weight packs, then x -> (a_3, None).  Training: statistics out of each conv, finalize, norm_act_bf16;
        eval with raw z: scale / shift of every layer from the running statistics in one launch up front instead; eval
        without: each a_i straight from its conv's epilogue."""
        self.packs.emit(prog, store)
        wp = lambda i: store.wp(self.recs[0]) if i == 0 else self.packs.fwd(self.recs[i])
        if not self.raw_z:
            self._emit_fused_eval(prog, emit_conv_fwd_act_bf16, x, wp, self.acts)
            return self.acts[3], None
        if not training:
            emit_eval_norms(prog, [(bn, nb, g.cout) for bn, nb, g in zip(self.bns, self.nbs, self.geoms)], x.device)
        for i, cv in enumerate(self.convs):
            if i == 0 and self.two_plane:
                rows = emit_conv2p_fwd(prog, self.geoms[0], x, self.cond, wp(0), cv.bias, self.zs[0],
                                       partials if training else None)
            else:
                rows = emit_conv_fwd_bf16(prog, self.geoms[i], x, wp(i), cv.bias, self.zs[i], partials if training else None)
            emit_norm_act_bf16(prog, self.zs[i], self.nbs[i], 0.2, self.acts[i], self.bns[i] if training else None,
                               partials, rows)
            x = self.acts[i]
        return x, None

    def emit_backward(self, prog, store: ParamStore, x, gas, dzs, partials, ws, *, want_param_grads: bool, g_x,
                      peers=None, fuse_stats: bool = False):
        """As ConvStack.emit_backward, on the stored bf16 tensors: dz_i goes to dzs[i], the weight gradients stay on the
        caller's stream, and there is no `ext` (gradients through materialised taps are fp32 storage only)."""
        gv = store.grad_view if want_param_grads else (lambda p: None)
        reduced = 0                                  # rows the previous backward-data launch left in `partials`
        for i in range(len(self.convs) - 1, -1, -1):
            dz, bn, cv = dzs[i], self.bns[i], self.convs[i]
            bias_part = emit_norm_bwd_bf16(prog, gas[i], self.zs[i], self.nbs[i], 0.2, dz, partials, gv(bn.weight),
                                           gv(bn.bias), peer=peers[i] if peers is not None else None,
                                           reduced_rows=reduced, bias_part=want_param_grads and i > 0)
            if want_param_grads and i == 0 and self.two_plane:
                emit_conv2p_wgrad(prog, self.geoms[0], x, self.cond, dz, gv(cv.weight), gv(cv.bias), ws)
            elif want_param_grads:
                emit_conv_wgrad_bf16(prog, self.geoms[i], self.acts[i - 1] if i > 0 else x, dz, gv(cv.weight),
                                     gv(cv.bias), ws, bias_part)
            if i > 0:
                # (fuse_stats: ... and the reduce pass of the layer in front in the same launch)
                reduced = emit_conv_dgrad_bf16(prog, self.geoms[i], dz, self.packs.bwd(self.recs[i]), gas[i - 1],
                                               stats=(self.zs[i - 1], self.nbs[i - 1], 0.2, partials) if fuse_stats else None)
            elif g_x is not None:
                emit_conv_dgrad_bf16(prog, image_plane_geom(self.geoms[0]), dz, store.wp_bwd(self.recs[0]), g_x)


class LinearHead:
    """Variant A's head, Flatten -> Linear(F,1) -> Sigmoid, on the last layer's tensor `src` read through `pro` (raw z
    with the BatchNorm + LeakyReLU prologue, or an activated fp32 tensor with none).  With disc.output == "logit" the
    Sigmoid is not applied: no `prob`, and the backward starts from `dlogit`, which the caller fills."""

    def __init__(self, disc, store: ParamStore, n: int, g_last: ConvGeom, spatial):
        dev = store.flat.device
        self.lin, self.n = disc.model_linear[1], n
        self.logits_out = getattr(disc, "output", "prob") == "logit"
        self.P, self.c = math.prod(g_last.out_dhw), g_last.cout
        if self.lin.in_features != self.P * self.c:
            raise ValueError(f"Linear.in_features {self.lin.in_features} != {self.c}*{self.P} for input {spatial}")
        self.rlin = store.register_conv(self.lin, cout=1, cin=self.c, taps=self.P)
        self.logit, self.prob = torch.empty(n, device=dev), (None if self.logits_out else torch.empty(n, device=dev))
        self.lin_part = torch.empty(ops.linear1_partials(n), device=dev)

    def emit_forward(self, prog, store: ParamStore, src, pro):
        pc = pro.c() if pro is not None else None
        prog.add("linear1_forward", lib().mpgan_linear1_forward, src.data_ptr(), C.byref(pc) if pc is not None else None,
                 self.n, self.P, self.c, store.wp(self.rlin).data_ptr(), self.lin.bias.data_ptr(),
                 self.lin_part.data_ptr(), self.logit.data_ptr(), _p(self.prob), keep=(pc, pro, src, self))

    def emit_backward(self, prog, store: ParamStore, src, pro, g_src, want_param_grads: bool):
        """g_prob (allocated here; the caller fills it; `dlogit` with disc.output == "logit") -> g_src, the gradient
        w.r.t. what `src` holds after `pro`."""
        gv = store.grad_view if want_param_grads else (lambda p: None)
        L, pc = lib(), (pro.c() if pro is not None else None)
        if self.logits_out:
            self.g_prob, dlogit = None, torch.empty_like(self.logit)
            self.dlogit = dlogit
        else:
            self.g_prob, dlogit = torch.empty_like(self.prob), torch.empty_like(self.prob)
            prog.add("sigmoid_backward", L.mpgan_sigmoid_backward, self.g_prob.data_ptr(), self.prob.data_ptr(), self.n,
                     dlogit.data_ptr(), keep=(dlogit, self))
        prog.add("linear1_backward", L.mpgan_linear1_backward, src.data_ptr(), C.byref(pc) if pc is not None else None,
                 self.n, self.P, self.c, store.wp(self.rlin).data_ptr(), dlogit.data_ptr(), g_src.data_ptr(),
                 _p(gv(self.lin.weight)), _p(gv(self.lin.bias)), 1.0, keep=(pc, pro, src, g_src, dlogit))


class MapHead:
    """Variant A's Markovian (PatchGAN) head, a last valid Conv(256, 1, k) -> Sigmoid on the last layer's tensor `src`
    read through `pro` (see LinearHead): a map of per-receptive-field verdicts, out = last - k + 1 per dimension.  One
    fp32 class for all four plans: the bf16 and the eval stacks hand it an fp32 activated tensor and no prologue.
    disc.output == "logit": as in LinearHead."""

    def __init__(self, disc, store: ParamStore, n: int, g_last: ConvGeom, spatial):
        dev = store.flat.device
        self.logits_out = getattr(disc, "output", "prob") == "logit"
        self.conv, self.n, self.c = disc.model_head[0], n, g_last.cout
        self.in_dhw = tuple(g_last.out_dhw)
        self.k = _t3(self.conv.kernel_size, disc.dimensions, 1)
        if min(i - k for i, k in zip(self.in_dhw, self.k)) < 0:
            raise ValueError(f"last feature map {self.in_dhw} smaller than the head's kernel {self.k} for input {spatial}")
        self.map_dhw = tuple(i - k + 1 for i, k in zip(self.in_dhw, self.k))
        self.P = math.prod(self.map_dhw)
        self.rconv = store.register_conv(self.conv, cout=1, cin=self.c, taps=math.prod(self.k))
        self.logit = torch.empty(n * self.P, device=dev)
        self.prob = None if self.logits_out else torch.empty(n * self.P, device=dev)
        self._in3, self._k3 = (C.c_int32 * 3)(*self.in_dhw), (C.c_int32 * 3)(*self.k)

    def emit_forward(self, prog, store: ParamStore, src, pro):
        pc = pro.c() if pro is not None else None
        prog.add("maphead_forward", lib().mpgan_maphead_forward, src.data_ptr(), C.byref(pc) if pc is not None else None,
                 self.n, self._in3, self.c, self._k3, store.wp(self.rconv).data_ptr(), self.conv.bias.data_ptr(),
                 self.logit.data_ptr(), _p(self.prob), keep=(pc, pro, src, self))

    def emit_backward(self, prog, store: ParamStore, src, pro, g_src, want_param_grads: bool):
        """g_prob (allocated here; the caller fills it; `dlogit` with disc.output == "logit") -> g_src, the gradient
        w.r.t. what `src` holds after `pro`."""
        gv = store.grad_view if want_param_grads else (lambda p: None)
        L, pc = lib(), (pro.c() if pro is not None else None)
        self.g_prob = None if self.logits_out else torch.empty_like(self.logit)
        dlogit = torch.empty_like(self.logit)
        self.dlogit = dlogit                        # read by tests: what maphead_backward was given
        ws_bytes = ops.maphead_workspace(self.n, self.in_dhw, self.c, self.k) if want_param_grads else 0
        ws = torch.empty(max(ws_bytes // 4, 4), device=self.logit.device) if want_param_grads else None
        if not self.logits_out:
            prog.add("sigmoid_backward", L.mpgan_sigmoid_backward, self.g_prob.data_ptr(), self.prob.data_ptr(),
                     self.n * self.P, dlogit.data_ptr(), keep=(dlogit, self))
        prog.add("maphead_backward", L.mpgan_maphead_backward, src.data_ptr(), C.byref(pc) if pc is not None else None,
                 self.n, self._in3, self.c, self._k3, store.wp(self.rconv).data_ptr(), dlogit.data_ptr(),
                 g_src.data_ptr(), _p(gv(self.conv.weight)), _p(gv(self.conv.bias)), 1.0, _p(ws), ws_bytes,
                 keep=(pc, pro, src, g_src, ws, dlogit))


class PatchHead:
    """Variant B's head, Flatten -> Linear(F,64) -> Linear(64,1) -> Sigmoid, on the last layer's tensor `src` read
    through `pro` (see LinearHead).  Linear(F,64) is a conv whose kernel spans the last feature map (packing realises
    the flatten order), split over K; Linear(64,1) a 1x1x1 conv."""

    def __init__(self, disc, store: ParamStore, n: int, g_last: ConvGeom, spatial):
        dev = store.flat.device
        E = lambda *shape: torch.empty(*shape, device=dev)
        lin1, lin2 = disc.model_linear[1], disc.model_linear[2]
        self.lin1, self.lin2, self.n = lin1, lin2, n
        size, c_last = tuple(g_last.out_dhw), g_last.cout
        P_last = math.prod(size)
        if lin1.in_features != P_last * c_last:
            raise ValueError(f"Linear.in_features {lin1.in_features} != {c_last}*{P_last} for patches {spatial}")
        self.g_l1 = ConvGeom(n, size, c_last, lin1.out_features, size, (1, 1, 1), (0, 0, 0))
        self.g_l2 = ConvGeom(n, (1, 1, 1), lin1.out_features, 1, (1, 1, 1), (1, 1, 1), (0, 0, 0))
        self.r_l1 = store.register_conv(lin1, cout=lin1.out_features, cin=c_last, taps=P_last, tco=True)
        # its data gradient as ONE GEMM: (P x 64) * (64 x taps*C) -> the channels-last gradient of the last map
        self.g_l1_bwd = ConvGeom(n, (1, 1, 1), lin1.out_features, P_last * c_last, (1, 1, 1), (1, 1, 1), (0, 0, 0))
        self.r_l2 = store.register_conv(lin2, cout=1, cin=lin1.out_features, taps=1)
        self.h = E(n, 1, 1, 1, lin1.out_features)
        self.logit, self.prob = E(n, 1, 1, 1, 1), E(n)
        self.splitk_ws = E(max(ops.conv_splitk_workspace(self.g_l1) // 4, 4))

    def want_scratch(self, scratch: Scratch):
        scratch.want_ws(self.g_l1)
        scratch.want_ws(self.g_l2)

    def alloc_grads(self):
        """Head gradients, and those arriving through the perceptual taps of the three head tensors (zero unless a
        perceptual loss deposited them)."""
        dev, n = self.h.device, self.n
        self.g_prob = torch.empty(n, device=dev)
        self.dlogit = torch.empty(n, 1, 1, 1, 1, device=dev)
        self.dh = torch.empty_like(self.h)
        self.tap_g_h, self.tap_g_logit, self.tap_g_prob = (torch.zeros(*s, device=dev) for s in (self.h.shape, (n,), (n,)))

    def emit_forward(self, prog, store: ParamStore, src, pro):
        gc1, pc = self.g_l1.c(), (pro.c() if pro is not None else None)
        prog.add("conv_forward_splitk", lib().mpgan_conv_forward_splitk, C.byref(gc1), src.data_ptr(), _ld(src),
                 store.wp(self.r_l1).data_ptr(), self.lin1.bias.data_ptr(), C.byref(pc) if pc is not None else None,
                 self.splitk_ws.data_ptr(), self.splitk_ws.numel() * 4, self.h.data_ptr(), _ld(self.h),
                 keep=(gc1, pc, pro, src, self), tag=("gather_conv_pipe_kernel<splitK>", 2.0 * conv_macs(self.g_l1)))
        emit_conv_fwd(prog, self.g_l2, self.h, store.wp(self.r_l2), self.lin2.bias, self.logit)
        prog.add("sigmoid_forward", lib().mpgan_sigmoid_forward, self.logit.data_ptr(), self.n, self.prob.data_ptr())

    def emit_backward(self, prog, store: ParamStore, src, pro, g_src, ws, want_param_grads: bool):
        """g_prob and the head taps' gradients -> g_src, the gradient w.r.t. what `src` holds after `pro`."""
        gv = store.grad_view if want_param_grads else (lambda p: None)
        L, n = lib(), self.n
        # sigmoid: dlogit = (g_prob + tap_prob) * p(1-p) + tap_logit
        prog.add("axpby", L.mpgan_axpby, self.g_prob.data_ptr(), 1.0, self.tap_g_prob.data_ptr(), 1.0, n,
                 self.g_prob.data_ptr(), keep=(self,))
        prog.add("sigmoid_backward", L.mpgan_sigmoid_backward, self.g_prob.data_ptr(), self.prob.data_ptr(), n,
                 self.dlogit.data_ptr())
        prog.add("axpby", L.mpgan_axpby, self.dlogit.data_ptr(), 1.0, self.tap_g_logit.data_ptr(), 1.0, n,
                 self.dlogit.data_ptr())
        if want_param_grads:
            emit_conv_wgrad(prog, self.g_l2, self.h, self.dlogit, gv(self.lin2.weight), ws, dbias=gv(self.lin2.bias))
        emit_conv_dgrad(prog, self.g_l2, self.dlogit, store.wp_bwd(self.r_l2), self.dh, resid=self.tap_g_h)
        if want_param_grads:
            emit_conv_wgrad(prog, self.g_l1, src, self.dh, gv(self.lin1.weight), ws, pro=pro, dbias=gv(self.lin1.bias))
        emit_conv_fwd(prog, self.g_l1_bwd, self.dh, store.wp_tco(self.r_l1), None, g_src.view(n, 1, 1, 1, -1))


class _DiscPlanBase:
    """What the plans of both discriminators share: the boundary, the conv stack (fp32 storage here; the bf16 plans
    mix in _StorageBF16) and its attributes as tests, tools and networks.py read them off the plan."""

    def _make_stack(self, disc, what: str, raw_z: bool):
        return ConvStack(disc, self.store, self.n, self.dhw, self.dims, raw_z=raw_z, what=what)

    def _setup(self, disc, store: ParamStore, n: int, spatial, what: str, *, training: bool, want_backward: bool,
               raw_z: bool):
        assert training or not want_backward, "eval plans are forward-only"
        self.n, self.dims, self.store, self.training = n, disc.dimensions, store, training
        self.dhw = _t3(spatial, self.dims, 1)
        self.x_in = torch.empty(n, *self.dhw, 1, device=store.flat.device)
        st = self.stack = self._make_stack(disc, f"{what} {spatial}", raw_z)
        # the conditional discriminator: the condition plane, bound like x_in (IoSlots "c")
        self.c_in = st.cond = torch.empty_like(self.x_in) if st.two_plane else None
        self.convs, self.bns, self.geoms, self.zs, self.nbs, self.recs = st.convs, st.bns, st.geoms, st.zs, st.nbs, st.recs
        return st


class _StorageBF16:
    def _make_stack(self, disc, what: str, raw_z: bool):
        st = ConvStackBF16(disc, self.store, self.n, self.dhw, self.dims, raw_z=raw_z, what=what)
        self.acts = st.acts
        return st


# --------------------------------------------------------------------------
# discriminator (variant A)
# --------------------------------------------------------------------------
class DiscPlan(_DiscPlanBase):
    """4 x (valid conv -> BN -> LeakyReLU 0.2) -> Flatten -> Linear(F,1) -> Sigmoid
    (code/GAN/GAN_final.py:159-209); with disc.head == "markovian" the head is Conv(256, 1, 4) -> Sigmoid instead
    (MapHead: `logit` / `prob` then hold a map per sample)."""

    def __init__(self, disc, store: ParamStore, n: int, spatial: Sequence[int], *, want_backward: bool,
                 want_input_grad: bool, want_param_grads: bool, training: bool = True):
        """training=False: the eval-mode program (running-statistics BatchNorm, forward only): every layer's BatchNorm
        + LeakyReLU rides in its conv's epilogue (mpgan_conv_forward_act; mpgan_conv_forward_act_bf16 in bf16 storage),
        the activated tensors are the only ones stored -- no raw z, no statistics, no norm_act_bf16 pass -- and the head
        reads the last one without a prologue.  The affine vectors are recomputed on the device at every run from the
        live parameters and running statistics; nothing else of the module is touched."""
        st = self._setup(disc, store, n, spatial, "discriminator input", training=training, want_backward=want_backward,
                         raw_z=training)
        head_cls = MapHead if getattr(disc, "head", "linear") == "markovian" else LinearHead
        head = self.head = head_cls(disc, store, n, st.geoms[-1], spatial)
        self.logit, self.prob = head.logit, head.prob
        scratch = Scratch(store.flat.device)
        if training:       # eval: no statistics partials, no weight-gradient workspace
            st.want_scratch(scratch, st.FUSE_BWD_STATS)
        scratch.alloc()
        f = self.fwd = Program()
        store.emit_pack(f)
        src, pro = st.emit_forward(f, store, self.x_in, scratch.partials, training)
        head.emit_forward(f, store, src, pro)
        self.busy = False
        b = self.bwd = Program()
        self.g_x = None
        if not want_backward:
            return
        if want_input_grad:
            self.g_x = torch.empty_like(self.x_in)
        # raw conv outputs, their gradients (`dzs`: after the norm backward), norm vectors: read by tests and tools
        self.gas, self.dzs = st.alloc_grads(disc)
        head.emit_backward(b, store, src, pro, self.gas[-1], want_param_grads)
        # what the caller fills before running `bwd`: g_prob, or with disc.output == "logit" g_logit (the other is None)
        self.g_prob, self.g_logit = head.g_prob, (head.dlogit if head.logits_out else None)
        st.emit_backward(b, store, self.x_in, self.gas, self.dzs, scratch.partials, scratch.ws,
                         want_param_grads=want_param_grads, g_x=self.g_x, fuse_stats=st.FUSE_BWD_STATS,
                         **(dict(wgrad_lane=_D_WGRAD_LANE) if st.SIDE_WGRAD else {}))
        if st.SIDE_WGRAD:
            b.join()


class DiscPlanBF16(_StorageBF16, DiscPlan):
    """The same network as DiscPlan with bf16 activations, activation gradients and packed weights in HBM
    (code/GAN/GAN_final.py:159-209 at the reference's 3-D shape); fp32 accumulation, statistics, parameters,
    weight gradients and Adam.  Per layer: raw conv output z (bf16) + fused fp32 statistics -> finalize ->
    a = LeakyReLU(BN(z)) materialised once (bf16; fp32 for the last layer, which the fp32 Linear head reads).
    The first layer (1 input channel) runs on the HBM-bound VALU kernels with fp32 weights."""


# --------------------------------------------------------------------------
# patch discriminator (variant B)
# --------------------------------------------------------------------------
class PatchDiscPlan(_DiscPlanBase):
    """4 x (valid k3 conv -> BN -> LeakyReLU 0.2) -> Flatten -> Linear(F,64) -> Linear(64,1) ->
    Sigmoid on small patches (test_runs/GAN.py:136-198).  The 16 perceptual taps are never
    materialised: their L1 terms and gradients come from the raw conv outputs of the two
    passes (`peer`), see mpgan_peer_taps."""

    def __init__(self, disc, store: ParamStore, n: int, spatial: Sequence[int], *, want_backward: bool,
                 want_input_grad: bool, want_param_grads: bool, training: bool = True, keep_taps: bool = True):
        """training=False: one of the two eval-mode programs (running-statistics BatchNorm, forward only).
        keep_taps: the raw z_i are stored as in training and every BatchNorm's scale / shift come from ONE
        mpgan_norm_from_running_multi launch instead of statistics + finalize -- consumers normalise on load (bf16
        storage: norm_act_bf16 as in training), and TapSet.materialize / the fused perceptual loss read the plan exactly
        as they read a training one (values only).
        not keep_taps: the fused program of DiscPlan (BatchNorm + LeakyReLU in each conv's epilogue, activated tensors
        only), the head reading the last one without a prologue."""
        self.disc, self.keep_taps = disc, keep_taps
        self.want_input_grad, self.want_param_grads = want_input_grad, want_param_grads
        st = self._setup(disc, store, n, spatial, "patch discriminator input", training=training,
                         want_backward=want_backward, raw_z=training or keep_taps)
        head = self.head = PatchHead(disc, store, n, st.geoms[-1], spatial)
        self.lin1, self.lin2, self.h, self.logit, self.prob = head.lin1, head.lin2, head.h, head.logit, head.prob
        dev = store.flat.device
        scratch = self.scratch = Scratch(dev)
        if training:
            st.want_scratch(scratch, False)
            head.want_scratch(scratch)
        scratch.alloc()
        self.lrelu = _lrelu
        f = self.fwd = Program()
        store.emit_pack(f)
        self._head_in = st.emit_forward(f, store, self.x_in, scratch.partials, training)
        head.emit_forward(f, store, *self._head_in)
        self.busy = False
        self.g_x = None
        self._bwd_cache = {}
        if not training and keep_taps:
            self._perc_weights(dev)
        if not want_backward:
            return
        self.gas, self.dzs = st.alloc_grads(disc)
        self._tap_buffers(dev)
        if want_input_grad:
            self.g_x = torch.empty_like(self.x_in)

    def _tap_buffers(self, dev):
        """Head gradients and the perceptual loss's per-plan state (both storage modes)."""
        head = self.head
        head.alloc_grads()
        self.g_prob, self.dlogit, self.dh = head.g_prob, head.dlogit, head.dh
        self.tap_g_h, self.tap_g_logit, self.tap_g_prob = head.tap_g_h, head.tap_g_logit, head.tap_g_prob
        # the per-layer (z, y, a) coefficients of the perceptual taps
        self.coef_all = torch.zeros(4 * len(self.convs), device=dev)   # one buffer: the perceptual loss fills it in one launch
        self.coef = [self.coef_all[4 * i:4 * i + 4] for i in range(len(self.convs))]
        self._perc_weights(dev)

    def _perc_weights(self, dev):
        """The perceptual loss's constant weights (all a tap-keeping eval plan needs of _tap_buffers: value only)."""
        # constant weights of the perceptual loss (test_runs/GAN.py:288-298: every tap's L1 mean / its numel; Flatten
        # repeats the last activation, key 12): forward terms in the order [layer0 z, y, a, layer1 ..., h, logit, prob]
        nl = len(self.convs)
        wf, wb = [], []
        for i, z in enumerate(self.zs):
            nel = float(z.numel())
            last = 2.0 if i == nl - 1 else 1.0
            wf += [1.0 / nel, 1.0 / nel, last / nel]
            wb += [1.0 / (nel * nel), 1.0 / (nel * nel), last / (nel * nel), 0.0]
        wf += [1.0 / self.h.numel(), 1.0 / self.logit.numel(), 1.0 / self.prob.numel()]
        self.perc_w_fwd = torch.tensor(wf, device=dev)
        self.perc_w_bwd = torch.tensor(wb, device=dev)

    def backward_program(self, peer: Optional["PatchDiscPlan"], ext=None) -> Program:
        """The head, then the conv stack; peer: the other pass of a fused perceptual loss; ext: see backward_program_ext."""
        key = id(peer) if peer is not None else 0
        if ext is not None:
            key = ("ext", key)
        if key in self._bwd_cache:
            return self._bwd_cache[key]
        st, store, b = self.stack, self.store, Program()
        self.head.emit_backward(b, store, *self._head_in, self.gas[-1], self.scratch.ws, self.want_param_grads)
        peers = None
        if peer is not None:
            peers = [st.PEER(peer.zs[i], peer.nbs[i].scale, peer.nbs[i].shift, self.coef[i]) for i in range(len(self.convs))]
        st.emit_backward(b, store, self.x_in, self.gas, self.dzs, self.scratch.partials, self.scratch.ws,
                         want_param_grads=self.want_param_grads, g_x=self.g_x, peers=peers,
                         **(dict(ext=ext) if ext is not None else {}))
        self._bwd_cache[key] = b
        return b

    def clear_taps(self):
        if hasattr(self, "tap_g_h"):
            self.tap_g_h.zero_()
            self.tap_g_logit.zero_()
            self.tap_g_prob.zero_()
        self.peer = None
        if getattr(self, "ext_used", False):
            self.clear_ext()

    # ---- external gradients on materialised taps (the reference's own perceptual_loss body on TapDict values) ----
    def _ext_buffers(self):
        if not hasattr(self, "gext"):
            # per conv layer: gradients arriving on (z, y, a) = (conv out, norm out, activation) as channels-last tensors
            self.gext = [[torch.zeros_like(z) for _ in range(3)] for z in self.zs]
            self.ext_used = False
        return self.gext

    def deposit_tap_grad(self, key: int, g: torch.Tensor):
        """Gradient of one of the 16 taps (NC(D)HW, as TapSet.materialize returned it)."""
        if not hasattr(self, "gas"):
            raise RuntimeError("this discriminator pass was run without a backward (no gradient can flow into its taps)")
        ge = self._ext_buffers()
        n = self.n
        if key < 12 or key == 12:
            i, kind = (3, 2) if key == 12 else divmod(key, 3)
            z = self.zs[i]
            gg = g.reshape(n, z.shape[-1], *z.shape[1:4])                     # NCDHW (2-D taps: D = 1)
            ge[i][kind].add_(gg.permute(0, 2, 3, 4, 1))
        elif key == 13:
            self.tap_g_h.view(n, -1).add_(g.reshape(n, -1))
        elif key == 14:
            self.tap_g_logit.add_(g.reshape(-1))
        else:
            self.tap_g_prob.add_(g.reshape(-1))
        self.ext_used = True

    def clear_ext(self):
        if hasattr(self, "gext"):
            for trio in self.gext:
                for t in trio:
                    t.zero_()
        self.ext_used = False

    def backward_program_ext(self, peer: Optional["PatchDiscPlan"]) -> Program:
        """backward_program with the external tap gradients folded in, layer by layer (ConvStack.emit_backward's `ext`).
        A compatibility path built from the existing kernels."""
        return self.backward_program(peer, ext=self._ext_buffers())


class PatchDiscPlanBF16(_StorageBF16, PatchDiscPlan):
    """PatchDiscPlan with DiscPlanBF16's storage contract: bf16 raw conv outputs z_i, activations
    a_0..a_2, activation gradients and packed weights of the three dense convs in HBM; fp32 accumulation, statistics,
    parameters, weight gradients and Adam.  a_3 and its gradient stay fp32 for the fp32 split-K head, which reads a_3
    with no prologue.  The perceptual taps are defined on the STORED z_i (y = z_i*scale + shift, a = LeakyReLU(y) in
    fp32): their values come from mpgan_tap_l1_bf16, their gradients from the peer entries of the bf16 norm backward.
    Gradients deposited into materialised taps are not offered (deposit_tap_grad raises)."""

    def deposit_tap_grad(self, key: int, g: torch.Tensor):
        raise NotImplementedError(
            "gradients through materialised perceptual taps are not offered in bf16 storage mode: use the fused "
            "mpgan_amd.gan_patch.perceptual_loss on the two TapDicts (or storage_dtype='f32')")

    def backward_program_ext(self, peer):
        raise NotImplementedError("backward_program_ext: fp32 storage only (see deposit_tap_grad)")
