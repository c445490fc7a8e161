#!/usr/bin/env python3
"""The frozen launch lists of the discriminator plans, fp32 and bf16 storage, and of the generator's plans, in a form that
can be diffed across commits (development aid: builds the plans, launches nothing).

    python tools/dump_programs.py [--storage {bf16,f32,both}]        # variant A and B, every program
    python tools/dump_programs.py --tree DIR                         # the same of another built checkout (the parent commit)
    python tools/dump_programs.py --head markovian                   # variant A with the Markovian (PatchGAN) head
    python tools/dump_programs.py --conditional [--head markovian]   # variant A conditional: D(cat(img, cond)), DESIGN.md 7e
    MPGAN_FUSE_BWD_STATS_BF16=1 python tools/dump_programs.py        # bf16 variant A train with the fused norm-backward sums
    MPGAN_DBG_NO_FUSE_BWD_STATS=1 python tools/dump_programs.py      # fp32 variant A train without them
    python tools/dump_programs.py --net generator                    # GeneratorPlan.fwd / .bwd of GENERATOR_CASES, 3 U-Nets each
    MPGAN_DBG_NO_FUSE_DOWN=1 python tools/dump_programs.py --net generator   # ... first conv and residual conv as two launches
    MPGAN_ACC_STATS=1 python tools/dump_programs.py --net generator  # ... with accumulator statistics (no finalize launches)
    python tools/dump_programs.py ... --digest                       # one line per program: call count, sha256 of its lines

One line per call: index, name, desc, tag, lane, the C entry and its arguments.  Every pointer (an argument or a structure
field the C signature declares as one) is replaced by an ordinal in order of first appearance within its plan (p0, p1,
...), so that the aliasing pattern is compared and the addresses are not; byref structures are expanded field by field.
Needs an MI355X only because the plans allocate their tensors there."""
import argparse
import ctypes as C
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ap = argparse.ArgumentParser()
_ap.add_argument("--storage", default="both", choices=("bf16", "f32", "both"))
_ap.add_argument("--head", default="linear", choices=("linear", "markovian"),
                 help="variant A's head; markovian lists variant A alone, at shapes whose last feature map is >= 4")
_ap.add_argument("--conditional", action="store_true",
                 help="variant A as the conditional (pix2pix) discriminator, listed alone: conv1 over two input planes")
_ap.add_argument("--net", default="discriminator", choices=("discriminator", "generator"),
                 help="generator lists the CasNet generator's plans alone (the other options do not apply to it)")
_ap.add_argument("--digest", action="store_true", help="one line per program: its call count and the sha256 of its lines")
_ap.add_argument("--tree", default=HERE, help="a built checkout to import the package from")
ARGS = _ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))

import torch  # noqa: E402
from mpgan_amd import engine  # noqa: E402
from mpgan_amd.networks import CasNetGenerator, Discriminator, PatchDiscriminator  # noqa: E402

DEV = "cuda"
# the default keeps the constructor call and the titles of the commits before the option existed (--tree)
HEAD_KW = {} if ARGS.head == "linear" else {"head": ARGS.head}
HEAD_TAG = "" if ARGS.head == "linear" else f" {ARGS.head}"
if ARGS.conditional:
    HEAD_KW["conditional"] = True
    HEAD_TAG += " conditional"


class Ordinals(dict):
    def __call__(self, ptr):
        return "None" if ptr is None else self.setdefault(ptr, f"p{len(self)}")


def _is_ptr(ctype):
    return ctype is C.c_void_p or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))


def _value(v, ctype, ords):
    if isinstance(v, C.Structure):
        return "{" + " ".join(f"{n}={_value(getattr(v, n), t, ords)}" for n, t in v._fields_) + "}"
    if isinstance(v, C.Array):
        return "[" + ",".join(str(x) for x in v) + "]"
    if hasattr(v, "_obj"):                                   # C.byref(structure)
        return _value(v._obj, None, ords)
    if v is None or (isinstance(v, int) and _is_ptr(ctype)):
        return ords(v)
    return repr(v)


def dump(title, prog, ords):
    lines = []
    for i, (fn, args) in enumerate(prog.calls):
        if fn is None:                                       # stream bookkeeping (join / mark / wait)
            entry, shown = args[0], []
        else:
            entry = fn.__name__
            types = getattr(fn, "argtypes", None) or [None] * len(args)
            shown = [_value(a, t, ords) for a, t in zip(args, types)]
        lines.append(f"{i:3d} {prog.names[i]} | {prog.descs[i]} | {prog.tags[i]} | lane{prog.lanes[i]} | {entry}({', '.join(shown)})")
    if ARGS.digest:
        print(f"== {title}: {len(prog)} calls, sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")
    else:
        print("\n".join([f"== {title}: {len(prog)} calls"] + lines))


def variant_a(shape, n):
    """Train forward / backward and the eval forward; under MPGAN_FUSE_BWD_STATS_BF16 the train pair alone, and only if a
    backward-data launch of this shape leaves fused norm-backward rows (returns whether it does)."""
    torch.manual_seed(0)
    d = Discriminator((1,) + shape, dimensions=len(shape), device=DEV, storage_dtype="bf16", **HEAD_KW)
    store, ords, name = d.store, Ordinals(), f"A bf16{HEAD_TAG} {'x'.join(map(str, shape))} n{n}"
    train = engine.DiscPlanBF16(d, store, n, shape, want_backward=True, want_input_grad=True, want_param_grads=True)
    if engine._FUSE_BWD_STATS_BF16:
        L = engine.lib()
        rows = [int(L.mpgan_conv_bwd_stats_rows_bf16(args[0])) for fn, args in train.bwd.calls
                if fn in (L.mpgan_conv_backward_data_bf16, L.mpgan_conv_backward_data_stats_bf16)]
        print(f"# {name}: mpgan_conv_bwd_stats_rows_bf16 of the backward-data launches (layers 3, 2, 1) = {rows}")
        if max(rows) <= 0:
            return False
    dump(f"{name} train fwd", train.fwd, ords)
    dump(f"{name} train bwd", train.bwd, ords)
    if not engine._FUSE_BWD_STATS_BF16:
        ev = engine.DiscPlanBF16(d, store, n, shape, want_backward=False, want_input_grad=False, want_param_grads=False,
                                 training=False)
        dump(f"{name} eval fwd", ev.fwd, Ordinals())
    return True


def variant_b(shape, n):
    torch.manual_seed(0)
    d = PatchDiscriminator((1,) + shape, dimensions=len(shape), patch=shape[0], device=DEV, storage_dtype="bf16")
    store, ords, name = d.store, Ordinals(), f"B bf16 {'x'.join(map(str, shape))} n{n}"
    kw = dict(want_backward=True, want_input_grad=True, want_param_grads=True)
    plan, peer = engine.PatchDiscPlanBF16(d, store, n, shape, **kw), engine.PatchDiscPlanBF16(d, store, n, shape, **kw)
    dump(f"{name} train fwd", plan.fwd, ords)
    dump(f"{name} backward_program(None)", plan.backward_program(None), ords)
    dump(f"{name} backward_program(peer)", plan.backward_program(peer), ords)
    for keep in (True, False):
        ev = engine.PatchDiscPlanBF16(d, store, n, shape, want_backward=False, want_input_grad=False,
                                      want_param_grads=False, training=False, keep_taps=keep)
        dump(f"{name} eval fwd keep_taps={keep}", ev.fwd, Ordinals())


def variant_a_f32(shape, n):
    """Train forward / backward with all gradients and as the G step takes them (input gradient only), and the eval
    forward; under MPGAN_DBG_NO_FUSE_BWD_STATS the all-gradients train pair alone."""
    torch.manual_seed(0)
    d = Discriminator((1,) + shape, dimensions=len(shape), device=DEV, **HEAD_KW)
    store, name = d.store, f"A f32{HEAD_TAG} {'x'.join(map(str, shape))} n{n}"
    steps = [("train", dict(want_input_grad=True, want_param_grads=True))]
    if engine._FUSE_BWD_STATS:
        steps.append(("G-step train", dict(want_input_grad=True, want_param_grads=False)))
    for what, kw in steps:
        plan, ords = engine.DiscPlan(d, store, n, shape, want_backward=True, **kw), Ordinals()
        dump(f"{name} {what} fwd", plan.fwd, ords)
        dump(f"{name} {what} bwd", plan.bwd, ords)
    if engine._FUSE_BWD_STATS:
        ev = engine.DiscPlan(d, store, n, shape, want_backward=False, want_input_grad=False, want_param_grads=False,
                             training=False)
        dump(f"{name} eval fwd", ev.fwd, Ordinals())


def variant_b_f32(shape, n):
    torch.manual_seed(0)
    d = PatchDiscriminator((1,) + shape, dimensions=len(shape), patch=shape[0], device=DEV)
    store, ords, name = d.store, Ordinals(), f"B f32 {'x'.join(map(str, shape))} n{n}"
    kw = dict(want_backward=True, want_input_grad=True, want_param_grads=True)
    plan, peer = engine.PatchDiscPlan(d, store, n, shape, **kw), engine.PatchDiscPlan(d, store, n, shape, **kw)
    dump(f"{name} train fwd", plan.fwd, ords)
    dump(f"{name} backward_program(None)", plan.backward_program(None), ords)
    dump(f"{name} backward_program(peer)", plan.backward_program(peer), ords)
    plan._ext_buffers()
    dump(f"{name} backward_program_ext(None)", plan.backward_program_ext(None), ords)
    dump(f"{name} backward_program_ext(peer)", plan.backward_program_ext(peer), ords)
    for keep in (True, False):
        ev = engine.PatchDiscPlan(d, store, n, shape, want_backward=False, want_input_grad=False, want_param_grads=False,
                                  training=False, keep_taps=keep)
        dump(f"{name} eval fwd keep_taps={keep}", ev.fwd, Ordinals())


# Three U-Nets each, so that the wait_mark rotation of the two gradient scratch sets (u + 2 < nU) appears.
# (title, spatial, n, CasNetGenerator keywords, GeneratorPlan keywords)
_TRAIN = dict(want_backward=True, want_input_grad=True, training=True)
_EVAL = dict(want_backward=False, want_input_grad=False, training=False)
GENERATOR_CASES = [
    ("train", (32, 32), 2, {}, _TRAIN),
    ("train no input grad", (32, 32), 2, {}, dict(_TRAIN, want_input_grad=False)),
    ("eval", (32, 32), 2, {}, _EVAL),                                         # BatchNorm: the fused-epilogue path
    ("train", (16, 16, 16), 2, {}, _TRAIN),
    ("train instance", (16, 16, 16), 2, dict(norm="instance"), _TRAIN),
    ("train mm_bf16", (16, 16, 16), 2, dict(matmul_dtype="bf16"), _TRAIN),
    ("eval instance", (16, 16, 16), 1, dict(norm="instance"), _EVAL),         # the non-fused eval path
    ("train identity bottom", (16, 24), 2, dict(channels=(8, 16, 16), strides=(2, 2)), _TRAIN),
    ("train variant B", (16, 16, 16), 1, dict(channels=(32, 64, 128, 256), strides=(2, 2, 2, 2)), _TRAIN),
]


def generator(what, shape, n, gen_kw, plan_kw):
    """One GeneratorPlan of a fresh 3-U-Net generator, through its constructor and `fwd` / `bwd` alone."""
    torch.manual_seed(0)
    gen = CasNetGenerator((1,) + shape, 3, dimensions=len(shape), device=DEV, **gen_kw)
    plan = engine.GeneratorPlan(gen, gen.store, n, shape, instance=gen.norm.startswith("instance"),
                                mm_bf16=gen.matmul_dtype == "bf16", **plan_kw)
    ords, name = Ordinals(), f"G {'x'.join(map(str, shape))} n{n} {what}"
    dump(f"{name} fwd", plan.fwd, ords)
    if plan_kw["want_backward"]:
        dump(f"{name} bwd", plan.bwd, ords)


def main():
    if ARGS.net == "generator":
        print(f"# MPGAN_DBG_NO_FUSE_DOWN={int(not engine._FUSE_DOWN)} MPGAN_ACC_STATS={int(engine._ACC_STATS)}")
        for case in GENERATOR_CASES:
            generator(*case)
        return
    bf16, f32 = ARGS.storage in ("bf16", "both"), ARGS.storage in ("f32", "both")
    if ARGS.head == "markovian" or ARGS.conditional:         # (24^3 ends in a 3^3 feature map: 32^3 here)
        for fn in ([variant_a] if bf16 else []) + ([variant_a_f32] if f32 else []):
            fn((40, 40), 3)
            fn((32, 32, 32), 2)
        return
    if engine._FUSE_BWD_STATS_BF16:                          # the second invocation: the first shape with fused rows
        print("# MPGAN_FUSE_BWD_STATS_BF16=1")
        if bf16 and not (variant_a((40, 40), 3) or variant_a((24, 24, 24), 2)):
            print("# neither small shape has fused rows: 3-D size 48, n 1")
            variant_a((48, 48, 48), 1)
        return
    if not engine._FUSE_BWD_STATS:                           # the third: fp32 variant A with the separate reduce passes
        print("# MPGAN_DBG_NO_FUSE_BWD_STATS=1")
        if f32:
            variant_a_f32((40, 40), 3)
            variant_a_f32((24, 24, 24), 2)
        return
    if bf16:
        variant_a((40, 40), 3)
        variant_a((24, 24, 24), 2)
        variant_b((16, 16, 16), 2)
    if f32:
        variant_a_f32((40, 40), 3)
        variant_a_f32((24, 24, 24), 2)
        variant_b_f32((16, 16, 16), 2)


if __name__ == "__main__":
    main()
