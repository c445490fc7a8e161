#!/usr/bin/env python3
"""The frozen launch lists of the bf16-storage discriminator plans, in a form that can be diffed across commits
(development aid: builds the plans, launches nothing).

    python tools/dump_programs.py                                    # variant A and B, every program
    MPGAN_FUSE_BWD_STATS_BF16=1 python tools/dump_programs.py        # variant A train with the fused norm-backward sums

One line per call: index, name, desc, tag, lane, the C entry and its arguments.  Every pointer (an argument or a structure
field the C signature declares as one) is replaced by an ordinal in order of first appearance within its plan (p0, p1,
...), so that the aliasing pattern is compared and the addresses are not; byref structures are expanded field by field.
Needs an MI355X only because the plans allocate their tensors there."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import torch  # noqa: E402
from mpgan_amd import engine  # noqa: E402
from mpgan_amd.networks import Discriminator, PatchDiscriminator  # noqa: E402

DEV = "cuda"


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
    print(f"== {title}: {len(prog)} calls")
    for i, (fn, args) in enumerate(prog.calls):
        if fn is None:                                       # stream bookkeeping (join / mark / wait)
            entry, shown = args[0], []
        else:
            entry = fn.__name__
            types = getattr(fn, "argtypes", None) or [None] * len(args)
            shown = [_value(a, t, ords) for a, t in zip(args, types)]
        print(f"{i:3d} {prog.names[i]} | {prog.descs[i]} | {prog.tags[i]} | lane{prog.lanes[i]} | {entry}({', '.join(shown)})")


def variant_a(shape, n):
    """Train forward / backward and the eval forward; under MPGAN_FUSE_BWD_STATS_BF16 the train pair alone, and only if a
    backward-data launch of this shape leaves fused norm-backward rows (returns whether it does)."""
    torch.manual_seed(0)
    d = Discriminator((1,) + shape, dimensions=len(shape), device=DEV, storage_dtype="bf16")
    store, ords, name = d.store, Ordinals(), f"A bf16 {'x'.join(map(str, shape))} n{n}"
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


def main():
    if engine._FUSE_BWD_STATS_BF16:                          # the second invocation: the first shape with fused rows
        print("# MPGAN_FUSE_BWD_STATS_BF16=1")
        if not (variant_a((40, 40), 3) or variant_a((24, 24, 24), 2)):
            print("# neither small shape has fused rows: 3-D size 48, n 1")
            variant_a((48, 48, 48), 1)
        return
    variant_a((40, 40), 3)
    variant_a((24, 24, 24), 2)
    variant_b((16, 16, 16), 2)


if __name__ == "__main__":
    main()
