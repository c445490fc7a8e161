"""Every weight-gradient kernel instance against fp64, at small shapes (the table of tests/wgrad_cases.py: at least one
case per instance of csrc/conv_wgrad.hip and of the MM16 half of csrc/conv_mm16.hip that a public entry can reach).

Per case: the operands are laid out as the case says (compact, a channel slice of a wider NaN-filled buffer, a base off
by one float); mpgan_conv_wgrad_kernel_name_at on those very tensors must return the case's label before anything is
launched; then ops.conv_backward_weight / conv_backward_weight_bf16dy / conv2p_backward_weight runs in both tiers of
tests/conv_ref.py -- tier X (dyadic operands, bit-exact) and tier R (uniform operands, the L = M + 2 + (2 if pro) + 1
budget and the fp32 yardstick) -- each with beta = 0 into NaN-filled dw / dbias and with beta = 1 onto dyadic contents,
on a NaN-filled workspace of exactly the queried size whose guard region must stay bit-unchanged.  The last test asserts
that the labels run are the library's whole symbol set but for the proven-unreachable instances."""
import pytest
import torch

import wgrad_cases as W

pytestmark = pytest.mark.gpu

RAN = set()
GUARD = 64                 # floats on either side of dw / dbias and behind the workspace
SENTINEL = 0x5A5A1234      # the guards' bit pattern
NAN = float("nan")


def _guarded(numel, fill):
    """(base, view): `numel` floats filled with `fill` between two guard regions."""
    base = torch.empty(numel + 2 * GUARD, dtype=torch.int32, device="cuda").fill_(SENTINEL).view(torch.float32)
    view = base[GUARD:GUARD + numel]
    view.fill_(fill)
    return base, view


def _guards_intact(base, numel):
    b = base.view(torch.int32)
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + numel:] == SENTINEL).all())


def _place(t, lay, dtype):
    """t (N, D, H, W, C) as a view of pitch lay[0], lay[1] elements into a NaN-filled buffer (16-byte aligned base)."""
    n, d, h, w, c = t.shape
    ld, off = lay[0] or c, lay[1]
    numel = n * d * h * w * ld
    base = torch.full((off + numel + 8,), NAN, dtype=dtype, device="cuda")
    assert base.data_ptr() % 16 == 0
    v = base[off:off + numel].as_strided((n, d, h, w, c), (d * h * w * ld, h * w * ld, w * ld, ld, 1))
    v.copy_(t.to(dtype))
    return v


def _vector(t, off):
    base = torch.full((off + t.numel() + 4,), NAN, device="cuda")
    assert base.data_ptr() % 16 == 0
    v = base[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _prologue(c, o):
    from mpgan_amd import ops
    if c.pro is None:
        return None
    leaky = c.pro.startswith("leaky")
    ptr = torch.full((1,), o.slope, device="cuda") if c.pro == "leaky_ptr" else None
    # with a device slope the host field holds another value: the kernel must read the pointer
    return ops.Prologue(_vector(o.scale, c.pro_off[0]), _vector(o.shift, c.pro_off[1]), c.g.cin if c.pro == "nc" else 0,
                        ops.ACT_LEAKY if leaky else ops.ACT_NONE, 0.5 if ptr is not None else o.slope, ptr)


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.id)
def test_instance_against_fp64(c):
    from mpgan_amd import engine, ops
    g = c.g
    two = c.entry.startswith("2p")
    ws_bytes = W.workspace_bytes(c)
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    fails = []
    for tier in ("X", "R"):
        o = W.operands(c, tier)
        ref = W.reference(c, o)
        dy = _place(o.dy, c.dy, torch.bfloat16 if c.bf16_dy else torch.float32)
        if two:
            planes = [o.x[..., i].contiguous().cuda() for i in (0, 1)]
            label = ops.conv2p_wgrad_kernel_name(g, c.bf16_dy)
        else:
            x = _place(o.x, c.x, torch.float32)
            pro = _prologue(c, o)
            label = engine.wgrad_kernel_name_at(g, x, dy, pro)
        assert label == c.label, f"{c.id}: these operands run {label}, the case is about {c.label}"
        for beta in (0.0, 1.0):
            wbase, dw = _guarded(ref.dw.numel(), NAN)
            bbase, db = _guarded(g.cout, NAN)
            if beta:
                dw.copy_(o.old_w.reshape(-1))
                db.copy_(o.old_b)
            dbias = db if c.dbias else None
            sbase, ws = _guarded(ws_bytes // 4, NAN)
            try:
                if two:
                    ops.conv2p_backward_weight(g, planes[0], planes[1], dy, dw, ws, beta=beta, dbias=dbias)
                elif c.bf16_dy:
                    ops.conv_backward_weight_bf16dy(g, x, dy, dw, ws, beta=beta, dbias=dbias)
                else:
                    ops.conv_backward_weight(g, x, dy, dw, ws, pro=pro, beta=beta, dbias=dbias)
                torch.cuda.synchronize()
            except RuntimeError as e:
                if "HIP error" in str(e) or "illegal memory access" in str(e):      # nothing after a device fault means anything
                    pytest.exit(f"{c.id} tier {tier} beta {beta:g} ({label}) faulted the device: {e}", returncode=3)
                raise
            RAN.add(label)
            want = W.with_beta(c, o, ref, beta)
            got_dw, got_db = dw.cpu(), (db.cpu() if c.dbias else None)
            new = W.check(c, tier, got_dw, got_db, want)
            print(f"  [{tier} beta {beta:g}] {c.id:<32} {label:<58} {'ok' if not new else new}")
            fails += [f"beta {beta:g}: {f}" for f in new]
            for what, base, numel in (("dw", wbase, dw.numel()), ("dbias", bbase, g.cout), ("workspace", sbase, ws.numel())):
                if not _guards_intact(base, numel):
                    fails.append(f"{c.id} tier {tier} beta {beta:g}: written outside {what}")
    assert not fails, "\n".join(fails)


def test_every_reachable_instance_ran():
    """Runs last in this file: the labels launched above are the library's symbols, but for the proven-unreachable ones."""
    symbols = W.library_symbols()
    unreachable = set(W.UNREACHABLE)
    assert not (RAN & unreachable), sorted(RAN & unreachable)
    assert RAN | unreachable == symbols, (sorted(symbols - RAN - unreachable), sorted(RAN - symbols))
