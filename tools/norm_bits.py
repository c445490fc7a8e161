"""sha256 of the raw bytes of every output of the normalisation passes' entries (csrc/norm_ops.hip, csrc/norm_bf16.hip)
and of the backward-data launches whose epilogue forms norm-backward sums, inputs from fixed CPU seeds, every output and
partials buffer zeroed before its call (unwritten tails hash alike).  One line per entry and case: the digest runs over
the entry's outputs in the order the line names them.

    python tools/norm_bits.py OUT.txt

The library is whatever MPGAN_LIB_PATH names (unset: the tree's own): run it once per build in a fresh process and
compare the two files line for line (profiles/README.md, r32_norm_bits_*.txt)."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from mpgan_amd import ops  # noqa: E402
from mpgan_amd._lib import check, lib  # noqa: E402
from gpu_helpers import to_cl  # noqa: E402
import test_patch_bf16_gpu as TP  # noqa: E402

BF = torch.bfloat16
groups = {}          # "case entry" -> (sha256 over its outputs' bytes, their names)


def rec(group, output, t):
    t = t.detach().contiguous().cpu()
    h, names = groups.setdefault(group, (hashlib.sha256(), []))
    h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    names.append(f"{output}{list(t.shape)}")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def at_offset(t, off):
    """The CUDA tensor t as a view that starts `off` elements into a fresh allocation (off 1: not 16-byte aligned)."""
    if not off:
        return t
    base = torch.zeros(t.numel() + off, dtype=t.dtype, device="cuda")
    v = base[off:].view(t.shape)
    v.copy_(t)
    return v


# ---- fp32: channel_stats -> norm_finalize[_strided], norm_act_add, the three backward launches -------------------------
FP32_CASES = [(16, (1, 40, 36), 3), (1, (1, 64, 64), 2), (6, (1, 160, 160), 8), (128, (1, 9, 7), 2), (512, (2, 2, 2), 4),
              (8, (1, 300, 280), 8), (4, (1, 256, 256), 72)]


def fp32_case(c, spatial, n, instance, off=0):
    tag = f"fp32 c{c} {spatial} n{n} {'instance' if instance else 'batch'}" + (f" offset{off}" if off else "")
    gen = torch.Generator().manual_seed(31 + c)
    u = lambda *s: torch.rand(*s, generator=gen)
    z = at_offset(to_cl(u(n, c, *spatial) * 3 - 1), off)
    zp = at_offset(to_cl(u(n, c, *spatial) * 3 - 1.5), off)
    r = at_offset(to_cl(u(n, c, *spatial) - 0.5), off)
    g = at_offset(to_cl(u(n, c, *spatial) * 2 - 1), off)
    gamma, beta = (u(c) + 0.5).cuda(), (u(c) - 0.5).cuda()
    s2, t2, ps, pt = (u(c) + 0.5).cuda(), (u(c) - 0.5).cuda(), (u(c) + 0.5).cuda(), (u(c) - 0.5).cuda()
    alpha = torch.tensor([0.25], device="cuda")
    coef = torch.tensor([3e-3, 2e-3, 4e-3], device="cuda")
    P = spatial[0] * spatial[1] * spatial[2]
    chunks, rows, m = ops.stats_chunks(P, c), n * ops.stats_chunks(P, c), (n * c if instance else c)

    partials = zeros((rows + 32) * 2 * c)
    ops.channel_stats(z, partials)
    rec(f"{tag} channel_stats", "partials", partials)
    scale, shift, mean, invstd = (zeros(m) for _ in range(4))
    run = (None, None, None) if instance else (zeros(c), torch.ones(c, device="cuda"), zeros((), dtype=torch.int64))
    ops.norm_finalize(partials, n, chunks, c, P, instance, gamma, beta, 1e-5, 0.1, *run, scale, shift, mean, invstd)
    for k, v in zip(("partials", "scale", "shift", "mean", "invstd"), (partials, scale, shift, mean, invstd)):
        rec(f"{tag} norm_finalize", k, v)
    if not instance:
        for k, v in zip(("running_mean", "running_var", "nbt"), run):
            rec(f"{tag} norm_finalize", k, v)
    W = c + 4                                               # the same rows at a pitch of W channels
    wide = zeros((rows + 32) * 2 * W)
    wide[:rows * 2 * W].view(rows, 2, W)[:, :, :c] = partials[:rows * 2 * c].view(rows, 2, c)
    out = [zeros(m) for _ in range(4)]
    run2 = (None, None, None) if instance else (zeros(c), torch.ones(c, device="cuda"), zeros((), dtype=torch.int64))
    check(lib().mpgan_norm_finalize_strided(wide.data_ptr(), n, chunks, c, W, P, int(instance), gamma.data_ptr(),
                                            beta.data_ptr(), 1e-5, 0.1, *(ops._ptr(t) for t in run2),
                                            *(t.data_ptr() for t in out), stream()), "norm_finalize_strided")
    for k, v in zip(("scale", "shift", "mean", "invstd"), out):
        rec(f"{tag} norm_finalize_strided", k, v)
    if not instance:
        for k, v in zip(("running_mean", "running_var", "nbt"), run2):
            rec(f"{tag} norm_finalize_strided", k, v)

    pro = ops.Prologue(scale, shift, c if instance else 0, ops.ACT_LEAKY, 1.0, alpha)
    pro_r = ops.Prologue(s2, t2, 0, ops.ACT_LEAKY, 0.1)
    for k, (rr, pr, tanh) in {"plain": (None, None, False), "residual": (r, pro_r, False),
                              "residual tanh": (r, pro_r, True), "raw residual": (r, None, False)}.items():
        out = at_offset(zeros(n, *spatial, c), off)
        ops.norm_act_add(z, pro, rr, pr, out, tanh_out=tanh)
        rec(f"{tag} norm_act_add", k, out)
    if not instance and c <= 256:                           # the fold form: accumulators as a conv's epilogue leaves them
        zd = z.double().reshape(-1, c)
        acc = torch.zeros(ops.ACC_REPLICAS, ops.ACC_WORDS, c, dtype=torch.int64, device="cuda")
        acc[0, 0], acc[0, 2] = torch.round(zd.sum(0) * 256).long(), torch.round((zd * zd).sum(0) * 256).long()
        acc[1, 1], acc[1, 3] = 12345, -6789
        bn = torch.nn.BatchNorm2d(c).cuda()
        with torch.no_grad():
            bn.weight.copy_(gamma); bn.bias.copy_(beta)
        vec = [zeros(c) for _ in range(4)]
        fold = ops.make_fold(acc.view(-1), ops.ACC_REPLICAS, c, n * P, bn, *vec)
        out = at_offset(zeros(n, *spatial, c), off)
        ops.norm_act_add_fold(z, ops.Prologue(scale, shift, 0, ops.ACT_LEAKY, 1.0, alpha), fold, r, pro_r, out)
        rec(f"{tag} norm_act_add_fold", "out", out)
        for k, v in zip(("scale", "shift", "mean", "invstd", "running_mean", "running_var", "nbt"),
                        (*vec, bn.running_mean, bn.running_var, bn.num_batches_tracked)):
            rec(f"{tag} norm_act_add_fold", k, v)

    for peer in ((None,) if instance else (None, ops.PeerTaps(zp, ps, pt, coef))):
        ptag = f"{tag} {'peer' if peer else 'no peer'}"
        part = zeros(rows * (3 * c + 1))
        ops.norm_bwd_reduce(g, z, pro, mean, invstd, part, peer)
        rec(f"{ptag} norm_bwd_reduce", "partials", part)
        dgamma, dbeta, dslope, c1, c2 = zeros(c), zeros(c), zeros(1), zeros(m), zeros(m)
        ops.norm_bwd_finalize(part, n, chunks, c, P, instance, dgamma, dbeta, dslope, c1, c2)
        for k, v in zip(("c1", "c2", "dgamma", "dbeta", "dslope"), (c1, c2, dgamma, dbeta, dslope)):
            rec(f"{ptag} norm_bwd_finalize", k, v)
        dz = at_offset(zeros(n, *spatial, c), off)
        ops.norm_bwd_apply(g, z, pro, mean, invstd, c1, c2, dz, peer)
        rec(f"{ptag} norm_bwd_apply", "dz", dz)
        g2 = at_offset(g.clone(), off)
        ops.norm_bwd_apply(g2, z, pro, mean, invstd, c1, c2, g2, peer)                  # dz aliases g
        rec(f"{ptag} norm_bwd_apply", "dz in place", g2)


for case in FP32_CASES:
    for instance in (False, True):
        fp32_case(*case, instance)
fp32_case(16, (1, 40, 36), 3, False, off=1)                # Vec<1> at c % 4 == 0: views offset by one float
fp32_case(16, (1, 40, 36), 3, True, off=1)


# ---- bf16: the norm backward at every NORM_BWD_CASES row x g dtype x peer; norm_act_bf16 -------------------------------
def bf16_norm_bwd(name, g_dtype, with_peer):
    n, c, sp, pitch, bias = TP.NORM_BWD_CASES[name]
    tag = f"bf16 {name} g {g_dtype} {'peer' if with_peer else 'no peer'}"
    z, zp, g, nbv, peer = TP._norm_bwd_inputs(n, c, sp, g_dtype)
    scale, shift, mean, invstd = (t.cuda().contiguous() for t in nbv)
    rows = z.numel() // c
    brow = ops.norm_bwd_rows_bf16(rows, c)
    part = zeros(brow * 4 * c + c)
    gc, zc = TP._pitched(to_cl(g).to(g_dtype), pitch), TP._pitched(to_cl(z).to(BF), pitch)
    pt = None
    if with_peer:
        pt = ops.PeerTapsBF16(TP._pitched(to_cl(peer[0]).to(BF), pitch), peer[1].cuda(), peer[2].cuda(),
                              torch.tensor((3e-3, 2e-3, 4e-3), device="cuda"))
    ops.norm_bwd_reduce_bf16(gc, zc, scale, shift, mean, invstd, 0.2, part, peer=pt)
    rec(f"{tag} reduce", "partials", part)
    dgamma, dbeta, c1, c2 = zeros(c), zeros(c), zeros(c), zeros(c)
    ops.norm_bwd_finalize(part, 1, brow, c, rows, False, dgamma, dbeta, None, c1, c2)
    for k, v in zip(("c1", "c2", "dgamma", "dbeta"), (c1, c2, dgamma, dbeta)):
        rec(f"{tag} finalize", k, v)
    dz = TP._pitched(torch.zeros_like(to_cl(z).to(BF)), pitch)
    bias_part = part[brow * 3 * c + c:] if bias else None
    ops.norm_bwd_apply_bf16(gc, zc, scale, shift, mean, invstd, c1, c2, 0.2, dz, bias_part, peer=pt)
    rec(f"{tag} apply", "dz", dz)
    rec(f"{tag} apply", "partials and bias partials", part)


for name in TP.NORM_BWD_CASES:
    for g_dtype in (BF, torch.float32):
        for with_peer in (False, True):
            bf16_norm_bwd(name, g_dtype, with_peer)

gen = torch.Generator().manual_seed(5)
for n, sp, c in ((2, (6, 7, 5), 64), (3, (14, 14, 14), 128), (1, (1, 1, 3), 8)):
    z = torch.randn(n, *sp, c, generator=gen).to(BF).cuda()
    sc, sh = (torch.rand(c, generator=gen) + 0.5).cuda(), (torch.rand(c, generator=gen) - 0.5).cuda()
    for dt in (BF, torch.float32):
        out = torch.zeros(n, *sp, c, dtype=dt, device="cuda")
        ops.norm_act_bf16(z, sc, sh, 0.2, out)
        rec(f"norm_act_bf16 n{n} {sp} c{c}", f"-> {dt}", out)

# ---- the perceptual tap L1 of both storage types ---------------------------------------------------------------------------
gen = torch.Generator().manual_seed(3)
for n, sp, c in ((2, (6, 7, 5), 64), (3, (14, 14, 14), 128), (2, (1, 9, 11), 6)):
    za, zb = torch.randn(n, *sp, c, generator=gen), torch.randn(n, *sp, c, generator=gen) * 0.7 + 0.1
    sa, sb = (torch.rand(c, generator=gen) + 0.5).cuda(), (torch.rand(c, generator=gen) + 0.5).cuda()
    ha, hb = (torch.rand(c, generator=gen) - 0.5).cuda(), (torch.rand(c, generator=gen) - 0.5).cuda()
    part, out = zeros(ops.tap_l1_partials()), zeros(3)
    ops.tap_l1(za.cuda(), ops.Prologue(sa, ha, 0, ops.ACT_LEAKY, 0.2), zb.cuda(), ops.Prologue(sb, hb, 0, ops.ACT_LEAKY, 0.2),
               part, out)
    rec(f"tap_l1 n{n} {sp} c{c}", "partials", part)
    rec(f"tap_l1 n{n} {sp} c{c}", "out", out)
    if c % 8 == 0:
        part, out = zeros(ops.tap_l1_partials()), zeros(3)
        ops.tap_l1_bf16(za.to(BF).cuda(), sa, ha, zb.to(BF).cuda(), sb, hb, 0.2, part, out)
        rec(f"tap_l1_bf16 n{n} {sp} c{c}", "partials", part)
        rec(f"tap_l1_bf16 n{n} {sp} c{c}", "out", out)

# ---- copy_slice, reduce_partials ---------------------------------------------------------------------------------------------
gen = torch.Generator().manual_seed(8)
for c, lead, width in ((16, 0, 16), (16, 4, 24), (16, 1, 20), (6, 0, 6)):
    src = torch.rand(2, 1, 9, 11, c, generator=gen).cuda()
    for accumulate in (False, True):
        base = (torch.rand(2, 1, 9, 11, width, generator=torch.Generator().manual_seed(c + lead)) if accumulate
                else torch.zeros(2, 1, 9, 11, width)).cuda()
        ops.copy_slice(src, base[..., lead:lead + c], accumulate=accumulate)
        rec(f"copy_slice c{c} lead{lead} width{width}", f"accumulate{int(accumulate)}", base)
for rows, stride, c in ((5, 16, 16), (300, 40, 33), (2048, 8, 8)):
    p = (torch.rand(rows, stride, generator=gen) - 0.3).cuda()
    for beta in (0.0, 1.0):
        out = (torch.rand(c, generator=torch.Generator().manual_seed(rows)) if beta else torch.zeros(c)).cuda()
        ops.reduce_partials(p, rows, stride, c, out, beta)
        rec(f"reduce_partials rows{rows} stride{stride} c{c}", f"beta{beta}", out)

# ---- eval-mode vectors: norm_from_running, its multi form, epi_vectors_multi -------------------------------------------------
gen = torch.Generator().manual_seed(12)
layers, eps = [], 1e-5
for c in (1, 6, 64, 300):
    layers.append([t.cuda() for t in (torch.rand(c, generator=gen) + 0.5, torch.rand(c, generator=gen) - 0.5,
                                      torch.rand(c, generator=gen) - 0.5, torch.rand(c, generator=gen) + 0.1,
                                      torch.rand(c + 8, generator=gen) - 0.5)])
eps_bits = int(torch.tensor(eps, dtype=torch.float32).view(torch.int32).item())
for gamma, beta, rm, rv, _ in layers:
    c = gamma.numel()
    out = [zeros(c) for _ in range(4)]
    check(lib().mpgan_norm_from_running(gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), eps, c,
                                        *(t.data_ptr() for t in out), stream()), "norm_from_running")
    for k, v in zip(("scale", "shift", "mean", "invstd"), out):
        rec(f"norm_from_running c{c}", k, v)
outs = [[zeros(l[0].numel()) for _ in range(4)] for l in layers]
table = torch.tensor([[l[0].data_ptr(), l[1].data_ptr(), l[2].data_ptr(), l[3].data_ptr(), *(t.data_ptr() for t in o),
                       l[0].numel(), eps_bits] for l, o in zip(layers, outs)], dtype=torch.int64).cuda()
check(lib().mpgan_norm_from_running_multi(table.data_ptr(), len(layers), stream()), "norm_from_running_multi")
for l, o in zip(layers, outs):
    for k, v in zip(("scale", "shift", "mean", "invstd"), o):
        rec("norm_from_running_multi", f"c{l[0].numel()} {k}", v)
alpha = torch.tensor([0.3], device="cuda")
outs = [[zeros(l[0].numel() + 8) for _ in range(3)] for l in layers]
table = torch.tensor([[l[0].data_ptr(), l[1].data_ptr(), l[2].data_ptr(), l[3].data_ptr(), l[4].data_ptr(),
                       alpha.data_ptr() if i % 2 == 0 else 0, *(t.data_ptr() for t in o), l[0].numel(), l[0].numel() + 8,
                       eps_bits] for i, (l, o) in enumerate(zip(layers, outs))], dtype=torch.int64).cuda()
check(lib().mpgan_epi_vectors_multi(table.data_ptr(), len(layers), stream()), "epi_vectors_multi")
for l, o in zip(layers, outs):
    for k, v in zip(("scale", "shift", "slope"), o):
        rec("epi_vectors_multi", f"c{l[0].numel()} {k}", v)

# ---- backward-data launches whose epilogue forms the norm-backward sums: the first (smallest) geometry that has them --------
gen = torch.Generator().manual_seed(21)
FUSED_F32 = [(1, (1, 12, 14), 64, 128, 3, 1), (2, (1, 34, 34), 64, 128, 3, 1), (3, (1, 131, 127), 64, 128, 3, 1)]
FUSED_BF16 = [(1, (9, 10, 12), 64, 128, 3, 1), (1, (12, 20, 22), 64, 128, 3, 1), (2, (1, 9, 30), 256, 256, 3, 1)]


def geom(n, sp, cin, cout, k, s):
    kk = tuple(1 if e == 1 else k for e in sp)
    return ops.ConvGeom(n, sp, cin, cout, kk, tuple(1 if e == 1 else s for e in sp), (0, 0, 0), min_blocks=1)


def fused_inputs(g, dtype):
    taps = g.k[0] * g.k[1] * g.k[2]
    w = ((torch.rand(g.cout, g.cin, *g.k, generator=gen) - 0.5) * 0.2).to(dtype).float()
    dy = (torch.rand(g.n, *g.out_dhw, g.cout, generator=gen) - 0.5).to(dtype).cuda()
    z = (torch.rand(g.n, *g.in_dhw, g.cin, generator=gen) * 2 - 1).to(dtype).cuda()
    vec = [t.cuda() for t in (torch.rand(g.cin, generator=gen) + 0.5, torch.rand(g.cin, generator=gen) - 0.5,
                              torch.rand(g.cin, generator=gen) - 0.5, torch.rand(g.cin, generator=gen) + 0.5)]
    return w.cuda(), dy, z, vec


g = next((geom(*q) for q in FUSED_F32 if ops.conv_bwd_stats_rows(geom(*q)) > 0), None)
if g is None:
    rec("conv_backward_data_stats", "no candidate geometry has fused sums", torch.zeros(0))
else:
    rows = ops.conv_bwd_stats_rows(g)
    w, dy, z, vec = fused_inputs(g, torch.float32)
    dx, part = torch.zeros_like(z), zeros(rows * 3 * g.cin)
    ops.conv_backward_data_stats(g, dy, ops.pack_weight(w, for_dgrad=True), dx, z, *vec, ops.ACT_LEAKY, 0.2, part)
    rec(f"conv_backward_data_stats {g.in_dhw} {g.cin}<-{g.cout} rows{rows}", "dx", dx)
    rec(f"conv_backward_data_stats {g.in_dhw} {g.cin}<-{g.cout} rows{rows}", "partials", part)
for q in FUSED_BF16:
    g = geom(*q)
    gc = g.c()
    rows = lib().mpgan_conv_bwd_stats_rows_bf16(C.byref(gc))
    if rows <= 0:
        continue
    w, dy, z, vec = fused_inputs(g, BF)
    dx, part = torch.zeros_like(z), zeros(rows * 3 * g.cin)
    check(lib().mpgan_conv_backward_data_stats_bf16(C.byref(gc), dy.data_ptr(), g.cout, ops.pack_weight_bf16(w, for_dgrad=True).data_ptr(),
                                                    dx.data_ptr(), g.cin, z.data_ptr(), g.cin, *(t.data_ptr() for t in vec), 0.2,
                                                    part.data_ptr(), stream()), "conv_backward_data_stats_bf16")
    rec(f"conv_backward_data_stats_bf16 {g.in_dhw} {g.cin}<-{g.cout} rows{rows}", "dx", dx)
    rec(f"conv_backward_data_stats_bf16 {g.in_dhw} {g.cin}<-{g.cout} rows{rows}", "partials", part)
    break
else:
    rec("conv_backward_data_stats_bf16", "no candidate geometry has fused sums", torch.zeros(0))

torch.cuda.synchronize()
lines = [f"{g}: {', '.join(names)} {h.hexdigest()}" for g, (h, names) in groups.items()]
with open(sys.argv[1], "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"{len(lines)} digests -> {sys.argv[1]} (library: {os.environ.get('MPGAN_LIB_PATH', 'the tree')})")
