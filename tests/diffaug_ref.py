"""Float64 restatement of the differentiable augmentation (include/mpgan_hip.h), index-based: forward and
closed-form backward, a literal port of the paper's 2-D translation and cutout arithmetic, and the shape and parameter
tables the tests share.  No GPU, nothing of the library.

    u[q]    = c (x[q] - m) + m + b
    keep(p) = inside(p + t) and not (lo_k <= p_k < lo_k + size_k for every axis k)
    y[p]    = keep(p) ? u[p + t] : fill
    g_u[q]  = inside(q - t) and keep(q - t) ? g_y[q - t] : 0
    g_x[q]  = c g_u[q] + (1 - c) / N * sum g_u
"""
import torch

BRIGHTNESS, CONTRAST, TRANSLATION, CUTOUT = 1, 2, 4, 8
COLOR, ALL = 3, 15

SHAPES_2D = [(1, 1, 5, 7), (3, 1, 8, 8), (2, 1, 33, 65)]
SHAPES_3D = [(2, 1, 4, 5, 6), (1, 1, 9, 16, 17), (2, 1, 16, 16, 16), (2, 1, 20, 33, 35)]
SHAPES = SHAPES_2D + SHAPES_3D
OPS_SPATIAL = [TRANSLATION, CUTOUT, TRANSLATION | CUTOUT]
OPS_COLOR = [BRIGHTNESS, CONTRAST, COLOR, COLOR | TRANSLATION, COLOR | CUTOUT, ALL]


def dhw(shape):
    s = tuple(shape[2:])
    return (1,) * (3 - len(s)) + s


def _r(s):
    return int(s / 8 + 0.5)


def hand_rows(shape):
    """Hand-made (b, c, geom row) triples for one sample of `shape`: t = 0, +-r, +-S (all fill), mixed signs; boxes with
    lo < 0, past the far edge, size 0, covering everything; c in {0.5, 1, the largest float below 1.5}, b = +-0.5."""
    D, H, W = dhw(shape)
    S = (D, H, W)
    two_d = len(shape) == 4
    r = tuple(0 if (two_d and k == 0) else _r(s) for k, s in enumerate(S))
    half = tuple(int(s / 2 + 0.5) for s in S)
    c_hi = float(torch.nextafter(torch.tensor(1.5, dtype=torch.float32), torch.tensor(0.0, dtype=torch.float32)))

    def g(t, lo, size):
        if two_d:                                   # the D entries of a 2-D row are 0, 0, 1
            t, lo, size = (0,) + tuple(t[1:]), (0,) + tuple(lo[1:]), (1,) + tuple(size[1:])
        return tuple(t) + tuple(lo) + tuple(size)

    zero = (0, 0, 0)
    rows = [
        (0.0, 1.0, g(zero, zero, zero)),                                             # identity
        (0.5, 0.5, g(r, tuple(-(h // 2) for h in half), half)),                      # t = +r, box with lo < 0
        (-0.5, c_hi, g(tuple(-v for v in r), tuple(s - h // 2 for s, h in zip(S, half)), half)),   # t = -r, past the far edge
        (0.25, 1.0, g((r[0], -r[1], r[2]), (0, 1, 2), (1, 2, 3))),                   # mixed signs, a small inner box
        (-0.25, 0.75, g((-r[0], r[1], -r[2]), (1, 0, 1), S)),                        # ... a box past every far edge
        (0.5, 1.25, g(S, zero, zero)),                                               # t = +S: all fill
        (-0.5, 0.5, g(tuple(-s for s in S), zero, half)),                            # t = -S: all fill
        (0.125, c_hi, g((0, 1, -1), tuple(-s for s in S), tuple(3 * s for s in S))),  # a box covering everything
        (0.0, 1.0, g((0, 0, W), zero, zero)),                                        # one axis shifted out: all fill
        (0.375, 0.875, g((0, -1, 3), (0, 2, 1), (D, 1, W))),                         # w shift that is no multiple of 4
    ]
    return rows


def param_sets(shape, seed=0):
    """[(name, color (B, 2) float32, geom (B, 9) int32)]: hand-made rows dealt over the batch so that the samples of one
    batch differ, then sampled sets (the paper's formulas, restated here with a seeded CPU generator)."""
    B = shape[0]
    rows = hand_rows(shape)
    sets = []
    for start in range(0, len(rows), B):
        pick = [rows[(start + i) % len(rows)] for i in range(B)]
        color = torch.tensor([[b, c] for b, c, _ in pick], dtype=torch.float32)
        geom = torch.tensor([g for _, _, g in pick], dtype=torch.int32)
        sets.append((f"hand{start}", color, geom))
    gen = torch.Generator().manual_seed(1000 + seed)
    S = dhw(shape)
    two_d = len(shape) == 4
    for i in range(2):
        color = torch.rand(B, 2, generator=gen) + torch.tensor([-0.5, 0.5])
        cols = []
        for k, s in enumerate(S):
            r = 0 if (two_d and k == 0) else _r(s)
            cols.append(torch.randint(-r, r + 1, (B,), generator=gen))
        sizes = [1 if (two_d and k == 0) else int(s / 2 + 0.5) for k, s in enumerate(S)]
        los = []
        for k, s in enumerate(S):
            if two_d and k == 0:
                los.append(torch.zeros(B, dtype=torch.int64))
            else:
                los.append(torch.randint(0, s + (1 - sizes[k] % 2), (B,), generator=gen) - sizes[k] // 2)
        cols += los + [torch.full((B,), z) for z in sizes]
        sets.append((f"sampled{i}", color.float(), torch.stack(cols, 1).to(torch.int32)))
    return sets


def make_input(shape, seed=0, offset=0.3):
    """fp32 values with a mean away from zero (the contrast op's m matters)."""
    gen = torch.Generator().manual_seed(77 + seed)
    return (torch.rand(*shape, generator=gen) * 2 - 1 + offset).float()


# ---- the restatement ------------------------------------------------------------------------------------------------
def _sample_maps(S, row, ops):
    """keep (D, H, W) bool and the source index arrays (clamped into range; meaningful where keep)."""
    t = row[0:3] if ops & TRANSLATION else (0, 0, 0)
    lo, size = (row[3:6], row[6:9]) if ops & CUTOUT else ((0, 0, 0), (0, 0, 0))
    idx, inside, inbox = [], [], []
    for k in range(3):
        p = torch.arange(S[k])
        src = p + int(t[k])
        inside.append((src >= 0) & (src < S[k]))
        idx.append(src.clamp(0, S[k] - 1))
        inbox.append((p >= int(lo[k])) & (p < int(lo[k]) + int(size[k])))
    ins = inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
    box = inbox[0][:, None, None] & inbox[1][None, :, None] & inbox[2][None, None, :]
    return ins & ~box, idx


def color_terms(x64, color, ops):
    """(b, c, m) per sample as (B, 1, 1, 1) float64: the fp32 table values, exact in float64; m the float64 mean."""
    B = x64.shape[0]
    col = color.double()
    b = col[:, 0] if ops & BRIGHTNESS else torch.zeros(B, dtype=torch.float64)
    c = col[:, 1] if ops & CONTRAST else torch.ones(B, dtype=torch.float64)
    m = x64.reshape(B, -1).mean(1) if ops & CONTRAST else torch.zeros(B, dtype=torch.float64)
    v = (B,) + (1,) * (x64.dim() - 1)
    return b.view(v), c.view(v), m.view(v)


def forward(x, color, geom, ops, fill=0.0):
    """y in float64 of x (any float dtype; taken to float64) under the tables; differentiable in x (torch ops only)."""
    x64 = x.double()
    S = dhw(x.shape)
    b, c, m = color_terms(x64, color, ops)
    u = c * (x64 - m) + m + b if ops & COLOR else x64
    u = u.reshape(x.shape[0], *S)
    out = []
    for s in range(x.shape[0]):
        keep, idx = _sample_maps(S, geom[s].tolist(), ops)
        moved = u[s][idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]
        out.append(torch.where(keep, moved, torch.full_like(moved, float(fill))))
    return torch.stack(out).reshape(x.shape)


def gathered_grad(gy, geom, ops):
    """g_u in float64: g_y moved back by t where keep, zero elsewhere."""
    g64 = gy.double()
    S = dhw(gy.shape)
    g64 = g64.reshape(gy.shape[0], *S)
    out = []
    for s in range(gy.shape[0]):
        keep, idx = _sample_maps(S, geom[s].tolist(), ops)
        gu = torch.zeros(S, dtype=torch.float64)
        pd, ph, pw = torch.nonzero(keep, as_tuple=True)
        gu[idx[0][pd], idx[1][ph], idx[2][pw]] = g64[s][pd, ph, pw]      # the shift is injective: no target twice
        out.append(gu)
    return torch.stack(out).reshape(gy.shape)


def backward(gy, color, geom, ops):
    """(g_x, g_u, sum g_u per sample) in float64, closed form."""
    gu = gathered_grad(gy, geom, ops)
    B = gy.shape[0]
    N = gu[0].numel()
    _, c, _ = color_terms(gu, color, ops)
    total = gu.reshape(B, -1).sum(1).view(c.shape)
    gx = c * gu + (1 - c) / N * total if ops & CONTRAST else gu.clone()
    return gx, gu, total


# ---- the paper's arithmetic (DiffAugment_pytorch.py: rand_translation, rand_cutout), with the parameters passed in ----
def paper_translation(x, tx, ty):
    """x (B, C, H, W); tx, ty (B,) integer shifts: pad by one, clamp the shifted grid into the pad, gather."""
    B, _, H, W = x.shape
    translation_x, translation_y = tx.view(B, 1, 1), ty.view(B, 1, 1)
    grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(B, dtype=torch.long), torch.arange(H, dtype=torch.long),
                                                torch.arange(W, dtype=torch.long), indexing="ij")
    grid_x = torch.clamp(grid_x + translation_x + 1, 0, H + 1)
    grid_y = torch.clamp(grid_y + translation_y + 1, 0, W + 1)
    x_pad = torch.nn.functional.pad(x, [1, 1, 1, 1, 0, 0, 0, 0])
    return x_pad.permute(0, 2, 3, 1).contiguous()[grid_batch, grid_x, grid_y].permute(0, 3, 1, 2)


def paper_cutout(x, offset_x, offset_y, cutout_size):
    """x (B, C, H, W); offsets (B,) as the paper draws them (the box centre), cutout_size = (size_x, size_y): the
    box's index grid clamped INTO the image, a mask of zeros there, x * mask."""
    B, _, H, W = x.shape
    grid_batch, grid_x, grid_y = torch.meshgrid(torch.arange(B, dtype=torch.long),
                                                torch.arange(cutout_size[0], dtype=torch.long),
                                                torch.arange(cutout_size[1], dtype=torch.long), indexing="ij")
    grid_x = torch.clamp(grid_x + offset_x.view(B, 1, 1) - cutout_size[0] // 2, min=0, max=H - 1)
    grid_y = torch.clamp(grid_y + offset_y.view(B, 1, 1) - cutout_size[1] // 2, min=0, max=W - 1)
    mask = torch.ones(B, H, W, dtype=x.dtype)
    mask[grid_batch, grid_x, grid_y] = 0
    return x * mask.unsqueeze(1)
