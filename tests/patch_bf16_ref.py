"""TEST INFRASTRUCTURE: CPU restatement of variant B's patch discriminator (test_runs/GAN.py:136-198,288-298) under
the bf16-storage contract of DESIGN.md 3a -- oracle/bf16_emul.py's C5 contract extended to the patch discriminator and
its 16 perceptual taps.  All arithmetic is fp32; a value is rounded to nearest-even bf16 exactly where the HIP path
stores it:
  * packed weights of conv layers 1-3 (layer 0 and the two Linear layers read fp32 weights),
  * every raw conv output z_i (its BatchNorm statistics come from the fp32 values, before the rounding),
  * a_i = LeakyReLU_0.2(BN(z_i)) for i = 0, 1, 2 (a_3 stays fp32: the fp32 split-K head reads it),
  * every activation gradient a backward-data kernel writes and every dz the norm backward writes (the gradient of a_3,
    written by the head's GEMM, stays fp32; so does the crops' gradient).
The taps are defined on the STORED z_i: tap z = z_i, y = z_i*scale + shift, a = LeakyReLU(y), all fp32; h, logit and
prob as the fp32 head computes them.

`pair_step` runs a fake and a real pass of one discriminator and the backward of
    loss = w_perc * perceptual_loss(fake taps, real taps) + BCE(D(fake), target)
with the HIP path's formulas (the norm backward written out, the peer-tap terms of mpgan_peer_taps).  rounding=False
turns every rounding off (then it is the fp32 network, pinned against oracle.refmodel by test_patch_bf16_host.py);
acc64=True lets every convolution accumulate in fp64 and round once to fp32 -- the same contract with another
summation order, the yardstick of bf16_emul.disc_step."""
import torch
import torch.nn.functional as F

from oracle.bf16_emul import rb


def _ident(t):
    return t


def _conv_fns(dims, acc64):
    conv_ = F.conv2d if dims == 2 else F.conv3d
    if acc64:
        def conv(a, w, b):
            return conv_(a.double(), w.double(), None if b is None else b.double()).float()
    else:
        def conv(a, w, b):
            return conv_(a, w, b)

    def conv_bwd(a_in, w, dz):
        """(data gradient, weight gradient) of the pad-free stride-1 conv at (a_in, w) for the output gradient dz."""
        a_req = (a_in.double() if acc64 else a_in).clone().requires_grad_(True)
        w_req = (w.double() if acc64 else w).clone().requires_grad_(True)
        out = conv_(a_req, w_req, None)
        ga, gw = torch.autograd.grad(out, (a_req, w_req), dz.double() if acc64 else dz)
        return ga.float(), gw.float()
    return conv, conv_bwd


def forward(disc, x, *, rounding=True, acc64=False, eps=1e-5, slope=0.2):
    """One training-mode pass of an oracle.refmodel.PatchDiscriminator (BatchNorm running statistics are left alone)."""
    R = rb if rounding else _ident
    dims = x.dim() - 2
    conv, _ = _conv_fns(dims, acc64)
    convs = [disc.model_conv[i] for i in (0, 3, 6, 9)]
    bns = [disc.model_conv[i] for i in (1, 4, 7, 10)]
    lin1, lin2 = disc.model_linear[1], disc.model_linear[2]
    red = [0] + list(range(2, 2 + dims))
    shp = [1, -1] + [1] * dims
    a, layers = x, []
    for i, (cv, bn) in enumerate(zip(convs, bns)):
        w = cv.weight.detach() if i == 0 else R(cv.weight.detach())
        z32 = conv(a, w, cv.bias.detach())
        mean = z32.mean(red)
        var = z32.var(red, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + eps)
        scale = bn.weight.detach() * invstd
        shift = bn.bias.detach() - mean * scale
        z = R(z32)
        y = z * scale.view(shp) + shift.view(shp)
        act = torch.where(y < 0, y * slope, y)
        layers.append(dict(a_in=a, w=w, z=z, y=y, act=act, mean=mean, invstd=invstd, scale=scale, shift=shift))
        a = act if i == 3 else R(act)
    n = x.shape[0]
    h = a.reshape(n, -1) @ lin1.weight.detach().t() + lin1.bias.detach()
    logit = h @ lin2.weight.detach().t() + lin2.bias.detach()
    prob = torch.sigmoid(logit)
    taps = {}
    for i, L in enumerate(layers):
        taps[3 * i], taps[3 * i + 1], taps[3 * i + 2] = L["z"], L["y"], L["act"]
    taps[12], taps[13], taps[14], taps[15] = layers[3]["act"].flatten(1), h, logit, prob
    return dict(layers=layers, a3=a, h=h, logit=logit, prob=prob, taps=taps, dims=dims)


def perceptual(taps_fake, taps_real):
    """test_runs/GAN.py:288-298: sum_k L1mean(real_k, fake_k) / numel_k (fp64 sum of fp32 terms), shape (1,)."""
    s = torch.zeros(1, dtype=torch.float64)
    for k in range(16):
        s = s + (taps_real[k].double() - taps_fake[k].double()).abs().mean() / taps_real[k].numel()
    return s.float()


def norm_bwd_peer(g, z, scale, shift, mean, invstd, slope=0.2, peer=None, coef=(0.0, 0.0, 0.0)):
    """The norm backward of the HIP path on given tensors (NC(D)HW, any float dtype; computed in the dtype of g):
    returns (dz before its bf16 rounding, sum gy, sum gy*zhat).  peer = (z_peer, scale_peer, shift_peer) adds the
    peer-tap terms g_a = g - c_a*sign(a_peer - a), gy = g_a*act'(y) - c_y*sign(y_peer - y), dz += -c_z*sign(z_peer - z)."""
    dims = z.dim() - 2
    red = [0] + list(range(2, 2 + dims))
    shp = [1, -1] + [1] * dims
    dt = g.dtype
    z, scale, shift, mean, invstd = (t.to(dt) for t in (z, scale, shift, mean, invstd))
    y = z * scale.view(shp) + shift.view(shp)
    cz, cy, ca = coef
    ga, gy_extra, dz_extra = g, 0.0, 0.0
    if peer is not None:
        zp, sp, hp = (t.to(dt) for t in peer)
        yp = zp * sp.view(shp) + hp.view(shp)
        ap = torch.where(yp < 0, yp * slope, yp)
        a = torch.where(y < 0, y * slope, y)
        ga = g - ca * torch.sign(ap - a)
        gy_extra = -cy * torch.sign(yp - y)
        dz_extra = -cz * torch.sign(zp - z)
    gy = torch.where(y < 0, ga * slope, ga) + gy_extra
    zh = (z - mean.view(shp)) * invstd.view(shp)
    cnt = z.numel() / z.shape[1]
    s1, s2 = gy.sum(red), (gy * zh).sum(red)
    dz = scale.view(shp) * (gy - (s1 / cnt).view(shp) - zh * (s2 / cnt).view(shp)) + dz_extra
    return dz, s1, s2


def _backward(disc, fw, peer, g_prob, w_perc, grads, *, rounding, acc64, slope=0.2, signs=None):
    """Backward of one pass: g_prob = dLoss/dprob from the BCE (None: no BCE on this pass); peer = the other pass's
    forward (its taps enter through the perceptual term, weight w_perc).  Adds the parameter gradients into `grads`
    and returns the input gradient.  signs: {"h", "logit", "prob"} -> sign(mine - other) to use for the head taps'
    terms instead of this pass's own (teacher forcing of those discrete decisions)."""
    R = rb if rounding else _ident
    _, conv_bwd = _conv_fns(fw["dims"], acc64)
    convs = [disc.model_conv[i] for i in (0, 3, 6, 9)]
    lin1, lin2 = disc.model_linear[1], disc.model_linear[2]
    dims = fw["dims"]
    red = [0] + list(range(2, 2 + dims))
    n = fw["prob"].shape[0]
    add = lambda name, v: grads.__setitem__(name, grads[name] + v if name in grads else v)
    def sg(key):                                                   # d(w * L1mean/numel)/d(mine) of a head tap
        mine, nel = fw[key], fw[key].numel()
        s = torch.sign(mine - peer[key]) if signs is None else signs[key].reshape(mine.shape).to(mine.dtype)
        return s * (w_perc / (nel * nel))
    prob, logit, h, a3 = fw["prob"], fw["logit"], fw["h"], fw["a3"]
    gp = torch.zeros_like(prob) if g_prob is None else g_prob
    if peer is not None:
        gp = gp + sg("prob")
    dlogit = gp * prob * (1 - prob)
    if peer is not None:
        dlogit = dlogit + sg("logit")
    add("model_linear.2.weight", dlogit.t() @ h)
    add("model_linear.2.bias", dlogit.sum(0))
    dh = dlogit @ lin2.weight.detach()
    if peer is not None:
        dh = dh + sg("h")
    add("model_linear.1.weight", dh.t() @ a3.reshape(n, -1))
    add("model_linear.1.bias", dh.sum(0))
    g = (dh @ lin1.weight.detach()).reshape(a3.shape)              # fp32: the gradient of the fp32 a_3
    for i in range(3, -1, -1):
        L = fw["layers"][i]
        nel = float(L["z"].numel())
        last = 2.0 if i == 3 else 1.0
        coef = (w_perc / (nel * nel), w_perc / (nel * nel), last * w_perc / (nel * nel))
        P = peer["layers"][i] if peer is not None else None
        dz, s1, s2 = norm_bwd_peer(g, L["z"], L["scale"], L["shift"], L["mean"], L["invstd"], slope,
                                   None if P is None else (P["z"], P["scale"], P["shift"]), coef)
        add(f"model_conv.{3 * i + 1}.weight", s2)
        add(f"model_conv.{3 * i + 1}.bias", s1)
        dz = R(dz)
        add(f"model_conv.{3 * i}.bias", dz.sum(red))
        ga, gw = conv_bwd(L["a_in"], L["w"], dz)
        add(f"model_conv.{3 * i}.weight", gw)
        g = ga if i == 0 else R(ga)
    return g


def pair_step(disc, x_fake, x_real, *, w_perc=1e6, target=1.0, rounding=True, acc64=False, head_signs=None):
    """Fake and real passes of an oracle.refmodel.PatchDiscriminator and the backward of
    w_perc * perceptual(fake, real) + BCE(D(fake), target) through both passes.  Returns validity (of the fake pass),
    the 16 taps of each pass, the perceptual value, the BCE, the loss, the stored z_i of each pass, the parameter
    gradients (both passes summed) and the two input gradients.  head_signs: {"h", "logit", "prob"} -> sign(fake - real)
    of another implementation's head outputs, used for the head taps' gradient terms of both passes."""
    ff = forward(disc, x_fake, rounding=rounding, acc64=acc64)
    fr = forward(disc, x_real, rounding=rounding, acc64=acc64)
    prob = ff["prob"]
    t = torch.full_like(prob, target)
    bce = F.binary_cross_entropy(prob, t)
    perc = perceptual(ff["taps"], fr["taps"])
    # torch's BCE backward: (p - t) / max((1-p) p, 1e-12) / n
    g_prob = (prob - t) / torch.clamp((1 - prob) * prob, min=1e-12) / prob.numel()
    grads = {}
    neg = None if head_signs is None else {k: -v for k, v in head_signs.items()}
    gx_fake = _backward(disc, ff, fr, g_prob, w_perc, grads, rounding=rounding, acc64=acc64, signs=head_signs)
    gx_real = _backward(disc, fr, ff, None, w_perc, grads, rounding=rounding, acc64=acc64, signs=neg)
    return dict(validity=prob, taps_fake=ff["taps"], taps_real=fr["taps"], perceptual=perc, bce=bce,
                loss=w_perc * perc.double() + bce.double(), zs_fake=[L["z"] for L in ff["layers"]],
                zs_real=[L["z"] for L in fr["layers"]], grads=grads, grad_x_fake=gx_fake, grad_x_real=gx_real)


def bce_step(disc, x, target, weight=1.0, *, rounding=True, acc64=False, grads=None):
    """One pass and the backward of weight * BCE(D(x), target) (the D step's halves, test_runs/GAN.py:393-438).
    Adds the parameter gradients into `grads` (a new dict when None); returns (validity, bce, input gradient, grads)."""
    fw = forward(disc, x, rounding=rounding, acc64=acc64)
    prob = fw["prob"]
    t = torch.full_like(prob, target)
    bce = F.binary_cross_entropy(prob, t)
    g_prob = weight * (prob - t) / torch.clamp((1 - prob) * prob, min=1e-12) / prob.numel()
    grads = {} if grads is None else grads
    gx = _backward(disc, fw, None, g_prob, 0.0, grads, rounding=rounding, acc64=acc64)
    return prob, bce, gx, grads
