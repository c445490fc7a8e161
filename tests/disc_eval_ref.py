"""TEST INFRASTRUCTURE (imported by tests/ only, never by the product path).

CPU restatement of the EVAL-mode discriminators (code/GAN/GAN_final.py:159-209, test_runs/GAN.py:136-198 after `.eval()`)
under the bf16-storage contract: fp32 arithmetic everywhere, with a round-to-nearest-even to bf16 (oracle.bf16_emul.rb)
at exactly the places where the HIP path stores a tensor:
  * packed weights of the three dense convs (the first conv and the Linear head read fp32 weights);
  * fused program (mpgan_conv_forward_act_bf16): a_i = lrelu(acc_i * scale_i + shift_i) from the fp32 accumulator, the
    conv bias folded into shift_i, stored ONCE -- rounded to bf16, the last one kept fp32 for the fp32 head;
  * tap-keeping program: the raw z_i = acc_i + bias_i rounded to bf16, then a_i = lrelu(z_i * scale_i + shift_i) rounded
    again (fp32 for the last one) -- two roundings per layer, as in training.
scale_i = gamma / sqrt(running_var + eps), shift_i = beta - running_mean * scale_i (+ bias * scale_i when folded)."""
import torch
import torch.nn.functional as F

from oracle.bf16_emul import rb


def lrelu(y, slope):
    return torch.where(y > 0, y, y * slope)


def conv_act_ref(x, w, bias, scale, shift, slope, stride=1, padding=0):
    """One fused launch in fp32: lrelu((conv(x, w) + bias) * scale + shift, slope) per channel (slope: float or (C,)),
    evaluated as the kernel does -- the bias folded into the shift, one fma per element.  Also returns z = conv + bias."""
    dims = x.dim() - 2
    conv = F.conv2d if dims == 2 else F.conv3d
    shp = [1, -1] + [1] * dims
    acc = conv(x, w, None, stride=stride, padding=padding)
    b = bias if bias is not None else torch.zeros_like(scale)
    sh = torch.addcmul(shift, b, scale)                               # shift + bias * scale
    y = torch.addcmul(sh.view(shp), acc, scale.view(shp))             # acc * scale + sh
    sl = slope.view(shp) if torch.is_tensor(slope) else slope
    return lrelu(y, sl), acc + b.view(shp)


def eval_affine(bn):
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias.detach() - bn.running_mean * scale


def disc_eval_bf16(disc, x, fused=True, slope=0.2):
    """disc: an oracle.refmodel.Discriminator or PatchDiscriminator (fp32 parameters, running statistics as they are;
    nothing is written).  Returns dict(validity, logit, acts): acts[i] as the HIP path stores them."""
    dims = x.dim() - 2
    conv = F.conv2d if dims == 2 else F.conv3d
    shp = [1, -1] + [1] * dims
    convs = [disc.model_conv[i] for i in (0, 3, 6, 9)]
    bns = [disc.model_conv[i] for i in (1, 4, 7, 10)]
    a, acts = x, []
    with torch.no_grad():
        for i, (cv, bn) in enumerate(zip(convs, bns)):
            w = cv.weight.detach() if i == 0 else rb(cv.weight.detach())
            scale, shift = eval_affine(bn)
            if fused:
                act, _ = conv_act_ref(a, w, cv.bias.detach(), scale, shift, slope, stride=cv.stride)
            else:
                z = rb(conv(a, w, cv.bias.detach(), stride=cv.stride))
                act = lrelu(z * scale.view(shp) + shift.view(shp), slope)
            a = act if i == 3 else rb(act)
            acts.append(a)
        h = a.reshape(a.shape[0], -1)
        for m in list(disc.model_linear)[1:-1]:
            h = m(h)
        return {"validity": torch.sigmoid(h), "logit": h, "acts": acts}
