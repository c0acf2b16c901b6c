"""Host-side helpers of the precision="f16" tests of the LoFTR ResNet-FPN (test_loftr_f16_cpu.py, test_gpu_conv_f16_routes.py,
test_gpu_loftr_f16.py).

`backbone_emul` is ResNetFPN_8_2 in fp64 with the roundings the plain-f16 mode promises and nothing else: every folded filter is
f16(w * 256) / 256, and every tensor a convolution reads — the image, each block's intermediate, output and 1 x 1 shortcut, the
two merged FPN maps and the two maps after the LeakyReLU — is f16(v * 8) / 8, rounded once where it is produced.  The three maps
the mode keeps in fp32 (x3_out, x2_out, x1_out) are not rounded.  With `rounding=False` it is the plain network on the folded
fp64 filters (test_loftr_f16_cpu.py holds that to torch's fp64 conv2d chain with separate BatchNorm).  It also reports whether a
value left the f16 range on the way: the CPU twin of the range flag."""
import torch
import torch.nn.functional as F

ACT, WSC = 8.0, 256.0          # POPE_PLANES_ACT_SCALE, POPE_PLANES_W_SCALE
F16_MAX = 65504.0


def up64(v):
    return (v + 63) // 64 * 64


class Emul:
    def __init__(self, rounding):
        self.rounding = rounding
        self.range_event = False

    def _r(self, v, scale):
        if not self.rounding:
            return v
        s = v * scale
        if not bool(torch.isfinite(s).all()) or float(s.abs().max()) >= F16_MAX:
            self.range_event = True
        return s.to(torch.float16).double() / scale     # fp64 -> f16: one rounding

    def act(self, v):
        return self._r(v, ACT)

    def w(self, v):
        return self._r(v, WSC)


def _fold(conv_w, sd, bn, eps):
    """conv -> BatchNorm(eval) `bn` (a key prefix, or None) as one filter and bias, in the dtype of `sd`."""
    if bn is None:
        return conv_w, None
    g = sd[bn + ".weight"] * torch.rsqrt(sd[bn + ".running_var"] + eps)
    return conv_w * g.view(-1, 1, 1, 1), sd[bn + ".bias"] - sd[bn + ".running_mean"] * g


def backbone_emul(sd, x, rounding=True, eps=1e-5):
    """sd: the backbone's state dict (keys without the 'backbone.' prefix), any float dtype; x [n, 1, H, W].  Returns
    (x3_out [n, 256, H/8, W/8], x1_out [n, 128, H/2, W/2], range_event) in fp64.  With rounding the BatchNorm is folded in fp32, as
    the module does it, before the filter is rounded to f16."""
    e = Emul(rounding)
    fold_dtype = torch.float32 if rounding else torch.float64
    sdf = {k: v.to(fold_dtype) for k, v in sd.items() if v.is_floating_point()}

    def conv(inp, wkey, bnkey, stride, pad):
        w, b = _fold(sdf[wkey + ".weight"], sdf, bnkey, eps)
        return F.conv2d(inp, e.w(w.double()), None if b is None else b.double(), stride, pad)

    def block(inp, p, stride):
        t = e.act(F.relu(conv(inp, p + ".conv1", p + ".bn1", stride, 1)))
        y = conv(t, p + ".conv2", p + ".bn2", 1, 1)
        s = inp if stride == 1 else e.act(conv(inp, p + ".downsample.0", p + ".downsample.1", stride, 0))
        return e.act(F.relu(y + s))

    up = lambda t: F.interpolate(t, scale_factor=2.0, mode="bilinear", align_corners=True)
    x0 = e.act(F.relu(conv(e.act(x.double()), "conv1", "bn1", 2, 3)))
    x1 = block(block(x0, "layer1.0", 1), "layer1.1", 1)
    x2 = block(block(x1, "layer2.0", 2), "layer2.1", 1)
    x3 = block(block(x2, "layer3.0", 2), "layer3.1", 1)
    x3_out = conv(x3, "layer3_outconv", None, 1, 0)
    m2 = e.act(conv(x2, "layer2_outconv", None, 1, 0) + up(x3_out))
    t2 = e.act(F.leaky_relu(conv(m2, "layer2_outconv2.0", "layer2_outconv2.1", 1, 1), 0.01))
    x2_out = conv(t2, "layer2_outconv2.3", None, 1, 1)
    m1 = e.act(conv(x1, "layer1_outconv", None, 1, 0) + up(x2_out))
    t1 = e.act(F.leaky_relu(conv(m1, "layer1_outconv2.0", "layer1_outconv2.1", 1, 1), 0.01))
    x1_out = conv(t1, "layer1_outconv2.3", None, 1, 1)
    return x3_out, x1_out, e.range_event


def errors(a, b):
    """(max |a - b|, rms(a - b)) in fp64."""
    d = a.double() - b.double()
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())
