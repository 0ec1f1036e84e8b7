"""TEST INFRASTRUCTURE: torchvision 0.13's tensor-path ColorJitter ops (brightness, saturation, hue; `functional_tensor.py`), restated in
plain torch so that they run in fp32 and in fp64.  The reference's train transform applies them to the [T, C, H, W] clip as a whole,
between RandomHorizontalFlip and Normalize (data_loader/transforms.py:16); contrast cannot be set by its configs and is not here.

Images are float RGB in [0, 1] with the channel at dim -3.  `apply(x, row)` runs the ops one row of the draw table
(`egovlp_amd.data_loader.transforms.train_transform_params_color`) names: (brightness factor, saturation factor, hue shift, code), the
code three base-4 digits, first applied op lowest, 0 nothing / 1 brightness / 2 saturation / 3 hue."""
import torch


def blend(a, b, f):
    return (f * a + (1.0 - f) * b).clamp(0.0, 1.0)


def gray(x):
    r, g, b = x.unbind(-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)


def brightness(x, f):
    return blend(x, torch.zeros_like(x), f)


def saturation(x, f):
    return blend(x, gray(x), f)


def rgb2hsv(x):
    r, g, b = x.unbind(-3)
    maxc = x.max(-3).values
    minc = x.min(-3).values
    eq = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eq, ones, maxc)
    div = torch.where(eq, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return torch.stack((h, s, maxc), -3)


def hsv2rgb(x):
    h, s, v = x.unbind(-3)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p = (v * (1.0 - s)).clamp(0.0, 1.0)
    q = (v * (1.0 - s * f)).clamp(0.0, 1.0)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0.0, 1.0)
    mask = i.unsqueeze(-3) == torch.arange(6, device=x.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), -3)
    a2 = torch.stack((t, v, v, q, p, p), -3)
    a3 = torch.stack((p, p, t, v, v, q), -3)
    a4 = torch.stack((a1, a2, a3), -4)                       # [..., 3, 6, H, W]
    return torch.einsum("...ijk,...xijk->...xjk", mask.to(x.dtype), a4)


def hue(x, d):
    hsv = rgb2hsv(x)
    h, s, v = hsv.unbind(-3)
    h = (h + d) % 1.0
    return hsv2rgb(torch.stack((h, s, v), -3))


def ops_of(code):
    """the op digits of a code in the order they are applied"""
    code = int(code)
    return [d for d in ((code >> (2 * k)) & 3 for k in range(3)) if d]


def apply(x, row):
    """x: [..., 3, H, W] in [0, 1]; row: the four numbers of one clip (brightness, saturation, hue, code)"""
    fb, fs, fh, code = (float(v) for v in row)
    for d in ops_of(code):
        x = brightness(x, fb) if d == 1 else saturation(x, fs) if d == 2 else hue(x, fh)
    return x
