"""The colour reference of tests/test_color_*.py, run with Pillow itself: torchvision's
_functional_pil colour ops restated (they are thin wrappers over Pillow) --
adjust_brightness / contrast / saturation = ImageEnhance.Brightness / Contrast / Color (.enhance),
adjust_hue = convert("HSV"), a wrapping uint8 add on H, convert("RGB"),
to_grayscale(3) = convert("L") replicated -- plus the crop / resize / flip / ToTensor / Normalize
chain around them, as tests/test_preprocess_gpu.py replays it."""
import numpy as np
import torch
from PIL import Image, ImageEnhance

from fsp_amd import _native as N
from fsp_amd.data import preprocess as P

BRIGHTNESS, CONTRAST, SATURATION, HUE, GRAYSCALE = (N.COLOR_BRIGHTNESS, N.COLOR_CONTRAST, N.COLOR_SATURATION,
                                                   N.COLOR_HUE, N.COLOR_GRAYSCALE)


def pil_op(im, op, value):
    """One op on a PIL RGB image; value: the blend factor, or the uint8 hue shift."""
    if op == BRIGHTNESS:
        return ImageEnhance.Brightness(im).enhance(value)
    if op == CONTRAST:
        return ImageEnhance.Contrast(im).enhance(value)
    if op == SATURATION:
        return ImageEnhance.Color(im).enhance(value)
    if op == HUE:
        h, s, v = im.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over="ignore"):
            np_h += np.uint8(value)  # wraps modulo 256, as torchvision's in-place uint8 add
        return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    if op == GRAYSCALE:
        g = np.array(im.convert("L"), dtype=np.uint8)
        return Image.fromarray(np.dstack([g, g, g]), "RGB")
    raise ValueError(op)


def pil_program(hwc, program):
    """uint8 [H, W, 3] -> uint8 [H, W, 3] after the program's ops in order."""
    im = Image.fromarray(np.ascontiguousarray(hwc))
    for op, value in program:
        im = pil_op(im, op, value)
    return np.asarray(im)


def planar(hwc_list):
    """list of uint8 [S, S, 3] -> uint8 tensor [B, 3, S, S]"""
    return torch.from_numpy(np.stack([np.transpose(a, (2, 0, 1)) for a in hwc_list]).copy())


def normalize(chw_u8, mean=P.MEAN, std=P.STD):
    """ToTensor + Normalize of torch on a uint8 [..., 3, S, S] tensor."""
    x = chw_u8.float().div(255)
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    return x.sub_(m).div_(s)


def pil_view(img, plan):
    """The reference's transform chain for one image and one drawn plan: crop -> resize(BICUBIC) ->
    flip -> the plan's colour program -> (uint8 [3, S, S], normalised fp32 [3, S, S])."""
    im = Image.fromarray(img)
    if (plan.x0, plan.y0, plan.w, plan.h) != (0, 0) + im.size:
        im = im.crop((plan.x0, plan.y0, plan.x0 + plan.w, plan.y0 + plan.h))
    im = im.resize((plan.rw, plan.rh), Image.BICUBIC)
    im = im.crop((plan.ox, plan.oy, plan.ox + plan.S, plan.oy + plan.S))
    if plan.flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    for op, value in plan.color:
        im = pil_op(im, op, value)
    t = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous()
    return t, normalize(t)


def all_triples(S=224):
    """All 2^24 RGB triples as S x S images: uint8 [B, S, S, 3], the tail padded with zeros."""
    i = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([i >> 16, (i >> 8) & 255, i & 255], -1).astype(np.uint8)
    per = S * S
    B = -(-rgb.shape[0] // per)
    out = np.zeros((B * per, 3), np.uint8)
    out[:rgb.shape[0]] = rgb
    return out.reshape(B, S, S, 3)
