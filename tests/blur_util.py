"""The blur reference of tests/test_blur_*.py: Pillow's own ImageFilter.GaussianBlur, a numpy
restatement of its box passes driven by gaussian_blur_params (the arithmetic the kernel runs, so a
CPU test can pin it against Pillow without a GPU), the test images, and the transform chain of
color_util.pil_view with the blur at its end."""
import numpy as np
import torch
from PIL import Image, ImageFilter

import color_util as CU
from fsp_amd.data import preprocess as P


def pil_blur(hwc, sigma):
    """uint8 [H, W, 3] -> uint8 [H, W, 3]: img.filter(ImageFilter.GaussianBlur(radius=sigma))."""
    return np.asarray(Image.fromarray(np.ascontiguousarray(hwc)).filter(ImageFilter.GaussianBlur(radius=sigma)))


def box_pass(a, r, ww, fw):
    """One box pass along the last axis of a uint8 array: the 2r + 1 inner samples weigh ww, the two
    just outside them fw, edges repeat the edge sample; 32-bit unsigned sum, + 2^23, >> 24."""
    n = a.shape[-1]
    x = np.arange(n)
    v = a.astype(np.uint64)
    acc = np.zeros(a.shape, np.uint64)
    for d in range(-r, r + 1):
        acc += v[..., np.clip(x + d, 0, n - 1)]
    far = v[..., np.clip(x - r - 1, 0, n - 1)] + v[..., np.clip(x + r + 1, 0, n - 1)]
    s = acc * np.uint64(ww) + far * np.uint64(fw) + np.uint64(1 << 23)
    assert int(s.max(initial=0)) < 1 << 32  # the kernel's accumulator is 32 bits wide
    return (s >> np.uint64(24)).astype(np.uint8)


def np_blur(hwc, sigma):
    """The restatement: three passes along x over every row, then three along y over every column,
    each on the uint8 output of the one before, per channel."""
    r, ww, fw = P.gaussian_blur_params(sigma)
    a = np.transpose(np.asarray(hwc, np.uint8), (2, 0, 1))  # [3, H, W]
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    a = np.swapaxes(a, 1, 2)
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    return np.ascontiguousarray(np.transpose(np.swapaxes(a, 1, 2), (1, 2, 0)))


def blur_images(S, seed=0):
    """{name: uint8 [S, S, 3]}: random, all 255 (the accumulator's headroom), a 0 / 255 checkerboard,
    one 255 pixel on black at a corner and in the middle (the impulse shows every tap and the edge
    rule), and rows that are constant."""
    rs = np.random.RandomState(seed + S)
    y, x = np.mgrid[0:S, 0:S]
    out = {"random": rs.randint(0, 256, size=(S, S, 3), dtype=np.uint8),
           "white": np.full((S, S, 3), 255, np.uint8),
           "checker": np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)}
    for name, (iy, ix) in (("corner", (0, S - 1)), ("middle", (S // 2, S // 2))):
        a = np.zeros((S, S, 3), np.uint8)
        a[iy, ix] = 255
        out["impulse_" + name] = a
    rows = rs.randint(0, 256, size=(S, 1, 3), dtype=np.uint8)
    out["rows"] = np.ascontiguousarray(np.broadcast_to(rows, (S, S, 3)))
    return out


def pil_view(img, plan):
    """color_util.pil_view with the plan's blur (plan.blur: sigma or None) after its colour program
    -> (uint8 [3, S, S], normalised fp32 [3, S, S])."""
    t, f = CU.pil_view(img, plan)
    if getattr(plan, "blur", None) is None:
        return t, f
    hwc = np.ascontiguousarray(t.permute(1, 2, 0).numpy())
    t = torch.from_numpy(pil_blur(hwc, plan.blur).copy()).permute(2, 0, 1).contiguous()
    return t, CU.normalize(t)
