"""GPU-side image preprocessing: the Dassl/torchvision transforms the CoOp/CoCoOp configs
use, on decoded uint8 HWC images, as two HIP kernels (csrc/preprocess.hip).

Reference pipeline (Dassl.pytorch/dassl/data/transforms/transforms.py:206-354, INPUT.
INTERPOLATION "bicubic", configs/trainers/CoCoOp/*.yaml):
* test:  Resize(shorter edge -> max(SIZE)) -> CenterCrop(SIZE) -> ToTensor -> Normalize
* train: RandomResizedCrop(SIZE, scale=RRCROP_SCALE) -> RandomHorizontalFlip -> ToTensor
         -> Normalize
torchvision applies these to PIL images, so the resampling is Pillow's
``Image.resize(BICUBIC)``: separable, antialiased (support x scale when shrinking),
horizontal pass first into a uint8 image, 22-bit fixed-point coefficients
(Pillow libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc). The coefficient
tables are computed here on the host in float64 exactly as that C code does; the kernels
do the integer multiply-accumulate, the uint8 rounding/clipping of both passes, the crop
window, the flip and ToTensor/Normalize in fp32 -- bit-exact to the PIL + torch pipeline
(tests/test_preprocess_*.py check against Pillow itself).

Colour augmentations (Dassl's ``colorjitter`` / ``randomgrayscale`` choices, and the SimCLR
distortion ``RandomApply([ColorJitter], p) -> RandomGrayscale`` behind NATIVE.SIMCLR_COLOR): torchvision
runs them on the PIL image after crop and flip, as thin wrappers over Pillow (ImageEnhance.*,
convert("HSV"), convert("L")). Here each image carries a short program of ops, drawn on the host
(``color_params``), and one more kernel (clipk_image_color) runs the programs on the resampled
uint8 pixels and writes the normalised fp32 -- every byte Pillow's (tests/test_color_*.py). With
no colour op configured nothing changes: the resample kernel writes fp32 directly.

Gaussian blur (the ``pil_gaussian_blur`` choice and NATIVE.SIMCLR_BLUR; the MoCo-v2 form
``RandomApply([GaussianBlur(sigma ~ U(lo, hi))], p)`` with ``img.filter(ImageFilter.GaussianBlur(
radius=sigma))``): Pillow approximates the Gaussian by three box passes of a fractional radius per
axis, in 24-bit fixed point on uint8 images. The host derives the pass constants from sigma as
Pillow's C does (``gaussian_blur_params``); the colour kernel runs the passes on the image it
already holds, after its colour program (clipk_image_color_blur: still one launch) -- every byte
Pillow's (tests/test_blur_*.py). With no blur drawn in a batch the call is the one made before.

Random crop parameters and the flip coin use a torch CPU generator (the transform's own, or
the global one) in torchvision's call order (RandomResizedCrop.get_params,
RandomHorizontalFlip), restated here: torchvision is not installed, so that sequence is
parity-unpinned (documented in DESIGN.md).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _native as N
from .. import ops

PRECISION_BITS = 32 - 8 - 2
MEAN = (0.48145466, 0.4578275, 0.40821073)  # configs/trainers/CoCoOp/*.yaml INPUT.PIXEL_MEAN
STD = (0.26862954, 0.26130258, 0.27577711)


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1,
                    np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resample_coeffs(in_size, out_size, in0=0.0, in1=None):
    """Pillow precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter (support 2):
    returns xmin [out], n [out] (taps used), k int32 [out, ksize]."""
    in1 = float(in_size) if in1 is None else float(in1)
    scale = (in1 - in0) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = in0 + (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)       # C (int) truncation
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = _bicubic((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = w.sum(axis=1, keepdims=True)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = np.where(w < 0, (-0.5 + w * (1 << PRECISION_BITS)), (0.5 + w * (1 << PRECISION_BITS)))
    k = np.trunc(k).astype(np.int32)  # C (int) conversion truncates toward zero
    return xmin.astype(np.int32), xmax.astype(np.int32), k


def shorter_edge_size(w, h, size):
    """torchvision F.resize(img, int): (ow, oh)."""
    if (w <= h and w == size) or (h <= w and h == size):
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


def center_crop_origin(w, h, cw, ch):
    """torchvision F.center_crop: (left, top) -- Python round() (half to even)."""
    return int(round((w - cw) / 2.0)), int(round((h - ch) / 2.0))


def rrc_params(width, height, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """torchvision RandomResizedCrop.get_params: (i, j, h, w) on torch's CPU RNG."""
    area = height * width
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)).item()
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,), generator=generator).item()
            j = torch.randint(0, width - w + 1, size=(1,), generator=generator).item()
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def _jitter_range(value, name, center=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True):
    """torchvision ColorJitter._check_input: a number v -> [center - v, center + v] (the low end
    clipped at 0 for brightness / contrast / saturation), a pair as given; None when the range is
    the single point `center` (the component is off and draws nothing)."""
    if isinstance(value, (int, float)) and not isinstance(value, bool):
        if value < 0:
            raise ValueError(f"If {name} is a single number, it must be non negative.")
        value = [center - float(value), center + float(value)]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        value = [float(value[0]), float(value[1])]
    else:
        raise TypeError(f"{name} should be a single number or a list/tuple with length 2.")
    if not bound[0] <= value[0] <= value[1] <= bound[1]:
        raise ValueError(f"{name} values should be between {bound}, but got {value}.")
    if value[0] == value[1] == center:
        return None
    return tuple(value)


def jitter_ranges(brightness=0, contrast=0, saturation=0, hue=0):
    """ColorJitter.__init__: the four sampling ranges (None: component off). ValueError / TypeError
    on what torchvision rejects (a negative number, a range outside [0, inf) or, for hue,
    [-0.5, 0.5], a reversed pair)."""
    return (_jitter_range(brightness, "brightness"), _jitter_range(contrast, "contrast"),
            _jitter_range(saturation, "saturation"),
            _jitter_range(hue, "hue", center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False))


def hue_shift(hue_factor):
    """torchvision adjust_hue's uint8 offset on Pillow's H channel, np.uint8(hue_factor * 255): the
    product truncated toward zero, modulo 256."""
    return int(hue_factor * 255) % 256


def color_params(brightness=0, contrast=0, saturation=0, hue=0, generator=None):
    """torchvision ColorJitter.get_params + forward as one image's colour program: torch.randperm(4)
    first, then one torch.empty(1).uniform_(lo, hi) each for brightness, contrast, saturation and
    hue in that order (a component whose range is off draws nothing) -> [(op, value), ...] in the
    permuted order, value the blend factor (an fp32 value as a Python float) or, for COLOR_HUE, the
    integer shift 0..255. Each argument: a number v (range [max(0, 1 - v), 1 + v]; hue [-v, v],
    0 <= v <= 0.5), a (lo, hi) pair, or None (off)."""
    ranges = jitter_ranges(*[0 if v is None else v for v in (brightness, contrast, saturation, hue)])
    order = torch.randperm(4, generator=generator).tolist()
    drawn = [None if r is None else float(torch.empty(1).uniform_(r[0], r[1], generator=generator)) for r in ranges]
    ops_ = (N.COLOR_BRIGHTNESS, N.COLOR_CONTRAST, N.COLOR_SATURATION, N.COLOR_HUE)
    prog = []
    for k in order:
        if drawn[k] is not None:
            prog.append((ops_[k], hue_shift(drawn[k]) if k == 3 else drawn[k]))
    return prog


def pack_color_programs(programs):
    """Host descriptors of clipk_image_color: int32 [B, COLOR_DESC] -- per image the op count, the op
    codes in order, then their parameters (fp32 factor bits, or the hue shift)."""
    desc = np.zeros((len(programs), N.COLOR_DESC), np.int32)
    for b, prog in enumerate(programs):
        prog = list(prog)
        if len(prog) > N.COLOR_MAX_OPS:
            raise ValueError(f"a colour program holds at most {N.COLOR_MAX_OPS} ops, got {len(prog)}")
        desc[b, 0] = len(prog)
        for k, (op, value) in enumerate(prog):
            desc[b, 1 + k] = int(op)
            if op in (N.COLOR_BRIGHTNESS, N.COLOR_CONTRAST, N.COLOR_SATURATION):
                desc[b, 1 + N.COLOR_MAX_OPS + k] = np.array(value, np.float32).view(np.int32)
            elif op == N.COLOR_HUE:
                desc[b, 1 + N.COLOR_MAX_OPS + k] = int(value)
    return desc


def gaussian_blur_params(sigma):
    """PIL.ImageFilter.GaussianBlur(radius=sigma) as the constants of its box passes -> (r, ww, fw):
    the integer box radius, and the 24-bit fixed-point weights of the 2r + 1 inner samples and of
    the two outer ones (libImaging BoxBlur.c: _gaussian_blur_radius with 3 passes, then
    ImagingLineBoxBlur8's ww / fw). Every variable and every operation is single precision and
    rounds on its own, as in the C source; only the sqrt and the floor run in double. The fp32
    division behind ww matters: in double, sigma = 1.0 gives 11184810 where Pillow has 11184811."""
    f = np.float32
    s = f(sigma)
    if not (s >= 0) or not np.isfinite(s):
        raise ValueError(f"a blur sigma must be finite and non negative, got {sigma}")
    sigma2 = s * s / f(3)
    big_l = f(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(math.floor((float(big_l) - 1.0) / 2.0))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * sigma2)
    a = a / (f(6) * (sigma2 - (l + f(1)) * (l + f(1))))
    radius = l + a
    r = int(radius)
    ww = int(f(1 << 24) / (radius * f(2) + f(1)))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def blur_sigma_range(value):
    """INPUT.GB_SIGMA -> (lo, hi). ValueError unless it is a pair with 0 <= lo <= hi whose upper end
    stays within the kernel's largest box radius (BLUR_MAX_RADIUS = 7: sigma below about 8.49)."""
    if not isinstance(value, (tuple, list)) or len(value) != 2:
        raise ValueError(f"GB_SIGMA must be a (lo, hi) pair, got {value!r}")
    lo, hi = float(value[0]), float(value[1])
    if not 0.0 <= lo <= hi or not math.isfinite(hi):
        raise ValueError(f"GB_SIGMA needs 0 <= lo <= hi, got {value!r}")
    if gaussian_blur_params(hi)[0] > N.BLUR_MAX_RADIUS:
        raise ValueError(f"GB_SIGMA's upper end {hi} gives a box radius above {N.BLUR_MAX_RADIUS}")
    return lo, hi


def pack_color_blur_programs(programs, blur):
    """Host descriptors of clipk_image_color_blur: int32 [B, COLORBLUR_DESC] -- pack_color_programs'
    12 ints, then per image r (-1: no blur), ww, fw (gaussian_blur_params of its sigma) and a zero.
    blur: one sigma or None per image."""
    blur = list(blur)
    if len(blur) != len(programs):
        raise ValueError("blur must hold one sigma or None per program")
    desc = np.zeros((len(programs), N.COLORBLUR_DESC), np.int32)
    desc[:, :N.COLOR_DESC] = pack_color_programs(programs)
    for b, sigma in enumerate(blur):
        if sigma is None:
            desc[b, N.COLOR_DESC] = -1
            continue
        r, ww, fw = gaussian_blur_params(sigma)
        if r > N.BLUR_MAX_RADIUS:
            raise ValueError(f"sigma {sigma} gives the box radius {r}, above {N.BLUR_MAX_RADIUS}")
        desc[b, N.COLOR_DESC:N.COLOR_DESC + 3] = (r, ww, fw)
    return desc


def color_batch(pix, programs, mean=MEAN, std=STD, out_uint8=False, blur=None):
    """clipk_image_color on uint8 planar pixels [B, 3, S, S] (a CUDA tensor, contiguous): program b
    runs on image b, then ToTensor + Normalize -> fp32 [B, 3, S, S], or the uint8 pixels when
    out_uint8. One launch. `pix` is scratch: unspecified afterwards when the image does not fit LDS.
    blur: one sigma or None per image; where any is set the launch is clipk_image_color_blur, which
    blurs those images after their programs (GaussianBlur(radius=sigma)); None or all None: the
    call made without the argument."""
    if pix.dtype != torch.uint8 or pix.dim() != 4 or pix.shape[1] != 3 or pix.shape[2] != pix.shape[3]:
        raise ValueError("pix must be uint8 [B, 3, S, S]")
    if not pix.is_contiguous() or len(programs) != pix.shape[0]:
        raise ValueError("pix must be contiguous, with one program per image")
    if blur is not None and len(blur) != len(programs):
        raise ValueError("blur must hold one sigma or None per image")
    B, S, dev = int(pix.shape[0]), int(pix.shape[2]), pix.device
    blurred = blur is not None and any(s is not None for s in blur)
    desc = pack_color_blur_programs(programs, blur) if blurred else pack_color_programs(programs)
    d_prog = torch.empty(max(B, 1) * desc.shape[1], dtype=torch.int32, device=dev)
    out = torch.empty(B, 3, S, S, device=dev, dtype=torch.uint8 if out_uint8 else torch.float32)
    mean_t = torch.tensor(mean, dtype=torch.float32, device=dev)
    std_t = torch.tensor(std, dtype=torch.float32, device=dev)
    N.call("clipk_image_color_blur" if blurred else "clipk_image_color", B, S, ops._p(pix), desc.ctypes.data,
           ops._p(d_prog), ops._p(mean_t), ops._p(std_t), 1 if out_uint8 else 0, ops._p(out), ops._stream())
    return out


class Plan:
    """One image's geometry: source window (x0, y0, w, h) resized to (rw, rh), output
    window (ox, oy, S, S) of the resized image, horizontal flip; `color`: the colour program
    [(op, value), ...] that runs after them (empty: none); `blur`: the sigma of the Gaussian blur
    that runs last (None: none)."""

    def __init__(self, x0, y0, w, h, rw, rh, ox, oy, S, flip, color=(), blur=None):
        self.x0, self.y0, self.w, self.h = x0, y0, w, h
        self.rw, self.rh, self.ox, self.oy, self.S, self.flip = rw, rh, ox, oy, S, flip
        self.color = list(color)
        self.blur = blur


def test_plan(w, h, size):
    rw, rh = shorter_edge_size(w, h, size)
    ox, oy = center_crop_origin(rw, rh, size, size)
    return Plan(0, 0, w, h, rw, rh, ox, oy, size, False)


def train_plan(w, h, size, scale=(0.08, 1.0), flip_p=0.5, generator=None):
    i, j, ch, cw = rrc_params(w, h, scale, generator=generator)
    flip = bool(torch.rand(1, generator=generator) < flip_p)
    return Plan(j, i, cw, ch, size, size, 0, 0, size, flip)


def _tables(plans, shapes):
    """Per-image descriptors (int64 [B, 16]) + packed coefficient tables (int32)."""
    desc, tabs, tmp_off, tab_off = [], [], 0, 0
    for p, (H, W) in zip(plans, shapes):
        hx, hn, hk = resample_coeffs(p.w, p.rw)
        vy, vn, vk = resample_coeffs(p.h, p.rh)
        hx, hn, hk = hx[p.ox:p.ox + p.S], hn[p.ox:p.ox + p.S], hk[p.ox:p.ox + p.S]
        vy, vn, vk = vy[p.oy:p.oy + p.S], vn[p.oy:p.oy + p.S], vk[p.oy:p.oy + p.S]
        ty0 = int(vy.min())
        ty1 = int((vy + vn).max())
        rows = max(ty1 - ty0, 1)
        hks, vks = hk.shape[1], vk.shape[1]
        h_tab = np.concatenate([hx[:, None], hn[:, None], hk], axis=1).astype(np.int32)
        v_tab = np.concatenate([(vy - ty0)[:, None], vn[:, None], vk], axis=1).astype(np.int32)
        desc.append([0, W, p.x0, p.y0 + ty0, p.S, int(p.flip), tab_off, hks, tab_off + h_tab.size, vks,
                     tmp_off, rows, H, 0, 0, 0])
        tabs += [h_tab.ravel(), v_tab.ravel()]
        tab_off += h_tab.size + v_tab.size
        tmp_off += rows * p.S * 3
    return np.asarray(desc, np.int64), np.concatenate(tabs).astype(np.int32), tmp_off


def axis_taps(in_size, out_size, xx):
    """resample_coeffs' (ksize, xmin[xx], xmax[xx]) of one output index in Python floats: the same
    IEEE double operations in the same order, int() for C's truncation."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    center = (xx + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0)
    xmax = min(int(center + support + 0.5), in_size) - xmin
    return int(math.ceil(support)) * 2 + 1, xmin, xmax


def _table_params(plans, shapes):
    """_tables without the tables: the same descriptors (int64 [B, 16]) and temp size, plus the
    records clipk_resample_tables builds the block from (int64 [B, RESAMPLE_PARAMS]) and the
    block's size in ints. Scalar work only: center, xmin and xmin + xmax are nondecreasing in the
    output index, so the temp rows start at the first v row's xmin and end at the last one's
    xmin + xmax."""
    desc = np.zeros((len(plans), 16), np.int64)
    par = np.zeros((len(plans), N.RESAMPLE_PARAMS), np.int64)
    tmp_off = tab_off = 0
    for b, (p, (H, W)) in enumerate(zip(plans, shapes)):
        hks = axis_taps(p.w, p.rw, 0)[0]
        vks, ty0, _ = axis_taps(p.h, p.rh, p.oy)
        _, ylast, nlast = axis_taps(p.h, p.rh, p.oy + p.S - 1)
        rows = max(ylast + nlast - ty0, 1)
        v_off = tab_off + p.S * (2 + hks)
        desc[b] = (0, W, p.x0, p.y0 + ty0, p.S, int(p.flip), tab_off, hks, v_off, vks, tmp_off, rows, H, 0, 0, 0)
        par[b] = (p.w, p.rw, p.ox, tab_off, hks, p.h, p.rh, p.oy, v_off, vks, p.S, ty0)
        tab_off = v_off + p.S * (2 + vks)
        tmp_off += rows * p.S * 3
    return desc, par, tab_off, tmp_off


class Resident:
    """A decoded image that already lies in device memory (data/image_bank.py): the address of its
    first byte, uint8 HWC, rows packed. Stands where preprocess_batch takes an image; `keep` holds
    whatever owns the memory."""

    def __init__(self, address, H, W, keep=None):
        self.address, self.keep = int(address), keep
        self.shape = (int(H), int(W), 3)


def preprocess_batch(images, plans, mean=MEAN, std=STD, device="cuda", out_uint8=False, src_index=None,
                     color=None, blur=None, tables="host"):
    """images: list of uint8 HWC (RGB) numpy arrays or CPU/GPU torch tensors; plans: Plan
    per image (all with the same S). Returns fp32 [B, 3, S, S] normalised on `device` (or
    the uint8 resampled pixels [B, 3, S, S] when out_uint8, for bit-exact checks).
    src_index: plans[k] reads images[src_index[k]] (B = len(plans) outputs from fewer source
    images, each uploaded once: the two views of a SimCLR batch); None: plans[k] reads images[k].
    color: one colour program per plan (color_params' form), run after crop and flip. When any is
    non-empty the resample writes uint8 and clipk_image_color writes the output (one more launch);
    None or all empty: the resample kernel writes the output itself, as without the argument.
    blur: one sigma or None per plan, GaussianBlur(radius=sigma) after the colour program, in the
    colour launch (clipk_image_color_blur; color_batch). None or all None: as without the argument.
    tables: "host" (the coefficient tables come from _tables and are uploaded) or "device"
    (clipk_resample_tables builds the same block on the GPU from one record per plan; descriptors,
    records and mean / std travel in ONE non-blocking copy from pinned memory). The same bits.
    An image may be a Resident (pixels already on the device, read where they lie); with any the
    launch is clipk_image_resample_at and only the other images are uploaded."""
    dev = torch.device(device)
    if tables not in ("host", "device"):
        raise ValueError(f'tables must be "host" or "device", got {tables!r}')
    S = plans[0].S
    if any(p.S != S for p in plans):
        raise ValueError("all plans must share the output size")
    ts = [im if isinstance(im, Resident) else torch.as_tensor(im) for im in images]
    for t in ts:
        if not isinstance(t, Resident) and (t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3):
            raise ValueError("images must be uint8 [H, W, 3]")
    color = None if color is None else [list(c) for c in color]
    if color is not None and len(color) != len(plans):
        raise ValueError("color must hold one program per plan")
    blur = None if blur is None else list(blur)
    if blur is not None and len(blur) != len(plans):
        raise ValueError("blur must hold one sigma or None per plan")
    if blur is not None and all(s is None for s in blur):
        blur = None
    staged = (color is not None and any(color)) or blur is not None
    src_index = [int(k) for k in (range(len(plans)) if src_index is None else src_index)]
    if len(src_index) != len(plans) or any(not 0 <= k < len(ts) for k in src_index):
        raise ValueError("src_index must name one source image per plan")
    img_shapes = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
    shapes = [img_shapes[k] for k in src_index]  # of the image each plan reads
    for p, (H, W) in zip(plans, shapes):
        if p.x0 < 0 or p.y0 < 0 or p.x0 + p.w > W or p.y0 + p.h > H or p.rw < p.ox + S or p.rh < p.oy + S:
            raise ValueError("plan window outside the image")
        if tables == "device" and (p.w < 1 or p.h < 1 or p.ox < 0 or p.oy < 0 or S < 1):
            raise ValueError("plan window outside the image")
    if tables == "host":
        desc, tab, tmp_elems = _tables(plans, shapes)
    else:
        desc, par, tab_elems, tmp_elems = _table_params(plans, shapes)
    # the uploaded images, packed; a Resident stays where it is
    host = [k for k, t in enumerate(ts) if not isinstance(t, Resident)]
    offs = np.zeros(len(ts) + 1, np.int64)
    offs[1:][host] = [img_shapes[k][0] * img_shapes[k][1] * 3 for k in host]
    offs = np.cumsum(offs)
    src = torch.cat([ts[k].reshape(-1) for k in host]).to(dev, non_blocking=True) if host else None
    absolute = len(host) < len(ts)
    if absolute:
        base = src.data_ptr() if host else 0
        addr = np.asarray([t.address if isinstance(t, Resident) else base + int(o) for t, o in zip(ts, offs[:-1])],
                          np.int64)
        desc[:, 0] = addr[src_index]
    else:
        desc[:, 0] = offs[:-1][src_index]
    B = len(plans)
    if tables == "host":
        d_desc = torch.from_numpy(desc).to(dev)
        d_tab = torch.from_numpy(tab).to(dev)
        mean_t = torch.tensor(mean, dtype=torch.float32, device=dev)
        std_t = torch.tensor(std, dtype=torch.float32, device=dev)
    else:
        nd, npar = desc.size, par.size
        stage = torch.empty(nd + npar + 3, dtype=torch.int64, pin_memory=True)
        sn = stage.numpy()
        sn[:nd], sn[nd:nd + npar] = desc.ravel(), par.ravel()
        sn[nd + npar:].view(np.float32)[:] = tuple(mean) + tuple(std)
        d_stage = stage.to(dev, non_blocking=True)
        d_desc, d_par = d_stage[:nd], d_stage[nd:nd + npar]
        mean_t, std_t = d_stage[nd + npar:].view(torch.float32).split(3)
        d_tab = torch.empty(max(tab_elems, 1), dtype=torch.int32, device=dev)
        N.call("clipk_resample_tables", B, S, ops._p(d_par), ops._p(d_tab), ops._stream())
    tmp = torch.empty(max(tmp_elems, 1), dtype=torch.uint8, device=dev)
    to_u8 = out_uint8 or staged
    out = torch.empty(B, 3, S, S, device=dev, dtype=torch.uint8 if to_u8 else torch.float32)
    rows_max = int(desc[:, 11].max())
    if absolute:
        N.call("clipk_image_resample_at", B, S, rows_max, ops._p(d_desc), ops._p(d_tab), ops._p(tmp),
               ops._p(mean_t), ops._p(std_t), 1 if to_u8 else 0, ops._p(out), ops._stream())
    else:
        N.call("clipk_image_resample", B, S, rows_max, ops._p(src), ops._p(d_desc), ops._p(d_tab), ops._p(tmp),
               ops._p(mean_t), ops._p(std_t), 1 if to_u8 else 0, ops._p(out), ops._stream())
    if staged:
        return color_batch(out, color if color is not None else [[]] * B, mean, std, out_uint8, blur)
    return out


class GpuTransform:
    """Dassl transform_train / transform_test equivalent for the CoOp/CoCoOp configs
    (random_resized_crop + random_flip + normalize / resize + center_crop + normalize), plus
    Dassl's colorjitter (ColorJitter(INPUT.COLORJITTER_B/C/S/H), under RandomApply when
    INPUT.COLORJITTER_P < 1) and randomgrayscale (RandomGrayscale(INPUT.RGS_P)) for training, in
    the reference's order: crop, flip, colour, grayscale, ToTensor, Normalize. With
    NATIVE.SIMCLR_COLOR and a two-view objective (data/manager.py two_views) the training transform
    carries the SimCLR distortion whatever INPUT.TRANSFORMS says: the jitter under
    RandomApply(NATIVE.SIMCLR_COLOR_P), then RandomGrayscale(INPUT.RGS_P).
    pil_gaussian_blur (this package's choice, the MoCo-v2 form; training only): RandomApply(INPUT.GB_P)
    around PIL's ImageFilter.GaussianBlur(radius = sigma), sigma ~ U(INPUT.GB_SIGMA), last in the
    uint8 chain; NATIVE.SIMCLR_BLUR gives it to the two views of a two-view objective under
    RandomApply(NATIVE.SIMCLR_BLUR_P), with or without SIMCLR_COLOR. Dassl's gaussian_blur stays
    unimplemented: current Dassl wires that name to torchvision's GaussianBlur(kernel_size=GB_K), a
    float convolution and another function than Pillow's filter."""

    def __init__(self, cfg, is_train, device="cuda", generator=None):
        choices = list(cfg.INPUT.TRANSFORMS)
        allowed = {"random_resized_crop", "random_flip", "normalize", "colorjitter", "randomgrayscale",
                   "pil_gaussian_blur"}
        if is_train and not set(choices) <= allowed:
            hint = (" (gaussian_blur, torchvision's convolution, is not built: pil_gaussian_blur is Pillow's "
                    "ImageFilter.GaussianBlur)" if "gaussian_blur" in choices else "")
            raise NotImplementedError(f"GPU transforms implement {sorted(allowed)}, got {choices}{hint}")
        if cfg.INPUT.INTERPOLATION != "bicubic":
            raise NotImplementedError("GPU transforms implement bicubic interpolation")
        self.is_train = is_train
        self.size = max(cfg.INPUT.SIZE)
        self.rrc = "random_resized_crop" in choices
        self.flip = "random_flip" in choices
        self.scale = tuple(cfg.INPUT.get("RRCROP_SCALE", (0.08, 1.0)))
        norm = "normalize" in choices
        self.mean = tuple(cfg.INPUT.PIXEL_MEAN) if norm else (0.0, 0.0, 0.0)
        self.std = tuple(cfg.INPUT.PIXEL_STD) if norm else (1.0, 1.0, 1.0)
        self.device = device
        self.generator = generator  # None: torch's global CPU RNG
        # NATIVE.DEVICE_TABLES: the resample tables are built on the GPU (preprocess_batch tables="device")
        self.tables = "device" if bool(cfg.get("NATIVE", {}).get("DEVICE_TABLES", False)) else "host"
        # colour stage (training only): jitter ranges (None: no jitter), the RandomApply probability
        # around it (>= 1: no coin is drawn) and RandomGrayscale's probability (None: not configured)
        self.jitter, self.jitter_p, self.gray_p = None, 1.0, None
        # blur (training only): the sigma range (None: no blur) and the RandomApply probability around it
        self.blur_sigma, self.blur_p = None, 1.0
        if is_train:
            from .manager import two_views
            simclr_blur = bool(cfg.get("NATIVE", {}).get("SIMCLR_BLUR", False)) and two_views(cfg)
            if simclr_blur or "pil_gaussian_blur" in choices:
                self.blur_sigma = blur_sigma_range(cfg.INPUT.get("GB_SIGMA", (0.1, 2.0)))
                self.blur_p = float(cfg.NATIVE.get("SIMCLR_BLUR_P", 0.5) if simclr_blur
                                    else cfg.INPUT.get("GB_P", 0.5))
            simclr = bool(cfg.get("NATIVE", {}).get("SIMCLR_COLOR", False)) and two_views(cfg)
            if simclr or "colorjitter" in choices:
                inp = cfg.INPUT
                self.jitter = jitter_ranges(inp.get("COLORJITTER_B", 0.4), inp.get("COLORJITTER_C", 0.4),
                                            inp.get("COLORJITTER_S", 0.4), inp.get("COLORJITTER_H", 0.1))
                self.jitter_p = float(cfg.NATIVE.get("SIMCLR_COLOR_P", 0.8) if simclr
                                      else cfg.INPUT.get("COLORJITTER_P", 1.0))
            if simclr or "randomgrayscale" in choices:
                self.gray_p = float(cfg.INPUT.get("RGS_P", 0.2))

    def color_program(self):
        """One image's colour draws, after its crop and flip: the RandomApply coin (torch.rand(1);
        skipped when p < coin) when jitter_p < 1, the jitter draws (color_params), the grayscale
        coin (torch.rand(1) < p). Draws nothing when no colour op is configured."""
        prog = []
        if self.jitter is not None:
            if not (self.jitter_p < 1.0 and self.jitter_p < float(torch.rand(1, generator=self.generator))):
                prog += color_params(*self.jitter, generator=self.generator)
        if self.gray_p is not None and bool(torch.rand(1, generator=self.generator) < self.gray_p):
            prog.append((N.COLOR_GRAYSCALE, 0))
        return prog

    def blur_draw(self):
        """One image's blur draws, after its colour draws: the RandomApply coin (torch.rand(1); skipped
        when p < coin; none at p >= 1), then, if the blur is applied, sigma =
        torch.empty(1).uniform_(lo, hi). Draws nothing and returns None when no blur is configured."""
        if self.blur_sigma is None:
            return None
        if self.blur_p < 1.0 and self.blur_p < float(torch.rand(1, generator=self.generator)):
            return None
        return float(torch.empty(1).uniform_(self.blur_sigma[0], self.blur_sigma[1], generator=self.generator))

    def plan(self, w, h):
        if not self.is_train:
            return test_plan(w, h, self.size)
        if self.rrc:
            p = train_plan(w, h, self.size, self.scale, 0.5 if self.flip else 0.0, generator=self.generator)
        else:
            rw = rh = self.size  # Resize(input_size) when no random crop
            p = Plan(0, 0, w, h, rw, rh, 0, 0, self.size, False)
            if self.flip:
                p.flip = bool(torch.rand(1, generator=self.generator) < 0.5)
        p.color = self.color_program()
        p.blur = self.blur_draw()
        return p

    def plans(self, sizes, views=1):
        """Plans for images of the given (w, h) sizes, `views` draws each, image-major from the
        transform's generator: image 0 view 1, image 0 view 2, image 1 view 1, ..."""
        return [self.plan(w, h) for w, h in sizes for _ in range(views)]

    def __call__(self, images, views=1):
        """views=1: the transformed batch [B, 3, S, S]. views=2 (SimCLR): two independent draws of
        the transform per image -> (x1, x2), the two halves of ONE [2B, 3, S, S] output (no copy);
        the pixels are uploaded once and one resample launch (and, with colour ops or blur, one
        colour / blur launch) covers both views. An image may be a preprocess.Resident (an image
        bank's record): its size is the recorded one and its pixels are read where they lie."""
        sizes = [(int(im.shape[1]), int(im.shape[0])) for im in images]
        if views == 1:
            drawn = self.plans(sizes)
            return preprocess_batch(images, drawn, self.mean, self.std, self.device, color=[p.color for p in drawn],
                                    blur=[p.blur for p in drawn], tables=self.tables)
        if views != 2:
            raise ValueError(f"views must be 1 or 2, got {views}")
        B = len(sizes)
        drawn = self.plans(sizes, 2)  # image-major
        drawn = drawn[0::2] + drawn[1::2]
        out = preprocess_batch(images, drawn, self.mean, self.std, self.device, src_index=list(range(B)) * 2,
                               color=[p.color for p in drawn], blur=[p.blur for p in drawn], tables=self.tables)
        return out[:B], out[B:]
