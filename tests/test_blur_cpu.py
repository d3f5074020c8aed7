"""CPU: the host side of the Gaussian blur (PIL.ImageFilter.GaussianBlur for the SimCLR views and
the pil_gaussian_blur transform) -- Pillow's pass constants from sigma, the pass arithmetic restated
in numpy against Pillow itself, the config surface, GB_SIGMA's validation, the draw order against a
replay by hand, the no-blur guard, the C-ABI registration and the descriptor packing."""
import os
import re

import numpy as np
import pytest
import torch

import blur_util as BU
from fsp_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_ = 5  # COLOR_GRAYSCALE

# sigma -> (r, ww, fw): Pillow 12.2's constants (the fp32 division behind ww: 1.0 -> ...811, not ...810)
PINNED = {0.1: (0, 16721291, 27962), 0.5: (0, 15379114, 699051), 1.0: (0, 11184811, 2796202),
          1.5: (1, 5452595, 209715), 2.0: (1, 4473924, 1677722), 3.0: (2, 2876094, 1198373),
          8.0: (7, 1052688, 493448), 0.0: (0, 16777216, 0)}


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _uniform(g, lo, hi):
    return float(torch.empty(1).uniform_(lo, hi, generator=g))


def test_gaussian_blur_params_equal_pillows_constants():
    from fsp_amd.data.preprocess import gaussian_blur_params
    for sigma, want in PINNED.items():
        got = gaussian_blur_params(sigma)
        assert got == want and all(isinstance(v, int) for v in got), (sigma, got)
        r, ww, fw = got
        assert (2 * r + 1) * ww + 2 * fw <= 1 << 24  # the 32-bit accumulator's condition
    rs = np.random.RandomState(0)
    assert {gaussian_blur_params(s)[0] for s in rs.uniform(0.1, 2.0, 200)} == {0, 1}
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            gaussian_blur_params(bad)


SIZES_HW = [(1, 1), (2, 3), (7, 7), (33, 20), (64, 64)]


def _seeded_sigmas():
    return [float(s) for s in np.random.RandomState(42).uniform(0.1, 2.0, 20)]


@pytest.mark.parametrize("hw", SIZES_HW, ids=["%dx%d" % s for s in SIZES_HW])
def test_numpy_restatement_equals_pillow(hw):
    rs = np.random.RandomState(hw[0] * 100 + hw[1])
    imgs = [rs.randint(0, 256, size=hw + (3,), dtype=np.uint8), np.full(hw + (3,), 255, np.uint8)]
    bad = 0
    for sigma in [0.1, 0.3, 0.5, 1.0, 1.5, 2.0, 3.0, 8.0] + _seeded_sigmas():
        for im in imgs:
            bad += int((BU.np_blur(im, sigma) != BU.pil_blur(im, sigma)).sum())
    assert bad == 0


def test_restatement_on_the_gpu_tests_images():
    for S in (1, 2, 7):
        for name, im in BU.blur_images(S).items():
            for sigma in (0.1, 1.0, 1.5, 3.0, 8.0):
                assert np.array_equal(BU.np_blur(im, sigma), BU.pil_blur(im, sigma)), (S, name, sigma)
    im = BU.blur_images(7)["impulse_middle"]
    assert len(np.unique(BU.pil_blur(im, 1.5))) > 3  # the impulse spreads: a blur, not the identity
    assert np.array_equal(BU.pil_blur(im, 0.0), im)


def _cfg(transforms=(), **inp):
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    cfg.INPUT.TRANSFORMS = ["random_resized_crop", "random_flip", "normalize"] + list(transforms)
    for k, v in inp.items():
        cfg.INPUT[k] = v
    return cfg


def _simclr_cfg(blur, color=False, name="CoOp", **native):
    cfg = _cfg()
    cfg.TRAINER.NAME = name
    cfg.TRAINER.COOP.LOSS_TYPE = "simclr"
    cfg.TRAINER.IVLP.SIMCLR_ALPHA = 0.5
    cfg.NATIVE.SIMCLR_BLUR = blur
    cfg.NATIVE.SIMCLR_COLOR = color
    for k, v in native.items():
        cfg.NATIVE[k] = v
    return cfg


SIZES = [(80, 60), (61, 97), (120, 120), (64, 200)]


def test_config_defaults():
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    assert cfg.INPUT.GB_P == 0.5 and tuple(cfg.INPUT.GB_SIGMA) == (0.1, 2.0)
    assert cfg.NATIVE.SIMCLR_BLUR is False and cfg.NATIVE.SIMCLR_BLUR_P == 0.5
    assert "pil_gaussian_blur" not in cfg.INPUT.TRANSFORMS
    cfg.merge_from_list(["INPUT.GB_SIGMA", "[0.5, 1.5]", "NATIVE.SIMCLR_BLUR", "True"])
    assert cfg.INPUT.GB_SIGMA == (0.5, 1.5) and cfg.NATIVE.SIMCLR_BLUR is True


def test_pil_gaussian_blur_is_a_training_choice_and_gaussian_blur_still_raises():
    from fsp_amd.data.preprocess import GpuTransform
    t = GpuTransform(_cfg(["pil_gaussian_blur"]), True, "cpu", _gen(0))
    assert t.blur_sigma == (0.1, 2.0) and t.blur_p == 0.5 and t.jitter is None and t.gray_p is None
    t = GpuTransform(_cfg(["pil_gaussian_blur"], GB_P=1.0, GB_SIGMA=[0.5, 0.5]), True, "cpu", _gen(0))
    assert t.blur_sigma == (0.5, 0.5) and t.blur_p == 1.0
    # the evaluation transform never blurs
    t = GpuTransform(_cfg(["pil_gaussian_blur"]), False, "cpu")
    assert t.blur_sigma is None and t.plan(80, 60).blur is None
    assert GpuTransform(_simclr_cfg(True), False, "cpu").blur_sigma is None
    # Dassl's name is a different function (torchvision's convolution): refused, pointing at this one
    with pytest.raises(NotImplementedError, match="pil_gaussian_blur"):
        GpuTransform(_cfg(["gaussian_blur"]), True, "cpu")
    with pytest.raises(NotImplementedError):
        GpuTransform(_cfg(["pil_gaussian_blur", "randaugment"]), True, "cpu")
    # without the choice or the flag there is no blur
    t = GpuTransform(_cfg(), True, "cpu", _gen(0))
    assert t.blur_sigma is None and t.plan(80, 60).blur is None


def test_gb_sigma_validation():
    from fsp_amd.data.preprocess import GpuTransform, blur_sigma_range, gaussian_blur_params
    for bad in (1.0, (0.1,), (0.1, 1.0, 2.0), (-0.1, 2.0), (2.0, 0.1), (0.1, 8.5), (0.1, 100.0)):
        with pytest.raises(ValueError):
            GpuTransform(_cfg(["pil_gaussian_blur"], GB_SIGMA=bad), True, "cpu")
        with pytest.raises(ValueError):
            GpuTransform(_with_sigma(_simclr_cfg(True), bad), True, "cpu")
    assert gaussian_blur_params(8.48)[0] == 7 and gaussian_blur_params(8.5)[0] == 8  # the limit, about 8.49
    assert blur_sigma_range([0.0, 8.48]) == (0.0, 8.48) and blur_sigma_range((0.3, 0.3)) == (0.3, 0.3)
    # not read where no blur is configured
    GpuTransform(_cfg(GB_SIGMA=(2.0, 0.1)), True, "cpu")
    GpuTransform(_cfg(["pil_gaussian_blur"], GB_SIGMA=(2.0, 0.1)), False, "cpu")


def _with_sigma(cfg, sigma):
    cfg.INPUT.GB_SIGMA = sigma
    return cfg


def _replay_view(r, w, h, jitter_p, gray_p, blur_p, lo=0.1, hi=2.0):
    """One view's draws by hand: crop, flip, the colour draws (jitter_p None: no colour configured),
    the blur coin (only when p < 1), sigma (only if applied)."""
    from fsp_amd.data.preprocess import color_params, train_plan
    ref = train_plan(w, h, 32, generator=r)
    if jitter_p is not None:
        if jitter_p >= 1.0 or not (jitter_p < float(torch.rand(1, generator=r))):
            ref.color += color_params(0.4, 0.4, 0.4, 0.1, generator=r)
        if bool(torch.rand(1, generator=r) < gray_p):
            ref.color.append((G_, 0))
    if blur_p is not None:
        if blur_p >= 1.0 or not (blur_p < float(torch.rand(1, generator=r))):
            ref.blur = _uniform(r, lo, hi)
    return ref


def _same(a, b):
    return ((a.x0, a.y0, a.w, a.h, a.rw, a.rh, a.ox, a.oy, a.S, a.flip, a.color, a.blur) ==
            (b.x0, b.y0, b.w, b.h, b.rw, b.rh, b.ox, b.oy, b.S, b.flip, b.color, b.blur))


@pytest.mark.parametrize("blur_p", [1.0, 0.5])
@pytest.mark.parametrize("color", [False, True])
def test_draw_order_per_view_replayed_by_hand(color, blur_p):
    from fsp_amd.data.preprocess import GpuTransform
    names = (["colorjitter", "randomgrayscale"] if color else []) + ["pil_gaussian_blur"]
    t = GpuTransform(_cfg(names, GB_P=blur_p, COLORJITTER_P=0.7, RGS_P=0.5), True, "cpu", _gen(7))
    plans = t.plans(SIZES * 2, views=2)
    r = _gen(7)
    ref = [_replay_view(r, w, h, 0.7 if color else None, 0.5, blur_p) for w, h in SIZES * 2 for _ in range(2)]
    assert len(plans) == len(ref) == 16
    for k, (a, b) in enumerate(zip(plans, ref)):
        assert _same(a, b), k
        assert a.blur is None or (0.1 <= a.blur <= 2.0 and float(np.float32(a.blur)) == a.blur)
    assert torch.equal(t.generator.get_state(), r.get_state())  # nothing more, nothing less was drawn
    blurred = {p.blur is not None for p in plans}
    assert blurred == ({True} if blur_p >= 1.0 else {False, True})
    if color:
        assert {bool(p.color) for p in plans} == {False, True}


@pytest.mark.parametrize("name", ["CoOp", "IVLP"])
@pytest.mark.parametrize("color", [False, True])
def test_simclr_blur_flag_on_two_view_objectives(name, color):
    from fsp_amd.data.preprocess import GpuTransform
    t = GpuTransform(_simclr_cfg(True, color, name, SIMCLR_BLUR_P=0.6), True, "cpu", _gen(2))
    assert t.blur_sigma == (0.1, 2.0) and t.blur_p == 0.6
    assert (t.jitter is not None) == color and (t.gray_p is not None) == color  # independent of SIMCLR_COLOR
    plans = t.plans(SIZES * 4, views=2)
    r = _gen(2)
    ref = [_replay_view(r, w, h, 0.8 if color else None, 0.2, 0.6) for w, h in SIZES * 4 for _ in range(2)]
    assert all(_same(a, b) for a, b in zip(plans, ref)) and torch.equal(t.generator.get_state(), r.get_state())
    assert 0 < sum(p.blur is not None for p in plans) < len(plans)
    # the default probability, and INPUT.GB_P is not the flag's
    assert GpuTransform(_simclr_cfg(True, color, name), True, "cpu").blur_p == 0.5
    # not a two-view objective: the flag alone changes nothing
    assert GpuTransform(_simclr_cfg(True, color, "CoCoOp"), True, "cpu").blur_sigma is None
    cfg = _simclr_cfg(True, color, "CoOp")
    cfg.TRAINER.COOP.LOSS_TYPE = "ce"
    assert GpuTransform(cfg, True, "cpu").blur_sigma is None


@pytest.mark.parametrize("views", [1, 2])
def test_no_blur_configured_draws_todays_stream(views):
    """Guard: without the choice and the flag, plans and generator state after a batch are those of
    the chain without a blur -- with colour configured and without."""
    from fsp_amd.data.preprocess import GpuTransform
    for cfg, jp, gp in ((_cfg(), None, 0.0), (_simclr_cfg(False), None, 0.0), (_simclr_cfg(False, True), 0.8, 0.2),
                        (_cfg(["colorjitter", "randomgrayscale"]), 1.0, 0.2)):
        t = GpuTransform(cfg, True, "cpu", _gen(9))
        plans = t.plans(SIZES, views=views)
        r = _gen(9)
        ref = [_replay_view(r, w, h, jp, gp, None) for w, h in SIZES for _ in range(views)]
        assert len(plans) == len(ref) and all(_same(a, b) for a, b in zip(plans, ref))
        assert all(p.blur is None for p in plans)
        assert torch.equal(t.generator.get_state(), r.get_state())


def test_blur_symbol_and_constants_are_registered():
    hdr = open(os.path.join(ROOT, "include", "clipk.h")).read()
    assert _native.COLORBLUR_DESC == 16 and _native.BLUR_MAX_RADIUS == 7
    assert re.search(r"\bCLIPK_COLORBLUR_DESC = 16\b", hdr) and re.search(r"\bCLIPK_BLUR_MAX_RADIUS = 7\b", hdr)
    assert _native.COLOR_MAX_OPS == 5 and _native.COLOR_DESC == 12  # clipk_image_color's ABI is untouched
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint clipk_image_color_blur\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m and len(m.group(1).split(",")) == 10
    assert _native.SIGNATURES["clipk_image_color_blur"] == _native.SIGNATURES["clipk_image_color"]
    assert hasattr(_native.load(), "clipk_image_color_blur")


def test_descriptor_packing():
    from fsp_amd.data.preprocess import pack_color_blur_programs, pack_color_programs
    progs = [[(1, 0.5), (4, 243)], [], [(G_, 0)], []]
    d = pack_color_blur_programs(progs, [1.5, None, 0.0, 8.0])
    assert d.dtype == np.int32 and d.shape == (4, 16) and d.flags["C_CONTIGUOUS"]
    assert np.array_equal(d[:, :12], pack_color_programs(progs))
    assert d[:, 12:].tolist() == [[1, 5452595, 209715, 0], [-1, 0, 0, 0], [0, 1 << 24, 0, 0], [7, 1052688, 493448, 0]]
    for bad in (8.5, 20.0):  # r > 7
        with pytest.raises(ValueError):
            pack_color_blur_programs(progs, [None, None, bad, None])
    with pytest.raises(ValueError):
        pack_color_blur_programs(progs, [None] * 3)
    with pytest.raises(ValueError):
        pack_color_blur_programs([[(1, 1.0)] * 6], [1.0])
