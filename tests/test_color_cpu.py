"""CPU: the host side of the colour stage (ColorJitter / RandomGrayscale for the SimCLR views) --
color_params' generator consumption against a replay by hand, the GpuTransform surface, the
flag-off guard, the C-ABI registration of clipk_image_color and the descriptor packing."""
import os
import re

import numpy as np
import pytest
import torch

from fsp_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_, C_, S_, H_, G_ = 1, 2, 3, 4, 5


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _uniform(g, lo, hi):
    return float(torch.empty(1).uniform_(lo, hi, generator=g))


def test_color_op_codes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "clipk.h")).read()
    for name, val in (("BRIGHTNESS", B_), ("CONTRAST", C_), ("SATURATION", S_), ("HUE", H_), ("GRAYSCALE", G_),
                      ("MAX_OPS", 5), ("DESC", 12)):
        assert getattr(_native, "COLOR_" + name) == val
        assert re.search(r"\bCLIPK_COLOR_%s = %d\b" % (name, val), hdr), name


def test_color_symbol_is_registered():
    hdr = open(os.path.join(ROOT, "include", "clipk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint clipk_image_color\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m
    assert "clipk_image_color" in _native.SIGNATURES
    assert len(_native.SIGNATURES["clipk_image_color"][1]) == len(m.group(1).split(",")) == 10
    assert hasattr(_native.load(), "clipk_image_color")
    assert "csrc/color_ops.h" in [rel for rel, _ in _native.source_files()]


def test_color_params_consumes_torchvisions_draws():
    from fsp_amd.data.preprocess import color_params
    for seed in range(8):
        g, r = _gen(seed), _gen(seed)
        prog = color_params(0.4, 0.4, 0.4, 0.1, generator=g)
        order = torch.randperm(4, generator=r).tolist()
        b, c, s = _uniform(r, 0.6, 1.4), _uniform(r, 0.6, 1.4), _uniform(r, 0.6, 1.4)
        h = _uniform(r, -0.1, 0.1)
        want = {0: (B_, b), 1: (C_, c), 2: (S_, s), 3: (H_, int(h * 255) % 256)}
        assert prog == [want[k] for k in order]
        assert torch.equal(g.get_state(), r.get_state())  # nothing more, nothing less was drawn
        for op, v in prog:
            if op == H_:
                assert isinstance(v, int) and (v <= 25 or v >= 231)
            else:
                assert 0.6 <= v <= 1.4 and float(np.float32(v)) == v  # an fp32 value
    # a number above 1 clips the low end at 0; pairs are taken as given
    g, r = _gen(3), _gen(3)
    prog = dict(color_params(1.5, (0.2, 0.3), 0, (-0.5, 0.5), generator=g))
    torch.randperm(4, generator=r)
    assert prog[B_] == _uniform(r, 0.0, 2.5) and prog[C_] == _uniform(r, 0.2, 0.3)
    assert S_ not in prog and prog[H_] == int(_uniform(r, -0.5, 0.5) * 255) % 256
    assert torch.equal(g.get_state(), r.get_state())


def test_color_params_disabled_components_draw_nothing():
    from fsp_amd.data.preprocess import color_params
    g, r = _gen(11), _gen(11)
    prog = color_params(0, 0.4, None, 0, generator=g)
    torch.randperm(4, generator=r)
    assert prog == [(C_, _uniform(r, 0.6, 1.4))]
    assert torch.equal(g.get_state(), r.get_state())
    g, r = _gen(12), _gen(12)
    assert color_params(0, (1.0, 1.0), 0, (0, 0), generator=g) == []  # the permutation is still drawn
    torch.randperm(4, generator=r)
    assert torch.equal(g.get_state(), r.get_state())


def test_hue_shift_truncates_toward_zero_modulo_256():
    from fsp_amd.data.preprocess import color_params, hue_shift
    assert [hue_shift(f) for f in (0.0, 0.1, -0.1, 0.5, -0.5, 0.003, -0.003, -0.004)] == [0, 25, 231, 127, 129, 0, 0,
                                                                                          255]
    seen = set()
    for seed in range(40):
        g, r = _gen(seed), _gen(seed)
        (op, shift), = color_params(0, 0, 0, 0.5, generator=g)
        torch.randperm(4, generator=r)
        f = _uniform(r, -0.5, 0.5)
        assert op == H_ and shift == (int(abs(f) * 255) if f >= 0 else (256 - int(abs(f) * 255)) % 256)
        seen.add(f < 0)
    assert seen == {False, True}


def test_color_params_rejects_what_torchvision_rejects():
    from fsp_amd.data.preprocess import color_params
    for bad in ((-0.1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -0.5, 0), (0, 0, 0, -0.1), (0, 0, 0, 0.6),
                (0, 0, 0, (-0.6, 0.1)), ((1.2, 0.8), 0, 0, 0), ((-0.5, 1.0), 0, 0, 0)):
        g = _gen(1)
        with pytest.raises(ValueError):
            color_params(*bad, generator=g)
        assert torch.equal(g.get_state(), _gen(1).get_state())  # rejected before any draw
    with pytest.raises(TypeError):
        color_params((0.1, 0.2, 0.3), 0, 0, 0)


def _cfg(transforms=(), **inp):
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    cfg.INPUT.TRANSFORMS = ["random_resized_crop", "random_flip", "normalize"] + list(transforms)
    for k, v in inp.items():
        cfg.INPUT[k] = v
    return cfg


def _simclr_cfg(flag, name="CoOp"):
    cfg = _cfg()
    cfg.TRAINER.NAME = name
    cfg.TRAINER.COOP.LOSS_TYPE = "simclr"
    cfg.TRAINER.IVLP.SIMCLR_ALPHA = 0.5
    cfg.NATIVE.SIMCLR_COLOR = flag
    return cfg


SIZES = [(80, 60), (61, 97), (120, 120), (64, 200)]


def test_config_defaults():
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    i = cfg.INPUT
    assert (i.COLORJITTER_B, i.COLORJITTER_C, i.COLORJITTER_S, i.COLORJITTER_H) == (0.4, 0.4, 0.4, 0.1)
    assert i.RGS_P == 0.2 and i.COLORJITTER_P == 1.0
    assert cfg.NATIVE.SIMCLR_COLOR is False and cfg.NATIVE.SIMCLR_COLOR_P == 0.8
    assert "colorjitter" not in i.TRANSFORMS and "randomgrayscale" not in i.TRANSFORMS


def test_gpu_transform_accepts_the_colour_names_only():
    from fsp_amd.data.preprocess import GpuTransform
    t = GpuTransform(_cfg(["colorjitter", "randomgrayscale"]), True, "cpu", _gen(0))
    assert t.jitter == ((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1)) and t.jitter_p == 1.0 and t.gray_p == 0.2
    t = GpuTransform(_cfg(["colorjitter"], COLORJITTER_B=0.0, COLORJITTER_H=0.5), True, "cpu", _gen(0))
    assert t.jitter[0] is None and t.jitter[3] == (-0.5, 0.5) and t.gray_p is None
    for bad in ("gaussian_blur", "randaugment", "cutout"):
        with pytest.raises(NotImplementedError):
            GpuTransform(_cfg(["colorjitter", bad]), True, "cpu")
    with pytest.raises(ValueError):
        GpuTransform(_cfg(["colorjitter"], COLORJITTER_H=0.7), True, "cpu")
    # the test transform has no colour stage
    t = GpuTransform(_cfg(["colorjitter", "randomgrayscale"]), False, "cpu")
    assert t.jitter is None and t.gray_p is None and t.plan(80, 60).color == []


def test_draw_order_per_image_replayed_by_hand():
    """crop, flip, RandomApply coin (only when p < 1), jitter, grayscale coin -- image-major over views."""
    from fsp_amd.data.preprocess import GpuTransform, color_params, train_plan
    for p_apply in (1.0, 0.6):
        t = GpuTransform(_cfg(["colorjitter", "randomgrayscale"], COLORJITTER_P=p_apply, RGS_P=0.5), True, "cpu",
                         _gen(7))
        plans = t.plans(SIZES, views=2)
        r = _gen(7)
        kinds = set()
        for k, (w, h) in enumerate(s for s in SIZES for _ in range(2)):
            ref = train_plan(w, h, 32, generator=r)
            prog = []
            if p_apply >= 1.0 or not (p_apply < float(torch.rand(1, generator=r))):
                prog += color_params(0.4, 0.4, 0.4, 0.1, generator=r)
            if bool(torch.rand(1, generator=r) < 0.5):
                prog.append((G_, 0))
            got = plans[k]
            assert (got.x0, got.y0, got.w, got.h, got.flip) == (ref.x0, ref.y0, ref.w, ref.h, ref.flip), k
            assert got.color == prog, k
            kinds.add((len(prog) >= 4, prog[-1:] == [(G_, 0)]))
        assert torch.equal(t.generator.get_state(), r.get_state())
        assert len(kinds) >= (3 if p_apply < 1.0 else 2), kinds  # the branches were all taken


def test_random_apply_costs_one_coin_per_view():
    """The same seed gives the same programs with and without COLORJITTER_P < 1, apart from the coin:
    with p just below 1 (the coin never skips) every view's draws sit one torch.rand(1) later."""
    from fsp_amd.data.preprocess import GpuTransform, color_params, train_plan
    t = GpuTransform(_cfg(["colorjitter"], COLORJITTER_P=1.0 - 1e-9), True, "cpu", _gen(4))
    plans = t.plans(SIZES)
    r = _gen(4)
    for got, (w, h) in zip(plans, SIZES):
        ref = train_plan(w, h, 32, generator=r)
        torch.rand(1, generator=r)  # the coin
        assert (got.x0, got.y0, got.w, got.h, got.flip) == (ref.x0, ref.y0, ref.w, ref.h, ref.flip)
        assert got.color == color_params(0.4, 0.4, 0.4, 0.1, generator=r) and len(got.color) == 4
    assert torch.equal(t.generator.get_state(), r.get_state())
    # p = 1: the same, without the coin
    t = GpuTransform(_cfg(["colorjitter"]), True, "cpu", _gen(4))
    plans = t.plans(SIZES)
    r = _gen(4)
    for got, (w, h) in zip(plans, SIZES):
        ref = train_plan(w, h, 32, generator=r)
        assert (got.x0, got.y0, got.w, got.h, got.flip) == (ref.x0, ref.y0, ref.w, ref.h, ref.flip)
        assert got.color == color_params(0.4, 0.4, 0.4, 0.1, generator=r)
    assert torch.equal(t.generator.get_state(), r.get_state())


@pytest.mark.parametrize("name", ["CoOp", "IVLP"])
def test_simclr_color_flag_adds_the_distortion_to_two_view_objectives(name):
    from fsp_amd.data.preprocess import GpuTransform
    t = GpuTransform(_simclr_cfg(True, name), True, "cpu", _gen(2))
    assert t.jitter == ((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1)) and t.jitter_p == 0.8 and t.gray_p == 0.2
    plans = t.plans(SIZES * 4, views=2)
    n_jit = sum(len(p.color) >= 4 for p in plans)
    n_gray = sum(p.color[-1:] == [(G_, 0)] for p in plans)
    assert 0 < n_jit < len(plans) and 0 < n_gray < len(plans)
    # not a two-view objective: the flag alone changes nothing
    cfg = _simclr_cfg(True, "CoCoOp")
    t = GpuTransform(cfg, True, "cpu", _gen(2))
    assert t.jitter is None and t.gray_p is None
    cfg = _simclr_cfg(True, "CoOp")
    cfg.TRAINER.COOP.LOSS_TYPE = "ce"
    assert GpuTransform(cfg, True, "cpu", _gen(2)).jitter is None
    # the evaluation transform never distorts
    assert GpuTransform(_simclr_cfg(True, name), False, "cpu").jitter is None


@pytest.mark.parametrize("views", [1, 2])
def test_flag_off_draws_exactly_train_plans_stream(views):
    """Guard: without the flag and the new names the plans and the generator state after a batch are
    those of train_plan called directly."""
    from fsp_amd.data.preprocess import GpuTransform, train_plan
    for cfg in (_cfg(), _simclr_cfg(False)):
        t = GpuTransform(cfg, True, "cpu", _gen(9))
        plans = t.plans(SIZES, views=views)
        r = _gen(9)
        ref = [train_plan(w, h, 32, generator=r) for w, h in SIZES for _ in range(views)]
        assert len(plans) == len(ref)
        for a, b in zip(plans, ref):
            assert (a.x0, a.y0, a.w, a.h, a.rw, a.rh, a.ox, a.oy, a.S, a.flip) == \
                   (b.x0, b.y0, b.w, b.h, b.rw, b.rh, b.ox, b.oy, b.S, b.flip)
            assert not getattr(a, "color", [])
        assert torch.equal(t.generator.get_state(), r.get_state())


def test_descriptor_packing_keeps_order_and_fp32_factors():
    from fsp_amd.data.preprocess import pack_color_programs
    f = [float(np.float32(v)) for v in (0.6, 1.4, 0.7321, 1.0)]
    progs = [[(S_, f[0]), (H_, 243), (C_, f[1]), (B_, f[2]), (G_, 0)], [], [(G_, 0)], [(H_, 0), (B_, f[3])]]
    d = pack_color_programs(progs)
    assert d.dtype == np.int32 and d.shape == (4, 12) and d.flags["C_CONTIGUOUS"]
    assert d[:, 0].tolist() == [5, 0, 1, 2]
    assert d[0, 1:6].tolist() == [S_, H_, C_, B_, G_]
    assert d[0, 6:11].view(np.float32)[[0, 2, 3]].tolist() == f[:3] and d[0, 7] == 243 and d[0, 10] == 0
    assert not d[1].any() and d[2, 1] == G_ and not d[2, 2:].any()
    assert d[3, 1:3].tolist() == [H_, B_] and d[3, 6] == 0 and d[3, 7:8].view(np.float32)[0] == 1.0
    assert not d[:, 11].any()
    with pytest.raises(ValueError):
        pack_color_programs([[(B_, 1.0)] * 6])


def test_synthetic_manager_rejects_the_colour_flag():
    from fsp_amd.data.synthetic import SyntheticDataManager
    with pytest.raises(ValueError, match="SIMCLR_COLOR"):
        SyntheticDataManager(5, 32, 4, device="cpu", two_views=True, simclr_color=True)
    assert len(SyntheticDataManager(5, 32, 4, n_batches=1, device="cpu", two_views=True).train_loader_x) == 1
