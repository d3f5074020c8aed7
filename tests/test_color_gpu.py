"""GPU colour stage (clipk_image_color, csrc/preprocess.hip) against Pillow itself
(tests/color_util.py): byte equality on the uint8 output, bitwise equality on the fp32 output,
no tolerance anywhere.

* the colour arithmetic over all 2^24 RGB triples (S = 224 images: the LDS-resident path);
* contrast's mean-L rounding at exactly k + 0.5 and one level below;
* program order (every permutation of the four jitter ops, with and without grayscale), mixed
  batches, empty programs bitwise the resample kernel's own fp32;
* shapes: fewer pixels than lanes, S * S % 4 != 0, the LDS limit, the in-place path;
* argument checks; the GpuTransform pipeline, the DataManager loader and two training steps."""
import contextlib
import functools
import io
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

import color_util as CU
from color_util import BRIGHTNESS, CONTRAST, GRAYSCALE, HUE, SATURATION
from fsp_amd import _native as N
from fsp_amd import ops
from fsp_amd.data import preprocess as P

pytestmark = pytest.mark.gpu


def _f32(v):
    return float(np.float32(v))


def _seeded_factor():
    g = torch.Generator()
    g.manual_seed(77)
    return float(torch.empty(1).uniform_(0.6, 1.4, generator=g))


FACTORS = [_f32(0.6), 1.0, _f32(1.4), _seeded_factor()]


def _run(hwc_list, programs, dev, out_uint8=True):
    """images (uint8 [S, S, 3] each) through clipk_image_color -> CPU tensor [B, 3, S, S]"""
    return P.color_batch(CU.planar(hwc_list).to(dev), programs, out_uint8=out_uint8).cpu()


def _check(hwc_list, programs, dev):
    """uint8 bytes and normalised fp32 bits against Pillow, image by image."""
    ref = CU.planar([CU.pil_program(a, p) for a, p in zip(hwc_list, programs)])
    got = _run(hwc_list, programs, dev)
    for b in range(len(hwc_list)):
        assert torch.equal(got[b], ref[b]), (b, programs[b], int((got[b] != ref[b]).sum()))
    gotf = _run(hwc_list, programs, dev, out_uint8=False)
    assert gotf.dtype == torch.float32 and torch.equal(gotf, CU.normalize(ref))
    return got


# ---- exhaustive colour arithmetic ---------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _triples():
    """All 2^24 triples as 335 images of S = 224 (host uint8 [335, 224, 224, 3], tail zero) and the
    same pixels as one 4096 x 4096 PIL image for the reference (these ops are per pixel)."""
    imgs = CU.all_triples(224)
    flat = imgs.reshape(-1, 3)[:1 << 24].reshape(4096, 4096, 3)
    return imgs, Image.fromarray(flat)


@functools.lru_cache(maxsize=1)
def _triples_dev(dev):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(_triples()[0], (0, 3, 1, 2)))).to(dev)


EXHAUSTIVE = ([(SATURATION, f) for f in FACTORS] + [(GRAYSCALE, 0)] + [(HUE, s) for s in (1, 128, 243)])


@pytest.mark.parametrize("op,value", EXHAUSTIVE, ids=[f"op{o}-{v:g}" for o, v in EXHAUSTIVE])
def test_every_rgb_triple_equals_pillow(dev, op, value):
    imgs, pil = _triples()
    B = imgs.shape[0]
    assert B == 335 and 3 * 224 * 224 == 150528  # the LDS-resident path
    pix = _triples_dev(dev).clone()
    got = P.color_batch(pix, [[(op, value)]] * B, out_uint8=True).cpu().numpy()
    got = np.transpose(got, (0, 2, 3, 1)).reshape(-1, 3)[:1 << 24].reshape(4096, 4096, 3)
    ref = np.asarray(CU.pil_op(pil, op, value))
    bad = int((got != ref).sum())
    print("op", op, "value", value, "bytes differing", bad)
    assert bad == 0


def test_brightness_all_values_equals_pillow(dev):
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.dstack([v, v[::-1], v.T])
    _check([img] * len(FACTORS), [[(BRIGHTNESS, f)] for f in FACTORS], dev)


# ---- contrast: the image-wide mean --------------------------------------------------------------

def _two_greys(k, n_hi):
    """S = 8: n_hi pixels grey k + 1, the rest grey k (mean L = k + n_hi / 64), shuffled."""
    flat = np.full(64, k, np.uint8)
    flat[:n_hi] = k + 1
    np.random.RandomState(k).shuffle(flat)
    g = flat.reshape(8, 8)
    return np.dstack([g, g, g])


@pytest.mark.parametrize("f", [_f32(0.6), _f32(1.4)])
def test_contrast_mean_rounding(dev, f):
    imgs = []
    for k in (0, 10, 127, 200, 254):
        imgs += [_two_greys(k, 32), _two_greys(k, 31)]  # mean exactly k + 0.5 -> k + 1; one level below -> k
    imgs.append(np.random.RandomState(5).randint(0, 256, size=(8, 8, 3), dtype=np.uint8))
    from PIL import ImageStat
    means = [int(ImageStat.Stat(Image.fromarray(a).convert("L")).mean[0] + 0.5) for a in imgs[:4]]
    assert means == [1, 0, 11, 10]  # the cases are what they claim to be
    _check(imgs, [[(CONTRAST, f)]] * len(imgs), dev)


# ---- program order ------------------------------------------------------------------------------

def _random_images(seed, n, S):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, size=(S, S, 3), dtype=np.uint8) for _ in range(n)]


JITTER = {BRIGHTNESS: _f32(1.3), CONTRAST: _f32(0.7), SATURATION: _f32(1.35), HUE: 243}


@pytest.mark.parametrize("gray", [False, True])
def test_every_op_order(dev, gray):
    perms = list(itertools.permutations([BRIGHTNESS, CONTRAST, SATURATION, HUE]))
    assert len(perms) == 24
    progs = [[(op, JITTER[op]) for op in perm] + ([(GRAYSCALE, 0)] if gray else []) for perm in perms]
    imgs = _random_images(31, 24, 32)
    got = _check(imgs, progs, dev)
    if not gray:  # the order matters: the 24 programs on ONE image do not all agree
        same = _run([imgs[0]] * 24, progs, dev)
        assert len({same[b].numpy().tobytes() for b in range(24)}) > 1
    else:
        assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])


def _source_images(seed, n, lo=60, hi=301):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, size=(int(rs.randint(lo, hi)), int(rs.randint(lo, hi)), 3), dtype=np.uint8)
            for _ in range(n)]


def test_mixed_batch_and_empty_programs(dev):
    images = _source_images(13, 6)
    g = torch.Generator()
    g.manual_seed(3)
    plans = [P.train_plan(im.shape[1], im.shape[0], 64, generator=g) for im in images]
    five = [(SATURATION, _f32(0.8)), (BRIGHTNESS, _f32(1.2)), (CONTRAST, _f32(1.3)), (HUE, 9), (GRAYSCALE, 0)]
    progs = [[], [(HUE, 200)], five, [], [(CONTRAST, _f32(0.6))], [(GRAYSCALE, 0)]]
    plain = P.preprocess_batch(images, plans, device=str(dev))  # clipk_image_resample(out_uint8=0)
    out = P.preprocess_batch(images, plans, device=str(dev), color=progs).cpu()
    out8 = P.preprocess_batch(images, plans, device=str(dev), color=progs, out_uint8=True).cpu()
    for b, (im, plan, prog) in enumerate(zip(images, plans, progs)):
        plan.color = prog
        r8, rf = CU.pil_view(im, plan)
        assert torch.equal(out8[b], r8), (b, prog)
        assert torch.equal(out[b], rf), (b, prog)
        if not prog:
            assert torch.equal(out[b], plain[b].cpu()), b
    # all programs empty: today's path, the same bits
    assert torch.equal(P.preprocess_batch(images, plans, device=str(dev), color=[[]] * 6), plain)
    with pytest.raises(ValueError):
        P.preprocess_batch(images, plans, device=str(dev), color=progs[:5])


# ---- shapes -------------------------------------------------------------------------------------

FIVE = [(BRIGHTNESS, _f32(0.9)), (HUE, 128), (CONTRAST, _f32(1.4)), (SATURATION, _f32(0.6)), (GRAYSCALE, 0)]
FOUR = FIVE[:4]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [7, 30, 224, 256])
def test_shapes_on_both_paths(dev, S, B):
    imgs = _random_images(100 + S, B, S)
    progs = [FIVE if b % 2 == 0 else FOUR for b in range(B)]
    got = _check(imgs, progs, dev)
    if S == 256:  # the in-place path agrees with the LDS path on the same pixels
        crop = [np.ascontiguousarray(a[:224, :224]) for a in imgs]
        hue_only = [[(HUE, 77), (SATURATION, _f32(1.2))]] * B
        big, small = _run(imgs, hue_only, dev), _run(crop, hue_only, dev)
        assert torch.equal(big[:, :, :224, :224], small)
    assert got.shape == (B, 3, S, S)


# ---- argument checks ----------------------------------------------------------------------------

def test_argument_checks_launch_nothing(dev):
    lib = N.load()
    B, S = 2, 8
    pix = torch.full((B, 3, S, S), 9, dtype=torch.uint8, device=dev)
    out = torch.full((B, 3, S, S), 7, dtype=torch.uint8, device=dev)
    outf = torch.full((B, 3, S, S), 7.0, dtype=torch.float32, device=dev)
    d_prog = torch.full((B * N.COLOR_DESC,), -1, dtype=torch.int32, device=dev)
    ms = torch.ones(3, dtype=torch.float32, device=dev)
    good = P.pack_color_programs([[(BRIGHTNESS, 0.5)], [(HUE, 3), (GRAYSCALE, 0)]])

    def call(B=B, S=S, pix=ops._p(pix), prog=good, prog_dev=ops._p(d_prog), mean=ops._p(ms), std=ops._p(ms), u8=1,
             out=ops._p(out)):
        prog = prog if prog is None else np.ascontiguousarray(prog, np.int32)
        return lib.clipk_image_color(B, S, pix, None if prog is None else prog.ctypes.data, prog_dev, mean, std, u8,
                                     out, ops._stream())

    def edit(row, col, value):
        d = good.copy()
        d[row, col] = value
        return d

    EINVAL, ESHAPE = -1, -2
    assert call(pix=None) == EINVAL and call(prog=None) == EINVAL and call(prog_dev=None) == EINVAL
    assert call(out=None) == EINVAL and call(out=ops._p(pix)) == EINVAL
    assert call(u8=0, mean=None, out=ops._p(outf)) == EINVAL and call(u8=0, std=None, out=ops._p(outf)) == EINVAL
    assert call(B=-1) == ESHAPE and call(S=0) == ESHAPE and call(S=-3) == ESHAPE
    assert call(prog=edit(0, 0, 6)) == ESHAPE and call(prog=edit(1, 0, -1)) == ESHAPE  # program length
    assert call(prog=edit(0, 1, 0)) == EINVAL and call(prog=edit(1, 2, 6)) == EINVAL  # unknown op code
    assert call(prog=edit(1, 6, 256)) == EINVAL and call(prog=edit(1, 6, -1)) == EINVAL  # hue shift
    for bad in (-0.5, float("nan"), float("inf")):
        assert call(prog=edit(0, 6, int(np.array(bad, np.float32).view(np.int32)))) == EINVAL
    with pytest.raises(N.ClipkError):
        N.call("clipk_image_color", B, S, ops._p(pix), edit(0, 1, 9).ctypes.data, ops._p(d_prog), ops._p(ms),
               ops._p(ms), 1, ops._p(out), ops._stream())
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((outf == 7.0).all()) and bool((pix == 9).all())
    assert bool((d_prog == -1).all())  # not even the descriptor copy
    # codes past the program's length are not read; B = 0 is fine and launches nothing
    assert call(prog=edit(0, 2, 99)) == 0
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert bool((out[0] == 4).all()) and bool((out[1] == 9).all())  # brightness 0.5 of 9; grey stays grey
    with pytest.raises(ValueError):
        P.color_batch(pix.float(), [[], []])
    with pytest.raises(ValueError):
        P.color_batch(pix, [[]])


# ---- pipeline, loader, training -----------------------------------------------------------------

def _cfg(size, two_view, **native):
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (size, size)
    if two_view:
        cfg.TRAINER.NAME = "CoOp"
        cfg.TRAINER.COOP.LOSS_TYPE = "simclr"
    for k, v in native.items():
        cfg.NATIVE[k] = v
    return cfg


def _replay(images, seed_or_gen, size, views, jitter_p, gray_p):
    """The draws of the chain, by hand, image-major over views: crop, flip, RandomApply coin (when
    p < 1), jitter, grayscale coin -> the Pillow reference of every view, as (uint8, fp32) lists."""
    if isinstance(seed_or_gen, torch.Generator):
        g = seed_or_gen
    else:
        g = torch.Generator()
        g.manual_seed(seed_or_gen)
    out = [[] for _ in range(views)]
    for im in images:
        for v in range(views):
            plan = P.train_plan(im.shape[1], im.shape[0], size, generator=g)
            if jitter_p >= 1.0 or not (jitter_p < float(torch.rand(1, generator=g))):
                plan.color += P.color_params(0.4, 0.4, 0.4, 0.1, generator=g)
            if bool(torch.rand(1, generator=g) < gray_p):
                plan.color.append((GRAYSCALE, 0))
            out[v].append((CU.pil_view(im, plan)[1], plan.color))
    return out


def test_gpu_transform_pipeline_equals_pillow(dev):
    images = _source_images(21, 6)
    # INPUT.TRANSFORMS form, one view
    cfg = _cfg(64, False)
    cfg.INPUT.TRANSFORMS = list(cfg.INPUT.TRANSFORMS) + ["colorjitter", "randomgrayscale"]
    cfg.INPUT.RGS_P = 0.5
    g = torch.Generator()
    g.manual_seed(5)
    x = P.GpuTransform(cfg, True, str(dev), g)(images).cpu()
    (ref,) = _replay(images, 5, 64, 1, 1.0, 0.5)
    assert x.shape == (6, 3, 64, 64) and x.dtype == torch.float32
    for b, (rf, prog) in enumerate(ref):
        assert torch.equal(x[b], rf), (b, prog)
    assert {p[-1:] == [(GRAYSCALE, 0)] for _, p in ref} == {False, True}
    # NATIVE.SIMCLR_COLOR two-view form (TRANSFORMS untouched)
    cfg = _cfg(64, True, SIMCLR_COLOR=True)
    g = torch.Generator()
    g.manual_seed(6)
    x1, x2 = P.GpuTransform(cfg, True, str(dev), g)(images, views=2)
    r1, r2 = _replay(images, 6, 64, 2, 0.8, 0.2)
    for b in range(6):
        assert torch.equal(x1[b].cpu(), r1[b][0]), (b, r1[b][1])
        assert torch.equal(x2[b].cpu(), r2[b][0]), (b, r2[b][1])
    assert x1._base is x2._base and x1._base.shape == (12, 3, 64, 64)  # still one output
    assert any(len(p) >= 4 for _, p in r1 + r2)


def _data_manager(images, size, color, dev):
    from fsp_amd.clip import synth
    from fsp_amd.data.fewshot import Datum
    from fsp_amd.data.manager import DataManager
    names = synth.synthetic_classnames(4)  # names the fallback tokenizer table holds
    cfg = _cfg(size, True, SIMCLR_COLOR=color)
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 3
    cfg.DATALOADER.TRAIN_X.SAMPLER = "SequentialSampler"

    class DS:
        train_x = [Datum(impath=str(i), label=i % 4, classname=names[i % 4]) for i in range(6)]
        test = train_x
        classnames = names
        lab2cname = dict(enumerate(names))
        num_classes = 4

    return cfg, DataManager(cfg, DS, dev, reader=lambda path: images[int(path)], num_workers=0)


def test_data_manager_colour_views(dev):
    images = _source_images(22, 6)
    torch.manual_seed(3)  # augment_generator seeds from torch's seed
    _, dm_on = _data_manager(images, 64, True, dev)
    _, dm_off = _data_manager(images, 64, False, dev)
    g = torch.Generator()
    g.set_state(dm_on.train_loader_x.transform.generator.get_state())
    on, off = list(dm_on.train_loader_x), list(dm_off.train_loader_x)
    assert len(on) == len(off) == 2
    for k, (a, b) in enumerate(zip(on, off)):
        assert a["img"] is a["img1"] and a["img1"].shape == a["img2"].shape == (3, 3, 64, 64)
        assert a["img1"]._base is a["img2"]._base and a["img1"]._base.shape == (6, 3, 64, 64)
        assert not torch.equal(a["img1"], b["img1"]) and not torch.equal(a["img2"], b["img2"])
        r1, r2 = _replay(images[3 * k:3 * k + 3], g, 64, 2, 0.8, 0.2)
        for i in range(3):
            assert torch.equal(a["img1"][i].cpu(), r1[i][0]), (k, i, r1[i][1])
            assert torch.equal(a["img2"][i].cpu(), r2[i][0]), (k, i, r2[i][1])
    # evaluation is not distorted
    assert torch.equal(next(iter(dm_on.test_loader))["img"], next(iter(dm_off.test_loader))["img"])


def test_coop_simclr_trains_on_colour_views(dev, tmp_path):
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    images = _source_images(23, 6, 40, 90)
    torch.manual_seed(4)
    cfg, dm = _data_manager(images, 32, True, dev)
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.OPTIM.MAX_EPOCH = 1
    cfg.TEST.NO_TEST = True
    c = cfg.TRAINER.COOP
    c.N_CTX, c.PREC = 4, "fp32"
    cfg.NATIVE.FUSED_SIMCLR = True
    with contextlib.redirect_stdout(io.StringIO()):
        tr = TRAINER_REGISTRY.get("CoOp")(cfg, dm=dm)
    ctx0 = tr.model.prompt_learner.ctx.detach().clone()
    losses = []
    fb = tr.forward_backward
    tr.forward_backward = lambda b: losses.append(float(fb(b)["loss"])) or {"loss": losses[-1]}
    with contextlib.redirect_stdout(io.StringIO()):
        tr.epoch = 0
        tr.run_epoch()
    assert len(losses) == 2 and np.isfinite(losses).all()
    ctx1 = tr.model.prompt_learner.ctx.detach()
    assert torch.isfinite(ctx1).all() and not torch.equal(ctx1, ctx0)
