"""GPU Gaussian blur (clipk_image_color_blur, csrc/preprocess.hip) against Pillow itself
(tests/blur_util.py: ImageFilter.GaussianBlur(radius=sigma)): byte equality on the uint8 output,
bitwise equality on the fp32 output, no tolerance anywhere.

* blur alone at S in {1, 2, 7, 30, 224, 256}: fewer pixels than lanes, S * S % 4 != 0, the LDS limit,
  the in-place path; sigmas 0.1, 1.0 (r = 0), 1.5 (r = 1), 3.0 (r = 2: larger than the image at
  S = 1, 2) and 8.0 (r = 7); random, all-255, checkerboard, impulse and constant-row images;
* the five-op colour program followed by blur, and batches that mix colour + blur, colour only,
  blur only and nothing (those bitwise the resample kernel's own output);
* preprocess_batch, GpuTransform (one view, two views, with and without the colour distortion),
  the DataManager loader and one CoOp SimCLR epoch;
* the argument checks of the new entry launch nothing and copy nothing."""
import contextlib
import io

import numpy as np
import pytest
import torch

import blur_util as BU
import color_util as CU
from color_util import BRIGHTNESS, CONTRAST, GRAYSCALE, HUE, SATURATION
from fsp_amd import _native as N
from fsp_amd import ops
from fsp_amd.data import preprocess as P

pytestmark = pytest.mark.gpu

SIGMAS = [0.1, 1.0, 1.5, 3.0, 8.0]


def _f32(v):
    return float(np.float32(v))


FIVE = [(BRIGHTNESS, _f32(0.9)), (HUE, 128), (CONTRAST, _f32(1.4)), (SATURATION, _f32(0.6)), (GRAYSCALE, 0)]
FOUR = FIVE[:4]


def _run(hwc_list, programs, blur, dev, out_uint8=True):
    return P.color_batch(CU.planar(hwc_list).to(dev), programs, out_uint8=out_uint8, blur=blur).cpu()


def _reference(hwc, program, sigma):
    a = CU.pil_program(hwc, program)
    return a if sigma is None else BU.pil_blur(a, sigma)


def _check(hwc_list, programs, blur, dev):
    """uint8 bytes and normalised fp32 bits against Pillow, image by image."""
    ref = CU.planar([_reference(a, p, s) for a, p, s in zip(hwc_list, programs, blur)])
    got = _run(hwc_list, programs, blur, dev)
    bad = [(b, len(programs[b]), blur[b], int((got[b] != ref[b]).sum())) for b in range(len(hwc_list))
           if not torch.equal(got[b], ref[b])]
    print("images", len(hwc_list), "with differing bytes", bad)
    assert not bad
    gotf = _run(hwc_list, programs, blur, dev, out_uint8=False)
    assert gotf.dtype == torch.float32 and torch.equal(gotf, CU.normalize(ref))
    return got


# ---- blur alone ---------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 2, 7, 30, 224, 256])
def test_blur_alone_equals_pillow(dev, S):
    assert (3 * 224 * 224 <= 150528 < 3 * 256 * 256)  # 224: the LDS limit; 256: the in-place path
    kinds = BU.blur_images(S)
    imgs, blur, names = [], [], []
    for name, im in kinds.items():
        for sigma in SIGMAS:
            imgs.append(im), blur.append(sigma), names.append(name)
    assert len(imgs) == 30 and {P.gaussian_blur_params(s)[0] for s in SIGMAS} == {0, 1, 2, 7}
    got = _check(imgs, [[]] * len(imgs), blur, dev)
    assert got.shape == (30, 3, S, S)
    if S >= 30:  # the blur did something: the impulse spread over (2 * 3 * (r + 1) + 1)^2 pixels
        k = names.index("impulse_middle") + SIGMAS.index(1.5)
        assert int((got[k, 0] > 0).sum()) > 9 and int(got[k, 0].max()) < 255
    if S == 256:  # away from the edges the in-place path agrees with the LDS path on the same pixels
        crop = [np.ascontiguousarray(a[:224, :224]) for a in imgs[:5]]
        small = _run(crop, [[]] * 5, blur[:5], dev)
        for b, sigma in enumerate(blur[:5]):
            m = 3 * (P.gaussian_blur_params(sigma)[0] + 1)  # reach of three passes
            assert torch.equal(got[b, :, :224 - m, :224 - m], small[b, :, :224 - m, :224 - m]), sigma


def test_uniform_sigmas_and_odd_batches(dev):
    """20 seeded draws from U(0.1, 2) (r is 0 or 1, ww / fw vary) on S = 33, more images than one wave."""
    sig = [_f32(s) for s in np.random.RandomState(42).uniform(0.1, 2.0, 20)]
    rs = np.random.RandomState(9)
    imgs = [rs.randint(0, 256, size=(33, 33, 3), dtype=np.uint8) for _ in sig]
    _check(imgs, [[]] * 20, sig, dev)


# ---- colour then blur, mixed batches ------------------------------------------------------------

@pytest.mark.parametrize("S", [30, 224, 256])
def test_colour_program_then_blur(dev, S):
    rs = np.random.RandomState(S)
    imgs = [rs.randint(0, 256, size=(S, S, 3), dtype=np.uint8) for _ in range(6)]
    progs = [FIVE, FOUR, FIVE, [], [(CONTRAST, _f32(0.6))], []]
    # (sigma 0.1 would not do for image 4: on pixels that contrast 0.6 pulled into 51..178 its outer
    # weight of 0.0017 never moves a byte, in Pillow either)
    blur = [1.5, 1.0, None, 3.0, 0.5, None]
    got = _check(imgs, progs, blur, dev)
    # the unblurred images are what clipk_image_color alone gives, and blur changes the others
    plain = P.color_batch(CU.planar(imgs).to(dev), progs, out_uint8=True).cpu()
    for b, s in enumerate(blur):
        assert torch.equal(got[b], plain[b]) == (s is None), b
    assert torch.equal(got[5], CU.planar(imgs)[5])


def _source_images(seed, n, lo=60, hi=301):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, size=(int(rs.randint(lo, hi)), int(rs.randint(lo, hi)), 3), dtype=np.uint8)
            for _ in range(n)]


def test_preprocess_batch_mixed(dev):
    images = _source_images(13, 6)
    g = torch.Generator()
    g.manual_seed(3)
    plans = [P.train_plan(im.shape[1], im.shape[0], 64, generator=g) for im in images]
    progs = [[], [(HUE, 200)], FIVE, [], [], [(GRAYSCALE, 0)]]
    blur = [None, 1.2, 0.8, 2.0, None, None]  # nothing, colour + blur (twice), blur only, nothing, colour only
    plain = P.preprocess_batch(images, plans, device=str(dev))  # clipk_image_resample(out_uint8=0)
    out = P.preprocess_batch(images, plans, device=str(dev), color=progs, blur=blur).cpu()
    out8 = P.preprocess_batch(images, plans, device=str(dev), color=progs, blur=blur, out_uint8=True).cpu()
    noblur8 = P.preprocess_batch(images, plans, device=str(dev), color=progs, out_uint8=True).cpu()
    for b, (im, plan) in enumerate(zip(images, plans)):
        plan.color, plan.blur = progs[b], blur[b]
        r8, rf = BU.pil_view(im, plan)
        assert torch.equal(out8[b], r8), (b, int((out8[b] != r8).sum()))
        assert torch.equal(out[b], rf), b
        if not progs[b] and blur[b] is None:
            assert torch.equal(out[b], plain[b].cpu()), b
        assert torch.equal(out8[b], noblur8[b]) == (blur[b] is None), b
    # blur alone, no colour argument; and no blur at all: today's path, the same bits
    only = P.preprocess_batch(images, plans, device=str(dev), blur=[0.7] + [None] * 5).cpu()
    plans[0].color, plans[0].blur = [], 0.7
    assert torch.equal(only[0], BU.pil_view(images[0], plans[0])[1]) and torch.equal(only[1:], plain[1:].cpu())
    assert torch.equal(P.preprocess_batch(images, plans, device=str(dev), color=[[]] * 6, blur=[None] * 6), plain)
    with pytest.raises(ValueError):
        P.preprocess_batch(images, plans, device=str(dev), blur=blur[:5])
    with pytest.raises(ValueError):
        P.preprocess_batch(images, plans, device=str(dev), blur=[9.0] + [None] * 5)  # r = 8


# ---- argument checks ----------------------------------------------------------------------------

def test_argument_checks_launch_nothing(dev):
    lib = N.load()
    B, S = 2, 8
    pix = torch.full((B, 3, S, S), 9, dtype=torch.uint8, device=dev)
    out = torch.full((B, 3, S, S), 7, dtype=torch.uint8, device=dev)
    outf = torch.full((B, 3, S, S), 7.0, dtype=torch.float32, device=dev)
    d_prog = torch.full((B * N.COLORBLUR_DESC,), -5, dtype=torch.int32, device=dev)
    ms = torch.ones(3, dtype=torch.float32, device=dev)
    good = P.pack_color_blur_programs([[(BRIGHTNESS, 0.5)], [(HUE, 3), (GRAYSCALE, 0)]], [1.5, None])
    assert good[0, 12:].tolist() == [1, 5452595, 209715, 0] and good[1, 12] == -1

    def call(B=B, S=S, pix=ops._p(pix), prog=good, prog_dev=ops._p(d_prog), mean=ops._p(ms), std=ops._p(ms), u8=1,
             out=ops._p(out), fn=lib.clipk_image_color_blur):
        prog = prog if prog is None else np.ascontiguousarray(prog, np.int32)
        return fn(B, S, pix, None if prog is None else prog.ctypes.data, prog_dev, mean, std, u8, out, ops._stream())

    def edit(*cells):
        d = good.copy()
        for row, col, value in cells:
            d[row, col] = value
        return d

    EINVAL, ESHAPE = -1, -2
    assert call(pix=None) == EINVAL and call(prog=None) == EINVAL and call(prog_dev=None) == EINVAL
    assert call(out=None) == EINVAL and call(out=ops._p(pix)) == EINVAL
    assert call(u8=0, mean=None, out=ops._p(outf)) == EINVAL and call(u8=0, std=None, out=ops._p(outf)) == EINVAL
    assert call(B=-1) == ESHAPE and call(S=0) == ESHAPE and call(S=4097) == ESHAPE
    assert call(prog=edit((0, 0, 6))) == ESHAPE and call(prog=edit((1, 0, -1))) == ESHAPE  # program length
    assert call(prog=edit((0, 1, 0))) == EINVAL and call(prog=edit((1, 2, 6))) == EINVAL  # unknown op code
    assert call(prog=edit((0, 1, 9))) == EINVAL and call(prog=edit((1, 6, 256))) == EINVAL  # code 9, hue shift
    assert call(prog=edit((0, 6, int(np.array(-0.5, np.float32).view(np.int32))))) == EINVAL
    assert call(prog=edit((0, 12, 8))) == EINVAL and call(prog=edit((1, 12, -2))) == EINVAL  # radius
    assert call(prog=edit((0, 13, 0))) == EINVAL and call(prog=edit((0, 13, -3))) == EINVAL  # ww
    assert call(prog=edit((0, 13, (1 << 24) + 1), (0, 12, 0), (0, 14, 0))) == EINVAL  # ww > 2^24
    assert call(prog=edit((0, 14, -1))) == EINVAL  # fw
    assert call(prog=edit((0, 14, 209716))) == EINVAL  # (2r + 1) ww + 2 fw = 2^24 + 1
    assert call(prog=edit((0, 12, 2))) == EINVAL  # the same weights at a larger radius: over 2^24
    with pytest.raises(N.ClipkError):
        N.call("clipk_image_color_blur", B, S, ops._p(pix), edit((0, 12, 8)).ctypes.data, ops._p(d_prog), ops._p(ms),
               ops._p(ms), 1, ops._p(out), ops._stream())
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((outf == 7.0).all()) and bool((pix == 9).all())
    assert bool((d_prog == -5).all())  # not even the descriptor copy
    # r = -1: ww / fw are not read; B = 0 is fine and launches nothing
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((d_prog == -5).all())
    assert call(prog=edit((1, 13, -7), (1, 14, -7))) == 0
    torch.cuda.synchronize()
    assert bool((out[0] == 4).all()) and bool((out[1] == 9).all())  # brightness 0.5 of 9, blurred flat; grey
    # clipk_image_color behaves as before: 12-int descriptors, codes 6 and 9 and six ops invalid
    good12 = P.pack_color_programs([[(BRIGHTNESS, 0.5)], [(HUE, 3), (GRAYSCALE, 0)]])
    out.fill_(7)
    d_prog.fill_(-5)
    for col, value, want in ((1, 6, EINVAL), (1, 9, EINVAL), (0, 6, ESHAPE)):
        d = good12.copy()
        d[0, col] = value
        assert call(prog=d, fn=lib.clipk_image_color) == want
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((d_prog == -5).all())
    assert call(prog=good12, fn=lib.clipk_image_color) == 0
    torch.cuda.synchronize()
    assert bool((out[0] == 4).all()) and bool((out[1] == 9).all())
    assert bool((d_prog[:B * N.COLOR_DESC].cpu() == torch.from_numpy(good12.ravel())).all())
    assert bool((d_prog[B * N.COLOR_DESC:] == -5).all())  # it copies 12 ints per image, no more
    with pytest.raises(ValueError):
        P.color_batch(pix, [[], []], blur=[1.0])


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


def _replay(images, seed_or_gen, size, views, jitter_p, gray_p, blur_p, sigma=(0.1, 2.0)):
    """The draws of the chain, by hand, image-major over views: crop, flip, the colour draws (none
    when jitter_p is None), the blur coin (when p < 1), sigma (if applied) -> per view a list of
    (Pillow's fp32 view, colour program, sigma or None)."""
    if isinstance(seed_or_gen, torch.Generator):
        g = seed_or_gen
    else:
        g = torch.Generator()
        g.manual_seed(seed_or_gen)
    out = [[] for _ in range(views)]
    for im in images:
        for v in range(views):
            plan = P.train_plan(im.shape[1], im.shape[0], size, generator=g)
            if jitter_p is not None:
                if jitter_p >= 1.0 or not (jitter_p < float(torch.rand(1, generator=g))):
                    plan.color += P.color_params(0.4, 0.4, 0.4, 0.1, generator=g)
                if bool(torch.rand(1, generator=g) < gray_p):
                    plan.color.append((GRAYSCALE, 0))
            if blur_p >= 1.0 or not (blur_p < float(torch.rand(1, generator=g))):
                plan.blur = float(torch.empty(1).uniform_(sigma[0], sigma[1], generator=g))
            out[v].append((BU.pil_view(im, plan)[1], plan.color, plan.blur))
    return out


def _both_occur(refs):
    return {s is not None for _, _, s in refs} == {False, True}


def test_gpu_transform_pipeline_equals_pillow(dev):
    images = _source_images(21, 6)
    # INPUT.TRANSFORMS form, one view
    cfg = _cfg(64, False)
    cfg.INPUT.TRANSFORMS = list(cfg.INPUT.TRANSFORMS) + ["pil_gaussian_blur"]
    g = torch.Generator()
    g.manual_seed(5)
    x = P.GpuTransform(cfg, True, str(dev), g)(images).cpu()
    (ref,) = _replay(images, 5, 64, 1, None, 0.0, 0.5)
    assert x.shape == (6, 3, 64, 64) and x.dtype == torch.float32
    for b, (rf, prog, sigma) in enumerate(ref):
        assert torch.equal(x[b], rf), (b, sigma)
    assert _both_occur(ref)
    # NATIVE.SIMCLR_BLUR two-view form (TRANSFORMS untouched), alone and with the colour distortion
    for seed, color in ((6, False), (8, True)):
        cfg = _cfg(64, True, SIMCLR_BLUR=True, SIMCLR_COLOR=color)
        g = torch.Generator()
        g.manual_seed(seed)
        x1, x2 = P.GpuTransform(cfg, True, str(dev), g)(images, views=2)
        r1, r2 = _replay(images, seed, 64, 2, 0.8 if color else None, 0.2, 0.5)
        for b in range(6):
            assert torch.equal(x1[b].cpu(), r1[b][0]), (color, b, r1[b][1:])
            assert torch.equal(x2[b].cpu(), r2[b][0]), (color, b, r2[b][1:])
        assert x1._base is x2._base and x1._base.shape == (12, 3, 64, 64)  # still one output
        assert _both_occur(r1 + r2)
        if color:
            assert any(len(p) >= 4 and s is not None for _, p, s in r1 + r2)  # jitter, then blur


def _data_manager(images, size, dev, **native):
    from fsp_amd.clip import synth
    from fsp_amd.data.fewshot import Datum
    from fsp_amd.data.manager import DataManager
    names = synth.synthetic_classnames(4)  # names the fallback tokenizer table holds
    cfg = _cfg(size, True, **native)
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 3
    cfg.DATALOADER.TRAIN_X.SAMPLER = "SequentialSampler"

    class DS:
        train_x = [Datum(impath=str(i), label=i % 4, classname=names[i % 4]) for i in range(6)]
        test = train_x
        classnames = names
        lab2cname = dict(enumerate(names))
        num_classes = 4

    return cfg, DataManager(cfg, DS, dev, reader=lambda path: images[int(path)], num_workers=0)


def test_data_manager_blurred_views(dev):
    images = _source_images(22, 6)
    torch.manual_seed(3)  # augment_generator seeds from torch's seed
    _, dm_on = _data_manager(images, 64, dev, SIMCLR_BLUR=True)
    _, dm_off = _data_manager(images, 64, dev)
    g = torch.Generator()
    g.set_state(dm_on.train_loader_x.transform.generator.get_state())
    on, off = list(dm_on.train_loader_x), list(dm_off.train_loader_x)
    assert len(on) == len(off) == 2
    seen = []
    for k, a in enumerate(on):
        assert a["img"] is a["img1"] and a["img1"].shape == a["img2"].shape == (3, 3, 64, 64)
        assert a["img1"]._base is a["img2"]._base and a["img1"]._base.shape == (6, 3, 64, 64)
        r1, r2 = _replay(images[3 * k:3 * k + 3], g, 64, 2, None, 0.0, 0.5)
        for i in range(3):
            assert torch.equal(a["img1"][i].cpu(), r1[i][0]), (k, i, r1[i][2])
            assert torch.equal(a["img2"][i].cpu(), r2[i][0]), (k, i, r2[i][2])
        seen += r1 + r2
    assert _both_occur(seen)
    # evaluation is not blurred
    assert torch.equal(next(iter(dm_on.test_loader))["img"], next(iter(dm_off.test_loader))["img"])


def test_coop_simclr_trains_on_blurred_colour_views(dev, tmp_path):
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    images = _source_images(23, 6, 40, 90)
    torch.manual_seed(4)
    cfg, dm = _data_manager(images, 32, dev, SIMCLR_BLUR=True, SIMCLR_COLOR=True)
    assert dm.train_loader_x.transform.blur_sigma == (0.1, 2.0) and dm.train_loader_x.transform.jitter is not None
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
