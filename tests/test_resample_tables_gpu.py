"""GPU: the resample tables built on the device (resample_tables_kernel, csrc/preprocess.hip) against
the block data/preprocess.py _tables builds on the host, and the pixels they give against the host
tables' and against Pillow itself. Bitwise everywhere; no tolerance."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from fsp_amd import _native as N
from fsp_amd import ops
from fsp_amd.data import preprocess as P

pytestmark = pytest.mark.gpu

INS = (1, 2, 3, 16, 61, 223, 224, 225, 500, 699)
OUTS = (1, 7, 32, 224)
CANARY, GUARD = 0x5A5A5A5A, 64


def test_kernel_block_equals_host_tables(dev):
    """Whole axes in -> out for every pair (both tables of a record; S differs between records of the
    one launch) and the cropped window of a 375 x 500 test image (resized height 298, oy = 37)."""
    plans = [P.Plan(0, 0, i, i, o, o, 0, 0, o, False) for i in INS for o in OUTS]
    shapes = [(i, i) for i in INS for o in OUTS]
    crop = P.test_plan(375, 500, 224)
    assert (crop.rw, crop.rh, crop.ox, crop.oy) == (224, 298, 0, 37)
    plans.append(crop)
    shapes.append((500, 375))
    desc, tab, _ = P._tables(plans, shapes)
    desc2, par, tab_elems, _ = P._table_params(plans, shapes)
    assert np.array_equal(desc, desc2) and tab_elems == tab.size
    assert par[:, 4].max() == 2797 and par[:, 4].min() == 5  # 699 -> 1 down to an upscale
    buf = torch.full((GUARD + tab_elems + GUARD,), CANARY, dtype=torch.int32, device=dev)
    d_par = torch.from_numpy(par).to(dev)
    N.call("clipk_resample_tables", len(plans), 224, ops._p(d_par), buf.data_ptr() + 4 * GUARD, ops._stream())
    got = buf.cpu().numpy()
    assert (got[:GUARD] == CANARY).all() and (got[-GUARD:] == CANARY).all()
    bad = int((got[GUARD:-GUARD] != tab).sum())
    print("records", len(plans), "ints", tab.size, "differing", bad)
    assert bad == 0
    # argument checks launch nothing
    lib = N.load()
    buf.fill_(CANARY)
    assert lib.clipk_resample_tables(1, 224, None, buf.data_ptr(), ops._stream()) == -1
    assert lib.clipk_resample_tables(1, 224, ops._p(d_par), None, ops._stream()) == -1
    assert lib.clipk_resample_tables(-1, 224, ops._p(d_par), buf.data_ptr(), ops._stream()) == -2
    assert lib.clipk_resample_tables(1, 0, ops._p(d_par), buf.data_ptr(), ops._stream()) == -2
    assert lib.clipk_resample_tables(0, 224, ops._p(d_par), buf.data_ptr(), ops._stream()) == 0
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())


def _ref(img, plan):
    """The reference chain of tests/test_preprocess_gpu.py: Pillow + torch on the CPU."""
    im = Image.fromarray(img)
    if (plan.x0, plan.y0, plan.w, plan.h) != (0, 0) + im.size:
        im = im.crop((plan.x0, plan.y0, plan.x0 + plan.w, plan.y0 + plan.h))  # RandomResizedCrop window
    im = im.resize((plan.rw, plan.rh), Image.BICUBIC)  # a same-size resize is a copy
    im = im.crop((plan.ox, plan.oy, plan.ox + plan.S, plan.oy + plan.S))  # CenterCrop (test)
    if plan.flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    a = np.asarray(im)
    t = torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous()
    x = t.float().div(255)
    m = torch.tensor(P.MEAN, dtype=torch.float32)[:, None, None]
    s = torch.tensor(P.STD, dtype=torch.float32)[:, None, None]
    return t, x.sub_(m).div_(s)


@functools.lru_cache(maxsize=1)
def _images():
    rs = np.random.RandomState(17)
    return [rs.randint(0, 256, size=(int(rs.randint(60, 701)), int(rs.randint(60, 701)), 3), dtype=np.uint8)
            for _ in range(12)]


@pytest.mark.parametrize("S", [224, 32])
@pytest.mark.parametrize("train", [False, True])
def test_device_tables_give_the_host_tables_pixels(dev, train, S):
    imgs = _images()
    g = torch.Generator().manual_seed(5)
    plans = [P.train_plan(im.shape[1], im.shape[0], S, generator=g) if train else
             P.test_plan(im.shape[1], im.shape[0], S) for im in imgs]
    plans[0].flip = True
    for u8 in (True, False):
        host = P.preprocess_batch(imgs, plans, device=str(dev), out_uint8=u8, tables="host")
        devt = P.preprocess_batch(imgs, plans, device=str(dev), out_uint8=u8, tables="device")
        assert devt.dtype == host.dtype and torch.equal(devt, host), u8
        got = devt.cpu()
        for b, (im, p) in enumerate(zip(imgs, plans)):
            assert torch.equal(got[b], _ref(im, p)[0 if u8 else 1]), (b, u8)
    with pytest.raises(ValueError):
        P.preprocess_batch(imgs, plans, device=str(dev), tables="gpu")


def test_gpu_transform_takes_the_flag(dev):
    from fsp_amd.engine.config import get_cfg_default
    imgs = _images()[:4]
    outs = []
    for flag in (False, True):
        cfg = get_cfg_default()
        cfg.INPUT.SIZE = (32, 32)
        cfg.NATIVE.DEVICE_TABLES = flag
        g = torch.Generator().manual_seed(9)
        tr, te = P.GpuTransform(cfg, True, str(dev), g), P.GpuTransform(cfg, False, str(dev))
        assert tr.tables == te.tables == ("device" if flag else "host")
        outs.append((tr(imgs), te(imgs), g.get_state()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2], outs[1][2])
