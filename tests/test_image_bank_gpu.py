"""GPU: the image bank (NATIVE.IMAGE_BANK, data/image_bank.py) against the streamed loader. With
equal seeds the banked run yields the same bits in every batch of every epoch and leaves every RNG
where the streamed run leaves it; the reader runs once per image; the resample reads a banked image
where it lies (clipk_image_resample_at) inside the recorded bounds. Bitwise; no tolerance."""
import collections
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from fsp_amd import _native as N
from fsp_amd import ops
from fsp_amd.data import preprocess as P
from fsp_amd.data.image_bank import ImageBank

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def _images():
    rs = np.random.RandomState(41)
    return [rs.randint(0, 256, size=(int(rs.randint(20, 91)), int(rs.randint(20, 91)), 3), dtype=np.uint8)
            for _ in range(24)]


def _cfg(mode, size, bank, tables, cap_gb, sampler, batch):
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (size, size)
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = batch
    cfg.DATALOADER.TRAIN_X.SAMPLER = sampler
    cfg.NATIVE.IMAGE_BANK, cfg.NATIVE.DEVICE_TABLES, cfg.NATIVE.IMAGE_BANK_MAX_GB = bank, tables, cap_gb
    if mode == "views":
        cfg.TRAINER.NAME = "CoOp"
        cfg.TRAINER.COOP.LOSS_TYPE = "simclr"
        cfg.NATIVE.SIMCLR_COLOR = cfg.NATIVE.SIMCLR_BLUR = True
    elif mode == "mixup":
        cfg.TRAINER.NAME = "IVLP"
        cfg.TRAINER.IVLP.USE_MIXUP = True
        cfg.TRAINER.IVLP.SIMCLR_ALPHA = 0.0
        cfg.NATIVE.MIXUP = True
    return cfg


KEYS = {"plain": ("img", "label", "index"), "views": ("img1", "img2", "label", "index"),
        "mixup": ("img", "label", "index", "y_b", "lam")}


def _run(images, dev, mode, bank, tables, cap_gb=16, epochs=3, size=32, sampler="RandomSampler", batch=4, seed=11):
    """`epochs` passes over the training loader -> per epoch (batches, torch's global RNG state, the
    transform generator's state, reader calls so far per image), and the DataManager."""
    from fsp_amd.clip import synth
    from fsp_amd.data.fewshot import Datum
    from fsp_amd.data.manager import DataManager
    names = synth.synthetic_classnames(4)
    reads = collections.Counter()

    def reader(path):
        reads[int(path)] += 1
        return images[int(path)]

    class DS:
        train_x = [Datum(impath=str(i), label=i % 4, classname=names[i % 4]) for i in range(len(images))]
        test = train_x[:4]
        classnames = names
        lab2cname = dict(enumerate(names))
        num_classes = 4

    torch.manual_seed(seed)  # the sampler stream, and augment_generator seeds from it
    dm = DataManager(_cfg(mode, size, bank, tables, cap_gb, sampler, batch), DS, dev, reader=reader, num_workers=0)
    assert (dm.image_bank is not None) == bank
    dm.generator_state_before = dm.train_loader_x.transform.generator.get_state()
    out = []
    for _ in range(epochs):
        batches = [{k: b[k] for k in KEYS[mode]} for b in dm.train_loader_x]
        out.append((batches, torch.get_rng_state(), dm.train_loader_x.transform.generator.get_state(), dict(reads)))
    return out, dm


def _same(a, b):
    return torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b


def _assert_equal_runs(x, y, mode):
    assert len(x) == len(y)
    for e, ((bx, tx, gx, _), (by, ty, gy, _)) in enumerate(zip(x, y)):
        assert len(bx) == len(by) == 6
        for k, (p, q) in enumerate(zip(bx, by)):
            for key in KEYS[mode]:
                assert _same(p[key], q[key]), (e, k, key)
        assert torch.equal(tx, ty), e  # torch's global RNG (the sampler, the DataLoader's seed draw)
        assert torch.equal(gx, gy), e  # the transform's generator (crop, flip, colour, blur, mix)


@functools.lru_cache(maxsize=None)
def _streamed(dev, mode):
    """The reference run of a mode: bank off, DEVICE_TABLES on. Computed once."""
    return _run(_images(), dev, mode, bank=False, tables=True)[0]


@pytest.mark.parametrize("mode", ["plain", "views", "mixup"])
def test_bank_equals_stream(dev, mode):
    ref = _streamed(dev, mode)
    got, dm = _run(_images(), dev, mode, bank=True, tables=True)
    _assert_equal_runs(got, ref, mode)
    # the reader: once per image, in epoch 1, never after it
    assert all(n == 3 for n in ref[2][3].values()) and len(ref[2][3]) == 24
    assert got[0][3] == {k: 1 for k in range(24)} and got[1][3] == got[0][3] and got[2][3] == got[0][3]
    assert len(dm.image_bank) == 24 and len(dm.image_bank.chunks) == 1
    for k in (0, 7, 23):
        assert np.array_equal(dm.image_bank.view(k).cpu().numpy(), _images()[k])
    if mode == "views":
        assert got[0][0][0]["img1"].shape == (4, 3, 32, 32) and not torch.equal(got[0][0][0]["img1"],
                                                                                got[0][0][0]["img2"])
    if mode == "mixup":
        assert 0.0 < got[0][0][0]["lam"] < 1.0
    # the epochs differ (RandomSampler, fresh crops): the equalities above compare like with like
    assert not torch.equal(got[0][0][0]["index"], got[1][0][0]["index"])


def test_device_tables_equal_flags_off(dev):
    ref = _streamed(dev, "plain")
    off, _ = _run(_images(), dev, "plain", bank=False, tables=False)
    _assert_equal_runs(off, ref, "plain")


def test_bank_with_host_tables(dev):
    got, _ = _run(_images(), dev, "plain", bank=True, tables=False)
    _assert_equal_runs(got, _streamed(dev, "plain"), "plain")


def test_cap_holds_half_the_set(dev):
    images = _images()
    total = sum(im.size for im in images)
    got, dm = _run(images, dev, "plain", bank=True, tables=True, cap_gb=(total // 2) / float(1 << 30))
    _assert_equal_runs(got, _streamed(dev, "plain"), "plain")
    bank = dm.image_bank
    held = {k for k in range(24) if bank.has(k)}
    assert 6 <= len(held) <= 18 and bank.allocated_bytes <= total // 2
    reads = got[2][3]
    assert all(reads[k] == 1 for k in held) and all(reads[k] == 3 for k in set(range(24)) - held)


def _pil(img, plan):
    im = Image.fromarray(img).crop((plan.x0, plan.y0, plan.x0 + plan.w, plan.y0 + plan.h))
    im = im.resize((plan.rw, plan.rh), Image.BICUBIC).crop((plan.ox, plan.oy, plan.ox + plan.S, plan.oy + plan.S))
    if plan.flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    x = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous().float().div(255)
    m = torch.tensor(P.MEAN, dtype=torch.float32)[:, None, None]
    s = torch.tensor(P.STD, dtype=torch.float32)[:, None, None]
    return x.sub_(m).div_(s)


def test_geometry_equals_pillow(dev):
    """Three 500 x 375 images to 224, bank on: the upload epoch and the banked epoch against Pillow."""
    rs = np.random.RandomState(3)
    images = [rs.randint(0, 256, size=(375, 500, 3), dtype=np.uint8) for _ in range(3)]
    got, dm = _run(images, dev, "plain", bank=True, tables=True, epochs=2, size=224, sampler="SequentialSampler",
                   batch=3, seed=21)
    assert got[1][3] == {0: 1, 1: 1, 2: 1} and len(dm.image_bank) == 3
    g = torch.Generator()
    g.set_state(dm.generator_state_before)  # replay the transform's draws
    for e in range(2):
        (batch,) = got[e][0]
        assert batch["img"].shape == (3, 3, 224, 224) and batch["index"].tolist() == [0, 1, 2]
        for b, im in enumerate(images):
            plan = P.train_plan(500, 375, 224, generator=g)
            assert torch.equal(batch["img"][b].cpu(), _pil(im, plan)), (e, b)


def test_window_outside_the_recorded_size_launches_nothing(dev, monkeypatch):
    bank = ImageBank(2, dev, max_bytes=1 << 20, chunk_bytes=1 << 16)
    img = _images()[0]
    H, W = img.shape[:2]
    assert bank.add(0, img)
    res = bank.resident(0)
    assert res.shape == (H, W, 3)
    calls = []
    monkeypatch.setattr(N, "call", lambda name, *a: calls.append(name))
    for bad in (P.Plan(0, 0, W + 1, H, 32, 32, 0, 0, 32, False), P.Plan(0, 1, W, H, 32, 32, 0, 0, 32, False),
                P.Plan(-1, 0, W, H, 32, 32, 0, 0, 32, False), P.Plan(0, 0, W, H, 32, 32, 1, 0, 32, False)):
        for tables in ("host", "device"):
            with pytest.raises(ValueError, match="outside the image"):
                P.preprocess_batch([res], [bad], device=str(dev), tables=tables)
    assert calls == []
    monkeypatch.undo()
    ok = P.preprocess_batch([res], [P.Plan(0, 0, W, H, 32, 32, 0, 0, 32, False)], device=str(dev), tables="device")
    assert torch.equal(ok, P.preprocess_batch([img], [P.Plan(0, 0, W, H, 32, 32, 0, 0, 32, False)], device=str(dev)))


def test_canaries_around_chunk_tmp_and_output(dev):
    """clipk_image_resample_at on caller-laid buffers: a bank chunk between guard bytes, banked and
    uploaded images in one launch, guards around the temp rows and the output."""
    imgs = _images()[:4]
    G, S = 256, 32
    g = torch.Generator().manual_seed(8)
    plans = [P.train_plan(im.shape[1], im.shape[0], S, generator=g) for im in imgs]
    plans[1] = P.Plan(0, 0, imgs[1].shape[1], imgs[1].shape[0], S, S, 0, 0, S, True)  # the whole image, to its edges
    shapes = [im.shape[:2] for im in imgs]
    nbytes = [im.size for im in imgs]
    store = torch.full((G + sum(nbytes[:3]) + G,), 0xA5, dtype=torch.uint8, device=dev)  # guard | chunk | guard
    upload = torch.from_numpy(imgs[3].reshape(-1).copy()).to(dev)  # the fourth image is streamed
    addr, off = [], G
    for im, n in zip(imgs[:3], nbytes):
        store[off:off + n] = torch.from_numpy(im.reshape(-1).copy()).to(dev)
        addr.append(store.data_ptr() + off)
        off += n
    addr.append(upload.data_ptr())
    desc, par, tab_elems, tmp_elems = P._table_params(plans, shapes)
    desc[:, 0] = addr
    d_desc, d_par = torch.from_numpy(desc).to(dev), torch.from_numpy(par).to(dev)
    tab = torch.empty(tab_elems, dtype=torch.int32, device=dev)
    tmp = torch.full((G + tmp_elems + G,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((G + 4 * 3 * S * S + G,), 0xA5, dtype=torch.uint8, device=dev)
    N.call("clipk_resample_tables", 4, S, ops._p(d_par), ops._p(tab), ops._stream())
    N.call("clipk_image_resample_at", 4, S, int(desc[:, 11].max()), ops._p(d_desc), ops._p(tab),
           tmp.data_ptr() + G, None, None, 1, out.data_ptr() + G, ops._stream())
    torch.cuda.synchronize()
    for buf in (store, tmp, out):
        assert bool((buf[:G] == 0xA5).all()) and bool((buf[-G:] == 0xA5).all())
    for k, im in enumerate(imgs[:3]):  # the chunk itself is only read
        lo = G + sum(nbytes[:k])
        assert np.array_equal(store[lo:lo + nbytes[k]].cpu().numpy(), im.reshape(-1))
    ref = P.preprocess_batch(imgs, plans, device=str(dev), out_uint8=True)
    assert torch.equal(out[G:-G].view(4, 3, S, S), ref)
    # the entry's own argument checks
    lib = N.load()
    assert lib.clipk_image_resample_at(4, S, 1, None, ops._p(tab), ops._p(tmp), None, None, 1, ops._p(out),
                                       ops._stream()) == -1
    assert lib.clipk_image_resample_at(4, S, 1, ops._p(d_desc), ops._p(tab), ops._p(tmp), None, None, 0, ops._p(out),
                                       ops._stream()) == -1  # fp32 output needs mean / std
    assert lib.clipk_image_resample_at(4, 0, 1, ops._p(d_desc), ops._p(tab), ops._p(tmp), None, None, 1, ops._p(out),
                                       ops._stream()) == -2


class _GuardedBank(ImageBank):
    """An ImageBank whose chunks are cut out of one larger buffer, guard bytes on either side."""

    GUARD = 256

    def _new_chunk(self, size):
        self.whole = torch.full((self.GUARD + size + self.GUARD,), 0xA5, dtype=torch.uint8, device=self.device)
        return self.whole[self.GUARD:self.GUARD + size]


def test_canaries_around_a_real_bank_chunk(dev):
    """The bank's own offsets: images filled into a guarded chunk by ImageBank.add and read through
    ImageBank.resident by preprocess_batch, whole images to their edges, the last one ending at the
    chunk's last byte."""
    imgs = _images()[:5]
    size = sum(im.size for im in imgs)
    bank = _GuardedBank(5, dev, max_bytes=size, chunk_bytes=size)
    assert all(bank.add(k, im) for k, im in enumerate(imgs)) and len(bank.chunks) == 1
    assert bank.offset[4] + imgs[4].size == bank.chunks[0].numel() == size
    plans = [P.Plan(0, 0, im.shape[1], im.shape[0], 32, 32, 0, 0, 32, k % 2 == 1) for k, im in enumerate(imgs)]
    res = [bank.resident(k) for k in range(5)]
    assert res[0].address == bank.whole.data_ptr() + bank.GUARD
    for tables in ("device", "host"):
        got = P.preprocess_batch(res, plans, device=str(dev), out_uint8=True, tables=tables)
        assert torch.equal(got, P.preprocess_batch(imgs, plans, device=str(dev), out_uint8=True))
    G = bank.GUARD
    assert bool((bank.whole[:G] == 0xA5).all()) and bool((bank.whole[-G:] == 0xA5).all())
    assert np.array_equal(bank.whole[G:-G].cpu().numpy(), np.concatenate([im.reshape(-1) for im in imgs]))
