"""CPU: the image bank's bookkeeping on CPU tensors (data/image_bank.py), the DatasetWrapper that
skips the read of a banked image (in the main process and in DataLoader workers), the flags'
defaults."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from fsp_amd.data.image_bank import ImageBank
from fsp_amd.data.manager import DatasetWrapper, _collate


def _img(seed, H, W):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3), dtype=np.uint8)


def test_offsets_and_chunk_boundaries():
    bank = ImageBank(8, "cpu", max_bytes=4000, chunk_bytes=1000)
    imgs = [_img(0, 10, 10), _img(1, 5, 20), _img(2, 11, 11), _img(3, 12, 12), _img(4, 4, 4)]
    assert [bank.add(k, im) for k, im in enumerate(imgs)] == [True] * 5
    # 300 + 300 + 363 = 963 of chunk 0; 432 does not fit the 37 left -> chunk 1; 48 follows it there
    assert bank.chunk[:5].tolist() == [0, 0, 0, 1, 1]
    assert bank.offset[:5].tolist() == [0, 300, 600, 0, 432]
    assert bank.height[:5].tolist() == [10, 5, 11, 12, 4] and bank.width[:5].tolist() == [10, 20, 11, 12, 4]
    assert len(bank.chunks) == 2 and all(c.numel() == 1000 and c.dtype == torch.uint8 for c in bank.chunks)
    assert len(bank) == 5 and bank.banked.tolist() == [True] * 5 + [False] * 3 and bank.banked.is_shared()
    for k, im in enumerate(imgs):
        assert np.array_equal(bank.view(k).numpy(), im), k
        r = bank.resident(k)
        assert r.shape == im.shape and r.address == bank.chunks[bank.chunk[k]].data_ptr() + bank.offset[k]
    # an image never straddles a chunk
    for k in range(5):
        assert bank.offset[k] + imgs[k].size <= bank.chunks[bank.chunk[k]].numel()
    with pytest.raises(KeyError):
        bank.view(6)
    with pytest.raises(KeyError):
        bank.resident(6)
    with pytest.raises(ValueError):
        bank.add(6, np.zeros((4, 4), np.uint8))


def test_chunks_are_never_moved_and_duplicates_change_nothing():
    bank = ImageBank(4, "cpu", max_bytes=4000, chunk_bytes=1000)
    a = _img(5, 10, 10)
    assert bank.add(0, a)
    ptr, used = bank.chunks[0].data_ptr(), bank._used
    assert bank.add(0, _img(6, 10, 10)) and bank.add(0, _img(7, 3, 3))  # duplicate adds: no-ops
    assert bank._used == used and len(bank) == 1 and np.array_equal(bank.view(0).numpy(), a)
    for k in (1, 2, 3):
        assert bank.add(k, _img(k, 15, 15))  # 675 bytes each: the first beside the 300, then a chunk apiece
    assert bank.chunks[0].data_ptr() == ptr and np.array_equal(bank.view(0).numpy(), a)
    assert bank.chunk.tolist() == [0, 0, 1, 2] and bank.offset.tolist() == [0, 300, 0, 0]
    assert bank.allocated_bytes == 3000


def test_cap_of_a_few_kb():
    bank = ImageBank(10, "cpu", max_bytes=2500, chunk_bytes=1000)
    got = [bank.add(k, _img(k, 16, 16)) for k in range(5)]  # 768 bytes each: one per chunk
    # chunks of 1000, 1000 and the 500 left under the cap, which holds no 768-byte image
    assert got == [True, True, False, False, False]
    assert bank.banked.tolist() == [True, True] + [False] * 8 and bank.allocated_bytes == 2000
    assert not bank.has(2) and bank.chunk[2] == -1
    img = _img(9, 16, 16)
    assert bank.fetch(2, img) is img  # past the cap: streamed, the host array itself
    assert bank.fetch(1, None).shape == (16, 16, 3) and bank.fetch(1, img).address == bank.resident(1).address
    with pytest.raises(KeyError):
        bank.fetch(3, None)  # a skipped read needs the image in the bank
    assert bank.add(5, _img(5, 8, 9))  # 216 bytes still fit what chunk 1 has left
    assert bank.chunk[5] == 1 and bank.offset[5] == 768
    assert not bank.add(6, _img(6, 40, 40)) and not ImageBank(1, "cpu", max_bytes=0).add(0, img)
    assert len(bank.chunks) == 2


class _Datum:
    def __init__(self, k):
        self.impath, self.label, self.domain = str(k), k % 3, 0


class _CountingReader:
    """Counts calls in a way that works across processes: one byte appended per call."""

    def __init__(self, path):
        self.path = path

    def __call__(self, impath):
        with open(self.path, "ab") as f:
            f.write(b"%c" % (65 + int(impath)))
        return _img(int(impath), 6, 7)

    def calls(self):
        return open(self.path, "rb").read() if os.path.exists(self.path) else b""


@pytest.mark.parametrize("workers", [0, 2])
def test_wrapper_skips_the_reader_for_banked_indices(tmp_path, workers):
    reader = _CountingReader(str(tmp_path / "calls"))
    bank = ImageBank(6, "cpu", max_bytes=1 << 20, chunk_bytes=1 << 12)
    for k in (1, 4):
        assert bank.add(k, _img(k, 6, 7))
    ds = DatasetWrapper([_Datum(k) for k in range(6)], reader, bank.banked)
    batches = list(DataLoader(ds, batch_size=3, num_workers=workers, collate_fn=_collate))
    imgs = [im for b in batches for im in b["img"]]
    assert [im is None for im in imgs] == [False, True, False, False, True, False]
    assert sorted(reader.calls()) == sorted(b"ACDF")
    assert torch.cat([b["index"] for b in batches]).tolist() == list(range(6))
    for k in (0, 2, 3, 5):
        assert np.array_equal(imgs[k], _img(k, 6, 7))
    # marks made after the wrapper was built are seen too (the tensor is shared, not copied)
    for k in (0, 2, 3, 5):
        assert bank.add(k, imgs[k])
    again = list(DataLoader(ds, batch_size=3, num_workers=workers, collate_fn=_collate))
    assert all(im is None for b in again for im in b["img"]) and sorted(reader.calls()) == sorted(b"ACDF")
    # without the tensor the wrapper reads as before
    plain = DatasetWrapper([_Datum(k) for k in range(6)], reader)
    assert np.array_equal(plain[4]["img"], _img(4, 6, 7)) and reader.calls().count(b"E") == 1


def test_flags_default_off():
    from fsp_amd.engine.config import get_cfg_default
    nat = get_cfg_default().NATIVE
    assert nat.DEVICE_TABLES is False and nat.IMAGE_BANK is False and nat.IMAGE_BANK_MAX_GB == 16
