"""ImageBank: the decoded training images of a few-shot run, kept on the device (NATIVE.IMAGE_BANK).

A few-shot training set is tiny (16,000 images at 16 shots x 1000 classes: a few GB of decoded
uint8) and is walked 50-200 times, so each image is decoded and uploaded once and stays: uint8
HWC, rows packed, keyed by its position in ``train_x``.

Storage is a list of fixed-size uint8 chunk tensors that are never reallocated or copied (an
image's address is stable for the bank's life); an image never straddles a chunk. An image that
does not fit what is left of the current chunk opens the next one; when the next chunk would pass
the cap, the image is not banked (it is streamed per batch as without the bank) -- there is no
eviction. What is left of a chunk when the next one opens is given up for good (only the last
chunk takes images; with 256 MiB chunks and images under a MB that is below half a percent), and
an image larger than a chunk, or than what the cap leaves for the next chunk, is never banked.
Per image the bank records chunk, byte offset, H and W. ``banked`` is a shared-memory bool tensor,
so the DataLoader's worker processes see what the main process has stored and skip the read
(data/manager.py DatasetWrapper). Pure torch, on whatever device the chunks live on.
"""
from __future__ import annotations

import numpy as np
import torch

from .preprocess import Resident

CHUNK_BYTES = 256 << 20


class ImageBank:
    def __init__(self, n_images, device="cuda", max_bytes=16 << 30, chunk_bytes=CHUNK_BYTES):
        if n_images < 0 or max_bytes < 0 or chunk_bytes <= 0:
            raise ValueError("ImageBank needs n_images >= 0, max_bytes >= 0 and chunk_bytes > 0")
        self.device = torch.device(device)
        self.max_bytes, self.chunk_bytes = int(max_bytes), int(chunk_bytes)
        self.banked = torch.zeros(int(n_images), dtype=torch.bool).share_memory_()
        self.chunk = np.full(int(n_images), -1, np.int64)  # per image: chunk, byte offset, H, W
        self.offset = np.zeros(int(n_images), np.int64)
        self.height = np.zeros(int(n_images), np.int64)
        self.width = np.zeros(int(n_images), np.int64)
        self.chunks = []  # uint8 [chunk size] each
        self._used = 0    # bytes taken in the last chunk

    def __len__(self):
        return int(self.banked.sum())

    @property
    def allocated_bytes(self):
        return sum(int(c.numel()) for c in self.chunks)

    def has(self, index):
        return bool(self.banked[index])

    def _new_chunk(self, size):
        return torch.empty(size, dtype=torch.uint8, device=self.device)

    def _place(self, nbytes):
        """(chunk, offset) for nbytes more, opening a chunk if the cap allows; None: no room."""
        if self.chunks and self._used + nbytes <= self.chunks[-1].numel():
            return len(self.chunks) - 1, self._used
        size = min(self.chunk_bytes, self.max_bytes - self.allocated_bytes)
        if nbytes > size:
            return None
        self.chunks.append(self._new_chunk(size))
        self._used = 0
        return len(self.chunks) - 1, 0

    def add(self, index, img):
        """Store the decoded image (uint8 [H, W, 3], numpy or torch) as train_x[index]: one copy,
        straight into bank storage. True: it is banked (now or from before -- a duplicate add changes
        nothing); False: the cap is reached and nothing was stored or marked."""
        if self.has(index):
            return True
        t = torch.as_tensor(img)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("images must be uint8 [H, W, 3]")
        nbytes = int(t.numel())
        if nbytes == 0:
            return False
        place = self._place(nbytes)
        if place is None:
            return False
        c, off = place
        self.chunks[c][off:off + nbytes].copy_(t.reshape(-1), non_blocking=True)
        self._used = off + nbytes
        self.chunk[index], self.offset[index] = c, off
        self.height[index], self.width[index] = int(t.shape[0]), int(t.shape[1])
        self.banked[index] = True  # last: a worker that sees the mark finds the record complete
        return True

    def view(self, index):
        """The stored pixels, uint8 [H, W, 3], a view of the chunk."""
        if not self.has(index):
            raise KeyError(f"image {index} is not banked")
        H, W, off = int(self.height[index]), int(self.width[index]), int(self.offset[index])
        return self.chunks[int(self.chunk[index])][off:off + H * W * 3].view(H, W, 3)

    def resident(self, index):
        """The record preprocess_batch reads a banked image through: address and recorded size."""
        if not self.has(index):
            raise KeyError(f"image {index} is not banked")
        c = self.chunks[int(self.chunk[index])]
        return Resident(c.data_ptr() + int(self.offset[index]), int(self.height[index]), int(self.width[index]),
                        keep=c)

    def fetch(self, index, img):
        """What the loader hands the transform for train_x[index]: the bank's record when the image
        is banked or can be stored now (img: the decoded pixels, None when a worker skipped the read
        because the image is banked), otherwise img itself (streamed)."""
        if img is None and not self.has(index):
            raise KeyError(f"image {index} was not read and is not banked")
        if self.has(index) or self.add(index, img):
            return self.resident(index)
        return img
