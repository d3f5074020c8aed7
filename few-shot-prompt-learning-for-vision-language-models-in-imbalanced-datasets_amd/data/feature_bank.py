"""FeatureBank: the image features of a training set, stored once and served as batches
(LinearProbeCLIP with TRAINER.LINEAR_PROBE.CACHE_FEATURES: the frozen encoder runs in the first
epoch only). Pure torch, on whatever device the features live on."""
from __future__ import annotations

import torch


class FeatureBank:
    def __init__(self):
        self._feat, self._labels = [], []
        self._all = None

    def add(self, feat, labels):
        """Store one batch (feat [n, E], labels [n]); its boundary is remembered."""
        if feat.dim() != 2 or labels.shape != (feat.shape[0],):
            raise ValueError(f"add needs feat [n, E] and labels [n], got {tuple(feat.shape)} and "
                             f"{tuple(labels.shape)}")
        if self._feat and (feat.shape[1] != self._feat[0].shape[1] or feat.device != self._feat[0].device):
            raise ValueError("every stored batch must have one width and one device")
        self._feat.append(feat.detach().clone())
        self._labels.append(labels.detach().clone())
        self._all = None

    def __len__(self):
        return sum(f.shape[0] for f in self._feat)

    @property
    def num_stored_batches(self):
        return len(self._feat)

    def num_batches(self, batch_size, shuffle, drop_last):
        if not shuffle:
            return len(self._feat)
        n = len(self)
        return n // batch_size if drop_last else (n + batch_size - 1) // batch_size

    def batches(self, batch_size, shuffle, drop_last):
        """Yield (feat, labels). shuffle: one torch.randperm of the global RNG over all stored rows,
        cut into batch_size rows (a short last batch dropped with drop_last). Not shuffle: the stored
        batches in their stored order, with their stored boundaries (batch_size and drop_last do
        not apply)."""
        if not shuffle:
            yield from zip(self._feat, self._labels)
            return
        if not self._feat:
            return
        if self._all is None:
            self._all = (torch.cat(self._feat), torch.cat(self._labels))
        feat, labels = self._all
        n = feat.shape[0]
        perm = torch.randperm(n).to(feat.device)
        stop = n - n % batch_size if drop_last else n
        for i in range(0, stop, batch_size):
            idx = perm[i:i + batch_size]
            yield feat[idx], labels[idx]
