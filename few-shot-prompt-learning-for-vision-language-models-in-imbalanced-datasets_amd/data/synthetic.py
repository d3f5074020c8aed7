"""Synthetic DataManager with the Dassl surface the trainers read
(``dm.dataset.classnames``, ``dm.dataset.lab2cname``, ``dm.train_loader_x``,
``dm.test_loader``; batches are dicts {"img", "label"}, plus {"img1", "img2"} with
``two_views`` or {"y_a", "y_b", "lam"} with ``mixup_alpha``; data_manager.py:55-162,234-263).

Images are seeded U[0,1) CLIP-normalised tensors, generated once and
kept resident on the device (no decode/augment in the timed region). Labels follow the
imbalanced per-class shot list when given (PER_CLASS_SHOTS), e.g. the repo's
ImageNet-LT setting [16]*500 + [1]*500 (scripts/coop/train.sh:56).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..clip import synth
from .manager import draw_mix


class _Dataset:
    def __init__(self, classnames):
        self.classnames = classnames
        self.lab2cname = {i: c for i, c in enumerate(classnames)}
        self.num_classes = len(classnames)


VIEW2_SEED = 500_000  # offset of the second view's image seed from its batch's (two_views)
MIX_SEED = 700_000  # offset of the mixup stream's seed (mixup_alpha)


class SyntheticDataManager:
    def __init__(self, n_cls, resolution, batch_size, n_batches=2, test_batch=100, n_test=0,
                 per_class_shots=None, device="cuda", seed=1, rank=0, n_test_device=0, two_views=False,
                 mixup_alpha=None, simclr_color=False):
        """simclr_color (NATIVE.SIMCLR_COLOR of the real loader): rejected -- the synthetic images are
        normalised noise, not uint8 pixels a colour op is defined on.
        mixup_alpha (not None): every training batch is mixed as data/manager.py GpuLoader mixes
        them (draw_mix from a generator seeded MIX_SEED + seed + 7919 * rank, one draw per batch in
        batch order; ops.mixup_images): "img" the mixed images, "y_a" (= "label", kept), "y_b",
        "lam" (a Python float). Not together with two_views.
        two_views: every training batch also carries "img1" (the same tensor as "img") and
        "img2", a second set of images drawn from the batch's seed + VIEW2_SEED (the SimCLR
        objectives, data/manager.py two_views; synthetic noise has no augmentation to share, so
        the views are two independent draws).
        n_test: test images made on the host (numpy RandomState, as the fixtures);
        n_test_device: a large test set drawn directly in HBM (torch generator on the
        device; U[0,1) then CLIP-normalised), e.g. the 50,000-image eval timing set of
        SURVEY §8(d) -- 30 GB at 224 px fp32, resident, every image distinct."""
        if two_views and mixup_alpha is not None:
            raise ValueError("two_views batches are not mixed")
        if simclr_color:
            raise ValueError("synthetic views are normalised noise, not uint8 pixels: the colour distortion "
                             "(NATIVE.SIMCLR_COLOR) needs the DataManager's GPU transform")
        self.dataset = _Dataset(synth.synthetic_classnames(n_cls))
        dev = torch.device(device)
        rs = np.random.RandomState(1000 + seed + 7919 * rank)
        if per_class_shots:
            pool = np.repeat(np.arange(n_cls), per_class_shots)
        else:
            pool = np.arange(n_cls)
        self.train_loader_x = []
        mix_gen = torch.Generator()
        mix_gen.manual_seed(MIX_SEED + seed + 7919 * rank)
        for i in range(n_batches):
            img = synth.make_images(batch_size, resolution, seed=seed + 31 * i + 7919 * rank)
            lab = rs.choice(pool, size=batch_size).astype(np.int64)
            batch = {"img": torch.from_numpy(img).to(dev), "label": torch.from_numpy(lab).to(dev)}
            if two_views:
                img2 = synth.make_images(batch_size, resolution, seed=seed + 31 * i + 7919 * rank + VIEW2_SEED)
                batch["img1"] = batch["img"]
                batch["img2"] = torch.from_numpy(img2).to(dev)
            if mixup_alpha is not None:
                lam, perm = draw_mix(float(mixup_alpha), batch_size, mix_gen)
                batch["img"], batch["y_b"] = ops.mixup_images(batch["img"], perm, lam, batch["label"])
                batch["y_a"], batch["lam"] = batch["label"], lam
            self.train_loader_x.append(batch)
        self.test_loader = []
        for i in range(0, n_test, test_batch):
            b = min(test_batch, n_test - i)
            img = synth.make_images(b, resolution, seed=10_000 + seed + i + 7919 * rank)
            lab = rs.randint(0, n_cls, size=b).astype(np.int64)
            self.test_loader.append({"img": torch.from_numpy(img).to(dev),
                                     "label": torch.from_numpy(lab).to(dev)})
        if n_test_device:
            g = torch.Generator(device=dev)
            g.manual_seed(20_000 + seed + 7919 * rank)
            mean = torch.tensor(synth.CLIP_MEAN, device=dev).view(1, 3, 1, 1)
            std = torch.tensor(synth.CLIP_STD, device=dev).view(1, 3, 1, 1)
            for i in range(0, n_test_device, test_batch):
                b = min(test_batch, n_test_device - i)
                img = torch.rand((b, 3, resolution, resolution), generator=g, device=dev).sub_(mean).div_(std)
                lab = torch.randint(0, n_cls, (b,), generator=g, device=dev)
                self.test_loader.append({"img": img, "label": lab})
        self.val_loader = None
