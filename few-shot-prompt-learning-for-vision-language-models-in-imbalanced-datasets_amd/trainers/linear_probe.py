"""LinearProbeCLIP: a linear classifier on the frozen CLIP image features, the baseline prompt
learning is compared against.

The fork registers a trainer of this name (``trainers/linear_probe.py``), but its source
is not at hand: the keys of TRAINER.LINEAR_PROBE and the arithmetic below are THIS PACKAGE'S
definition, not a port.

    u = F.normalize(f) if NORMALIZE else f,   f = visual(image).float()   (frozen, no gradient)
    logits = scale * u W^T + b                scale = LOGIT_SCALE if > 0 else CLIP's logit scale
    loss = CE or focal (LOSS_TYPE, the meaning the key has in TRAINER.COOP)

``classifier`` = nn.Linear(E, C, bias=BIAS) in fp32 is the only trainable module and the only
registered model: a checkpoint holds ``weight`` (and ``bias``) and nothing else. INIT "zeroshot":
weight = the normalised text features of the dataset's ZeroshotCLIP template, bias 0 -- with
NORMALIZE the untrained probe scores as ZeroshotCLIP does; "zeros": both 0.

NATIVE.FUSED_PROBE: the step's head is one ProbeHeadFn call (clipk_probe_head: normalisation,
Linear, loss and the gradients of weight and bias) and inference its scoring-only form, where it
takes the inputs; off (and elsewhere) the torch composition above with CrossEntropyFn and autograd.

CACHE_FEATURES: the first epoch run trains normally and stores each batch's fp32 features and
labels in a FeatureBank (data/feature_bank.py); every later epoch draws its batches from the bank and
the image encoder does not run. With CACHE_SHUFFLE the rows are re-cut every epoch from one
torch.randperm into DATALOADER.TRAIN_X.BATCH_SIZE rows (a short last batch dropped when the bank
holds at least one full batch: the loader's rule); without it the stored batches are replayed as
stored. The cached views are whatever the loader produced in that first epoch: with random crops
one augmented view per image; test-style transforms (INPUT.TRANSFORMS ["normalize"]) give the
un-augmented features. Single process only: a bank sharded over ranks is not implemented.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import dist, ops
from ..data.feature_bank import FeatureBank
from ..engine.registry import TRAINER_REGISTRY
from ..engine.trainer import TrainerX, load_clip
from ..engine.optim import build_optimizer, build_lr_scheduler
from ..engine.metrics import LossSummary
from ._fns import CrossEntropyFn, ProbeHeadFn, probe_head_fused_ok, backward_unit
from .losses import focal_alpha
from .zsclip import CUSTOM_TEMPLATES, encode_prompts


class LinearProbeModel(nn.Module):
    def __init__(self, cfg, classnames, clip_model):
        super().__init__()
        sec = cfg.TRAINER.LINEAR_PROBE
        self.clip_model = clip_model
        for p in clip_model.parameters():
            p.requires_grad_(False)
        dev = clip_model.logit_scale.device
        n_cls, width = len(classnames), clip_model.arch.embed_dim
        self.normalize = bool(sec.NORMALIZE)
        self.scale = float(sec.LOGIT_SCALE) if sec.LOGIT_SCALE > 0 else float(clip_model.logit_scale_value)
        self.classifier = nn.Linear(width, n_cls, bias=bool(sec.BIAS)).to(device=dev, dtype=torch.float32)
        with torch.no_grad():
            if sec.INIT == "zeroshot":
                temp = CUSTOM_TEMPLATES.get(cfg.DATASET.NAME, "a photo of a {}.")
                txt = encode_prompts(clip_model, [temp.format(c.replace("_", " ")) for c in classnames], dev)
                self.classifier.weight.copy_(F.normalize(txt.float(), dim=-1))
            elif sec.INIT == "zeros":
                self.classifier.weight.zero_()
            else:
                raise ValueError(f"Unknown TRAINER.LINEAR_PROBE.INIT = {sec.INIT}")
            if self.classifier.bias is not None:
                self.classifier.bias.zero_()
        self.alpha, self.gamma, self.focal = None, 0.0, False
        if sec.LOSS_TYPE == "focal":
            print(">> Use Focal Loss!")
            alpha = focal_alpha(cfg.DATASET.get("PER_CLASS_SHOTS", None), n_cls, zero_guard=True)
            if alpha is not None:
                self.alpha = torch.tensor(alpha, dtype=torch.float32, device=dev)
            self.gamma, self.focal = 2.0, True
        elif sec.LOSS_TYPE != "ce":
            raise ValueError(f"Unknown loss_type = {sec.LOSS_TYPE}")
        self.fused_probe = bool(cfg.get("NATIVE", {}).get("FUSED_PROBE", False))

    def image_features(self, image):
        """The frozen encoder's raw features in fp32 (no gradient)."""
        with torch.no_grad():
            return self.clip_model.visual(image).float().contiguous()

    def _fused(self, feat):
        return self.fused_probe and probe_head_fused_ok(feat, self.classifier.weight, self.classifier.bias)

    def logits(self, feat):
        w, b = self.classifier.weight, self.classifier.bias
        if not torch.is_grad_enabled() and self._fused(feat):  # scoring only: one launch
            return ops.probe_head(feat, w.detach(), None if b is None else b.detach(), None, None, 0.0, False,
                                  self.normalize, self.scale)[1]
        u = F.normalize(feat, dim=-1) if self.normalize else feat
        s = self.scale * F.linear(u, w)
        return s if b is None else s + b

    def loss(self, feat, label):
        if self._fused(feat):
            return ProbeHeadFn.apply(feat, self.classifier.weight, self.classifier.bias, label, self.alpha,
                                     self.gamma, self.focal, self.normalize, self.scale)
        return CrossEntropyFn.apply(self.logits(feat), label, self.alpha, self.gamma, self.focal)

    def forward(self, image):
        return self.logits(self.image_features(image))


@TRAINER_REGISTRY.register()
class LinearProbeCLIP(TrainerX):
    @property
    def sec(self):
        return self.cfg.TRAINER.LINEAR_PROBE

    def check_cfg(self, cfg):
        assert cfg.TRAINER.LINEAR_PROBE.PREC in ["fp16", "fp32", "bf16", "fp32s"]

    def build_model(self):
        cfg = self.cfg
        self.cache = bool(self.sec.CACHE_FEATURES)
        if self.cache and dist.world_size() > 1:
            raise ValueError("TRAINER.LINEAR_PROBE.CACHE_FEATURES: single process only")
        classnames = self.dm.dataset.classnames
        print(f"Loading CLIP (backbone: {cfg.MODEL.BACKBONE.NAME})")
        clip_model = load_clip(cfg, self.sec.PREC, self.device, text_grad=False, vision_grad=False)
        print("Building the linear probe")
        self.model = LinearProbeModel(cfg, classnames, clip_model)
        enabled = sorted(n for n, p in self.model.named_parameters() if p.requires_grad)
        print(f"Parameters to be updated: {set(enabled)}")
        if cfg.MODEL.INIT_WEIGHTS:
            self.load_pretrained_weights(self.model.classifier, cfg.MODEL.INIT_WEIGHTS)
        self.optim = build_optimizer(self.model.classifier, cfg.OPTIM)
        self.sched = build_lr_scheduler(self.optim, cfg.OPTIM)
        self.register_model("classifier", self.model.classifier, self.optim, self.sched)
        self.bank = FeatureBank() if self.cache else None
        self._bank_ready = False

    def parse_batch_train(self, batch):
        return batch["img"].to(self.device), batch["label"].to(self.device)

    def forward_backward(self, batch):
        if "feat" in batch:  # from the bank
            feat, label = batch["feat"], batch["label"]
        else:
            image, label = self.parse_batch_train(batch)
            feat = self.model.image_features(image)
            if self.cache and not self._bank_ready:
                self.bank.add(feat, label)
        loss = self.model.loss(feat, label)
        self.optim.zero_grad()
        w = self.batch_weight(batch, feat.shape[0])
        if w != 1.0:
            (loss * w).backward()
        else:
            backward_unit(loss)
        self.allreduce_grads(self.model.classifier)
        self.optim.step()
        out = LossSummary()
        out["loss"] = loss
        if (self.batch_idx + 1) == self.num_batches:
            self.update_lr()
        return out

    def run_epoch(self):
        if not (self.cache and self._bank_ready):
            super().run_epoch()
            self._bank_ready = self.cache
            return
        self.set_model_mode("train")
        bs = int(self.cfg.DATALOADER.TRAIN_X.BATCH_SIZE)
        shuffle = bool(self.sec.CACHE_SHUFFLE)
        drop_last = len(self.bank) >= bs  # the loader's rule (data/manager.py)
        self.num_batches = self.bank.num_batches(bs, shuffle, drop_last)
        self.batch_idx = -1
        self.next_batch = None
        for feat, label in self.bank.batches(bs, shuffle, drop_last):
            self.batch_idx += 1
            summary = self.forward_backward({"feat": feat, "label": label})
            if (self.batch_idx + 1) % self.cfg.TRAIN.PRINT_FREQ == 0 and dist.rank() == 0:
                print(f"epoch [{self.epoch + 1}/{self.max_epoch}] batch [{self.batch_idx + 1}/"
                      f"{self.num_batches}] {summary} lr {self.get_current_lr():.4e}")

    def model_inference(self, image):
        return self.model(image)
