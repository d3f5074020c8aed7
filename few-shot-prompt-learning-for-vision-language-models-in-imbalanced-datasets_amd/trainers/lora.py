"""LoRA: low-rank adapters on the attention projections of both CLIP encoders (CLIP-LoRA), the
strongest few-shot baseline next to the prompt learners.

The fork lists a trainer of this name, but its source is not at hand: the keys of TRAINER.LORA and
the arithmetic below are THIS PACKAGE'S definition (CLIP-LoRA's public one, restricted), not a port.

    W'_p = W0_p + (ALPHA / RANK) B_p A_p      p in PARAMS (q, k, v) of attn.in_proj_weight,
                                              in the layers POSITION names, of the encoders ENCODER
    A_p [RANK, W] ~ kaiming_uniform(a = sqrt 5), B_p [W, RANK] = 0; everything else frozen
    logits = logit_scale * cos(image feature, text feature of CUSTOM_TEMPLATES[dataset])
    loss = CE or focal (LOSS_TYPE, the meaning the key has in TRAINER.COOP)

LoRA is linear in the weight, so the encoders run on the MERGED weights W' (clipk_lora_merge, once per
optimizer step: the existing forward and input-gradient kernels on W' / W'^T are LoRA's forward and
its backward through the adapter) and the backward adds the adapters' own gradient
(clipk_lora_wgrad, hooked into the layer loop by clipk_encoder_set_lora). Not supported, and refused
with ValueError: DROPOUT_RATE > 0 (dropout on the adapter input cannot be expressed with merged
weights), adapters on the ``o`` projection or the MLP.

``adapters`` (text.lora_A, text.lora_B, visual.lora_A, visual.lora_B; fp32 [layers, 3, r, W] and
[layers, 3, W, r]) is the only registered model: a checkpoint holds these four tensors and nothing
else. With ENCODER text / vision the other encoder is the frozen one (its adapters stay at their
initial values, without gradient, and its features carry none; frozen text features are encoded
once). Eval merges once per parameter version and caches the text features.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..clip.model import LoraSpec, LoraTextEncodeFn, LoraVisionFn, lora_init
from ..clip.tokenizer import tokenize
from ..engine.registry import TRAINER_REGISTRY
from ..engine.trainer import TrainerX
from ..engine.optim import build_optimizer, build_lr_scheduler
from ..engine.metrics import LossSummary
from ._fns import CrossEntropyFn, backward_unit
from .losses import focal_alpha
from .prompt_base import TextShape
from .zsclip import CUSTOM_TEMPLATES

POSITIONS = ("all", "bottom", "mid", "up", "half-bottom", "half-up", "top3")
ENCODERS = ("both", "text", "vision")


def proj_mask(params) -> int:
    """TRAINER.LORA.PARAMS -> clipk_lora_*'s proj_mask (bit 0 q, 1 k, 2 v)."""
    params = list(params)
    bad = [p for p in params if p not in ops.LORA_PROJ_BITS]
    if bad or not params:
        raise ValueError(f"TRAINER.LORA.PARAMS must be a non-empty subset of q, k, v (got {params}): adapters on "
                         f"the o projection and the MLP are not supported")
    m = 0
    for p in params:
        m |= ops.LORA_PROJ_BITS[p]
    return m


def layer_mask(position: str, layers: int) -> int:
    """TRAINER.LORA.POSITION -> layer_mask (bit l = layer l) for an encoder of ``layers`` blocks,
    CLIP-LoRA's layer sets: thirds (bottom / mid / up), halves, the last three, all."""
    n = int(layers)
    if position not in POSITIONS:
        raise ValueError(f"TRAINER.LORA.POSITION must be one of {POSITIONS}, got {position!r}")
    if not 1 <= n <= 32:
        raise ValueError(f"LoRA supports encoders of 1..32 layers, got {n}")
    t1, t2, h = -(-n // 3), -(-2 * n // 3), n // 2
    lo, hi = {"all": (0, n), "bottom": (0, t1), "mid": (t1, t2), "up": (t2, n), "half-bottom": (0, h),
              "half-up": (h, n), "top3": (max(n - 3, 0), n)}[position]
    if hi <= lo:
        raise ValueError(f"TRAINER.LORA.POSITION {position!r} names no layer of a {n}-layer encoder")
    return sum(1 << l for l in range(lo, hi))


def lora_spec(sec, layers: int) -> LoraSpec:
    """The LoraSpec of TRAINER.LORA for an encoder of ``layers`` blocks (raises ValueError for what
    is not supported)."""
    if float(sec.DROPOUT_RATE) > 0.0:
        raise ValueError("TRAINER.LORA.DROPOUT_RATE > 0 is not supported: dropout on the adapter input cannot be "
                         "expressed with merged weights")
    if sec.ENCODER not in ENCODERS:
        raise ValueError(f"TRAINER.LORA.ENCODER must be one of {ENCODERS}, got {sec.ENCODER!r}")
    return LoraSpec(int(sec.RANK), float(sec.ALPHA) / float(sec.RANK), proj_mask(sec.PARAMS),
                    layer_mask(sec.POSITION, layers))


class _Adapter(nn.Module):
    def __init__(self, layers, rank, width, generator):
        super().__init__()
        A, B = lora_init(layers, rank, width, generator)
        self.lora_A = nn.Parameter(A)
        self.lora_B = nn.Parameter(B)


class LoraAdapters(nn.Module):
    """The trainable tensors: text.lora_A / lora_B and visual.lora_A / lora_B."""

    def __init__(self, arch, rank, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.text = _Adapter(arch.transformer_layers, rank, arch.transformer_width, g)
        self.visual = _Adapter(arch.vision_layers, rank, arch.vision_width, g)


def _version(params):
    return tuple((p.data_ptr(), p._version, getattr(p, "_clipk_gen", 0)) for p in params)


class LoraCLIP(nn.Module):
    """CLIP with LoRA encoders: image -> logits (eval) or the loss (training)."""

    def __init__(self, cfg, classnames, clip_model, adapters):
        super().__init__()
        sec = cfg.TRAINER.LORA
        object.__setattr__(self, "clip", clip_model)  # frozen native encoders: not submodules
        self.adapters = adapters
        self.text_on, self.vision_on = clip_model.text.lora is not None, clip_model.visual.lora is not None
        self.logit_scale_value = clip_model.logit_scale_value
        dev = clip_model.logit_scale.device
        temp = CUSTOM_TEMPLATES.get(cfg.DATASET.NAME, "a photo of a {}.")
        tok = torch.from_numpy(tokenize([temp.format(c.replace("_", " ")) for c in classnames]).astype(np.int64))
        eot = tok.argmax(dim=-1)
        L = int(eot.max()) + 1  # truncated to max EOT + 1: exact under the causal mask
        with torch.no_grad():
            emb = clip_model.token_embedding(tok)[:, :L].to(dev)
            self.x0 = (emb + clip_model.positional_embedding[:L]).contiguous()  # [C, L, W], frozen
        self.eot, self.L, self.n_cls = eot.to(dev), L, len(classnames)
        # NATIVE.MAX_TEXT_ROWS: classes per text-encoder call
        max_rows = int(cfg.get("NATIVE", {}).get("MAX_TEXT_ROWS", 2_000_000))
        self.chunk = max(1, max_rows // L)
        self.alpha, self.gamma, self.focal = None, 0.0, False
        if sec.LOSS_TYPE == "focal":
            print(">> Use Focal Loss!")
            alpha = focal_alpha(cfg.DATASET.get("PER_CLASS_SHOTS", None), self.n_cls, zero_guard=True)
            if alpha is not None:
                self.alpha = torch.tensor(alpha, dtype=torch.float32, device=dev)
            self.gamma, self.focal = 2.0, True
        elif sec.LOSS_TYPE != "ce":
            raise ValueError(f"Unknown loss_type = {sec.LOSS_TYPE}")
        self._merged = {}
        self._txt_cache = None

    def _shape(self, c0, c1):
        n = c1 - c0
        rows = (torch.arange(n, device=self.eot.device) * self.L + self.eot[c0:c1]).to(torch.int32)
        return TextShape(rows, nseq=n, L=self.L)

    def merge(self):
        """The encoders' tables <- the adapters' current values: once per parameter version."""
        for name, enc, on in (("text", self.clip.text, self.text_on), ("visual", self.clip.visual, self.vision_on)):
            ad = getattr(self.adapters, name)
            key = _version((ad.lora_A, ad.lora_B))
            if on and self._merged.get(name) != key:
                enc.lora.merge(ad.lora_A.detach(), ad.lora_B.detach())
                self._merged[name] = key

    def text_features(self):
        core, ad = self.clip.text, self.adapters.text
        W = self.x0.shape[-1]
        out = []
        for c0 in range(0, self.n_cls, self.chunk):
            c1 = min(c0 + self.chunk, self.n_cls)
            x0 = self.x0[c0:c1].reshape(-1, W)
            if self.text_on:  # (chunks: autograd sums their dA / dB)
                out.append(LoraTextEncodeFn.apply(ad.lora_A, ad.lora_B, x0, core, self._shape(c0, c1)))
            else:
                with torch.no_grad():
                    out.append(core.forward(x0, self._shape(c0, c1), save=False)[0])
        return out[0] if len(out) == 1 else torch.cat(out, 0)

    def cached_text_features(self):
        """Without autograd: encode the class prompts once per parameter version (a frozen text
        encoder: once)."""
        key = _version(self.adapters.text.parameters()) if self.text_on else ()
        if self._txt_cache is None or self._txt_cache[0] != key:
            with torch.no_grad():
                self._txt_cache = (key, self.text_features())
        return self._txt_cache[1]

    def image_features(self, image):
        if self.vision_on:
            ad = self.adapters.visual
            return LoraVisionFn.apply(ad.lora_A, ad.lora_B, image, self.clip.visual)
        with torch.no_grad():
            return self.clip.visual(image)

    def logits(self, image):
        self.merge()
        if not self.text_on or not torch.is_grad_enabled():
            txt = self.cached_text_features()
        else:
            txt = self.text_features()
        img = F.normalize(self.image_features(image), dim=-1)
        txt = F.normalize(txt, dim=-1)
        return self.logit_scale_value * img @ txt.t()

    def forward(self, image, label=None):
        logits = self.logits(image)
        if label is None:
            return logits
        return CrossEntropyFn.apply(logits, label, self.alpha, self.gamma, self.focal)


@TRAINER_REGISTRY.register()
class LoRA(TrainerX):
    @property
    def sec(self):
        return self.cfg.TRAINER.LORA

    def check_cfg(self, cfg):
        assert cfg.TRAINER.LORA.PREC in ["fp16", "fp32", "amp", "bf16", "fp32s"]

    def build_model(self):
        cfg, sec = self.cfg, self.sec
        classnames = self.dm.dataset.classnames
        from ..clip import synth
        from ..clip.weights import load_state_dict
        from ..clip.model import arch_from_state_dict, build_model, require_vit
        path = cfg.MODEL.get("WEIGHTS_PATH", "")
        print(f"Loading CLIP (backbone: {cfg.MODEL.BACKBONE.NAME})")
        if not path and cfg.MODEL.BACKBONE.NAME in synth.ARCHS:
            require_vit("LoRA", cfg.MODEL.BACKBONE.NAME, synth.ARCHS[cfg.MODEL.BACKBONE.NAME])
        sd = load_state_dict(path) if path else synth.make_state_dict(
            cfg.MODEL.BACKBONE.NAME, seed=0, fp16_values=bool(cfg.MODEL.get("SYNTH_FP16", False)))
        arch = arch_from_state_dict(sd)
        require_vit("LoRA", cfg.MODEL.BACKBONE.NAME, arch)
        text_on, vision_on = sec.ENCODER in ("both", "text"), sec.ENCODER in ("both", "vision")
        tspec, vspec = lora_spec(sec, arch.transformer_layers), lora_spec(sec, arch.vision_layers)
        clip_model = build_model(sd, prec=sec.PREC, device=self.device, text_grad=text_on, vision_grad=vision_on,
                                 text_lora=tspec if text_on else None, vision_lora=vspec if vision_on else None)
        print("Building LoRA CLIP")
        self.adapters = LoraAdapters(arch, int(sec.RANK), seed=max(int(cfg.get("SEED", 0)), 0)).to(self.device)
        self.adapters.text.requires_grad_(text_on)
        self.adapters.visual.requires_grad_(vision_on)
        self.model = LoraCLIP(cfg, classnames, clip_model, self.adapters)
        enabled = sorted(n for n, p in self.adapters.named_parameters() if p.requires_grad)
        print(f"Parameters to be updated: {set(enabled)}")
        if cfg.MODEL.INIT_WEIGHTS:
            self.load_pretrained_weights(self.adapters, cfg.MODEL.INIT_WEIGHTS)
        self.optim = build_optimizer(self.adapters, cfg.OPTIM)
        self.sched = build_lr_scheduler(self.optim, cfg.OPTIM)
        self.register_model("adapters", self.adapters, self.optim, self.sched)

    def parse_batch_train(self, batch):
        return batch["img"].to(self.device), batch["label"].to(self.device)

    def forward_backward(self, batch):
        image, label = self.parse_batch_train(batch)
        loss = self.model(image, label)
        self.optim.zero_grad()
        w = self.batch_weight(batch, image.shape[0])
        if w != 1.0:
            (loss * w).backward()
        else:
            backward_unit(loss)
        self.allreduce_grads(self.adapters)
        self.optim.step()
        out = LossSummary()
        out["loss"] = loss
        if (self.batch_idx + 1) == self.num_batches:
            self.update_lr()
        return out

    def model_inference(self, image):
        return self.model(image)
