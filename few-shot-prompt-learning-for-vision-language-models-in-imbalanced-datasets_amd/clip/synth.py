"""Seeded synthetic CLIP state dicts and inputs (no network, no checkpoints).

The reference loads OpenAI CLIP checkpoints by URL (``PromptSRC/clip/clip.py:39-68``),
which is impossible offline, so parity and benchmarks run on random weights that
follow the reference's own init stds (``PromptSRC/clip/model.py:563-590``) drawn from
``numpy.random.RandomState`` (legacy stream: version-stable, so the fixtures made in
the survey container regenerate bit-identically on the GPU box).

Key layout follows the CLIP state dict that ``build_model`` consumes
(``PromptSRC/clip/model.py:662-705``): ``visual.*``, ``transformer.resblocks.i.*``,
``token_embedding.weight``, ``positional_embedding``, ``ln_final.*``,
``text_projection``, ``logit_scale``.

Deviation from a pure reference init (documented in DESIGN.md): biases and LayerNorm
affine parameters are drawn non-trivially (bias ~ N(0, 0.02), LN gamma ~ 1 + N(0, 0.05),
LN beta ~ N(0, 0.02)) so that parity tests exercise every parameter; the reference
would leave MHA biases at 0 and LN at (1, 0).
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, asdict

import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


@dataclass(frozen=True)
class ClipArch:
    embed_dim: int
    image_resolution: int
    vision_layers: int | tuple  # ViT: layers; ModifiedResNet: the four block counts
    vision_width: int
    vision_patch_size: int | None  # None: ModifiedResNet
    context_length: int
    vocab_size: int
    transformer_width: int
    transformer_heads: int
    transformer_layers: int

    @property
    def is_resnet(self) -> bool:  # model.py:503 (vision_layers a tuple: ModifiedResNet)
        return isinstance(self.vision_layers, (tuple, list))

    @property
    def vision_heads(self) -> int:  # model.py:504 / 506
        return self.vision_width * 32 // 64 if self.is_resnet else self.vision_width // 64

    @property
    def grid(self) -> int:
        return self.image_resolution // self.vision_patch_size

    @property
    def image_tokens(self) -> int:
        return self.grid * self.grid + 1

    def as_dict(self):
        return asdict(self)


ARCHS = {
    "ViT-B/32": ClipArch(512, 224, 12, 768, 32, 77, 49408, 512, 8, 12),
    "ViT-B/16": ClipArch(512, 224, 12, 768, 16, 77, 49408, 512, 8, 12),
    "ViT-L/14": ClipArch(768, 224, 24, 1024, 14, 77, 49408, 768, 12, 12),
    "ViT-L/14@336px": ClipArch(768, 336, 24, 1024, 14, 77, 49408, 768, 12, 12),
    # Small shapes for exhaustive parity (every width a multiple of 128, head dim 64).
    "tiny": ClipArch(128, 32, 2, 128, 16, 77, 49408, 128, 2, 2),
    "tiny-p8": ClipArch(128, 32, 2, 128, 8, 77, 49408, 128, 2, 2),
    "tiny4": ClipArch(128, 32, 4, 128, 16, 77, 49408, 128, 2, 4),  # deep-prompt depth coverage
    # ModifiedResNet backbones (clip.py model table; model.py:94-150): vision_layers = block counts
    "RN50": ClipArch(1024, 224, (3, 4, 6, 3), 64, None, 77, 49408, 512, 8, 12),
    "RN101": ClipArch(512, 224, (3, 4, 23, 3), 64, None, 77, 49408, 512, 8, 12),
    # Small ResNets for parity: full channel widths (64 .. 2048), one block per layer, small maps
    # (resolution 96: 24 / 12 / 6 / 3) and the tiny text tower.
    "RN-tiny": ClipArch(128, 64, (1, 1, 1, 1), 64, None, 77, 49408, 128, 2, 2),
    "RN-tiny-96": ClipArch(128, 96, (2, 1, 1, 1), 64, None, 77, 49408, 128, 2, 2),
}


def _blocks(prefix, width, layers):
    out = []
    proj_std = (width ** -0.5) * ((2 * layers) ** -0.5)  # model.py:579-581
    attn_std = width ** -0.5
    fc_std = (2 * width) ** -0.5
    for i in range(layers):
        p = f"{prefix}.resblocks.{i}."
        out += [
            (p + "attn.in_proj_weight", (3 * width, width), "w", attn_std),
            (p + "attn.in_proj_bias", (3 * width,), "b", 0.0),
            (p + "attn.out_proj.weight", (width, width), "w", proj_std),
            (p + "attn.out_proj.bias", (width,), "b", 0.0),
            (p + "ln_1.weight", (width,), "lnw", 0.0),
            (p + "ln_1.bias", (width,), "lnb", 0.0),
            (p + "mlp.c_fc.weight", (4 * width, width), "w", fc_std),
            (p + "mlp.c_fc.bias", (4 * width,), "b", 0.0),
            (p + "mlp.c_proj.weight", (width, 4 * width), "w", proj_std),
            (p + "mlp.c_proj.bias", (width,), "b", 0.0),
            (p + "ln_2.weight", (width,), "lnw", 0.0),
            (p + "ln_2.bias", (width,), "lnb", 0.0),
        ]
    return out


def _text_specs(a: ClipArch):
    W, E = a.transformer_width, a.embed_dim
    specs = [
        ("token_embedding.weight", (a.vocab_size, W), "w", 0.02),   # model.py:564
        ("positional_embedding", (a.context_length, W), "w", 0.01),  # model.py:565
    ]
    specs += _blocks("transformer", W, a.transformer_layers)
    specs += [
        ("ln_final.weight", (W,), "lnw", 0.0),
        ("ln_final.bias", (W,), "lnb", 0.0),
        ("text_projection", (W, E), "w", W ** -0.5),  # model.py:589-590
    ]
    return specs


def _resnet_specs(a: ClipArch):
    """ModifiedResNet keys (model.py:94-150) in a FIXED order. Convolutions feeding a ReLU draw
    std sqrt(2 / fan_in); a block's conv3 and downsample draw fan_in^-0.5 / 2 and fan_in^-0.5, and
    BatchNorm is near the identity (weight 1 + N(0, 0.05), bias N(0, 0.02), running_mean N(0, 0.1),
    running_var U[0.5, 1.5)), so activations stay O(1) through all 16 or 33 blocks."""
    w = a.vision_width
    specs = []

    def conv(key, cout, cin, k, std):
        specs.append((key + ".weight", (cout, cin, k, k), "w", std))

    def bn(key, c):
        specs.extend([(key + ".weight", (c,), "lnw", 0.0), (key + ".bias", (c,), "lnb", 0.0),
                      (key + ".running_mean", (c,), "w", 0.1), (key + ".running_var", (c,), "var", 0.0),
                      (key + ".num_batches_tracked", (), "count", 0.0)])

    for i, (cout, cin) in enumerate(((w // 2, 3), (w // 2, w // 2), (w, w // 2)), 1):
        conv(f"visual.conv{i}", cout, cin, 3, (2.0 / (9 * cin)) ** 0.5)
        bn(f"visual.bn{i}", cout)
    inpl = w
    for l, n in enumerate(a.vision_layers):
        planes = w << l
        for i in range(n):
            p = f"visual.layer{l + 1}.{i}."
            conv(p + "conv1", planes, inpl, 1, (2.0 / inpl) ** 0.5)
            bn(p + "bn1", planes)
            conv(p + "conv2", planes, planes, 3, (2.0 / (9 * planes)) ** 0.5)
            bn(p + "bn2", planes)
            conv(p + "conv3", planes * 4, planes, 1, 0.5 * planes ** -0.5)
            bn(p + "bn3", planes * 4)
            if i == 0:  # stride > 1 or inplanes != 4 * planes: every layer's first block
                conv(p + "downsample.0", planes * 4, inpl, 1, inpl ** -0.5)
                bn(p + "downsample.1", planes * 4)
            inpl = planes * 4
    C, S = inpl, a.image_resolution // 32
    std = C ** -0.5  # model.py:567-572
    specs.append(("visual.attnpool.positional_embedding", (S * S + 1, C), "w", std))
    for name, out in (("q_proj", C), ("k_proj", C), ("v_proj", C), ("c_proj", a.embed_dim)):
        specs += [(f"visual.attnpool.{name}.weight", (out, C), "w", std), (f"visual.attnpool.{name}.bias", (out,), "b", 0.0)]
    return specs


def _param_specs(a: ClipArch):
    """(key, shape, kind, std) in a FIXED order; kind in {w, b, lnw, lnb, var, count}."""
    if a.is_resnet:
        return _resnet_specs(a) + _text_specs(a)
    specs = []
    D, E = a.vision_width, a.embed_dim
    vscale = D ** -0.5  # model.py:386-391
    specs += [
        ("visual.class_embedding", (D,), "w", vscale),
        ("visual.positional_embedding", (a.image_tokens, D), "w", vscale),
        ("visual.proj", (D, E), "w", vscale),
        ("visual.conv1.weight", (D, 3, a.vision_patch_size, a.vision_patch_size), "w",
         (3 * a.vision_patch_size ** 2) ** -0.5),
        ("visual.ln_pre.weight", (D,), "lnw", 0.0),
        ("visual.ln_pre.bias", (D,), "lnb", 0.0),
    ]
    specs += _blocks("visual.transformer", D, a.vision_layers)
    specs += [
        ("visual.ln_post.weight", (D,), "lnw", 0.0),
        ("visual.ln_post.bias", (D,), "lnb", 0.0),
    ]
    return specs + _text_specs(a)


def make_state_dict(arch: str | ClipArch, seed: int = 0, logit_scale: float = float(np.log(100.0)),
                    fp16_values: bool = False):
    """Return {key: float32 ndarray} for a CLIP model of the given architecture. fp16_values:
    every parameter rounded to fp16 (then stored as float32), as the released CLIP checkpoints
    hold them (fp16 archives, PromptSRC/clip/clip.py:154-180; build_model copies them into the
    fp32 model, model.py:699-701): the weights a real fp32 run multiplies."""
    a = ARCHS[arch] if isinstance(arch, str) else arch
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape, kind, std in _param_specs(a):
        if kind == "count":  # BatchNorm's num_batches_tracked
            sd[key] = np.asarray(0, dtype=np.int64)
            continue
        if kind == "var":  # BatchNorm's running_var in [0.5, 1.5)
            v = 0.5 + rs.random_sample(size=shape)
            sd[key] = np.ascontiguousarray(v.astype(np.float16) if fp16_values else v, dtype=np.float32)
            continue
        z = rs.standard_normal(size=shape)
        if kind == "w":
            v = z * std
        elif kind == "b":
            v = z * 0.02
        elif kind == "lnw":
            v = 1.0 + 0.05 * z
        elif kind == "lnb":
            v = 0.02 * z
        else:
            raise AssertionError(kind)
        if fp16_values:
            v = v.astype(np.float16)
        sd[key] = np.ascontiguousarray(v, dtype=np.float32)
    sd["logit_scale"] = np.asarray(logit_scale, dtype=np.float32)
    return sd


def state_dict_digest(sd) -> str:
    """Stable short digest of a state dict (detects generator drift vs fixtures)."""
    h = hashlib.sha256()
    for k in sorted(sd):
        v = np.asarray(sd[k], dtype=np.float32)
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()[:16]


def make_images(batch: int, resolution: int, seed: int = 1) -> np.ndarray:
    """U[0,1) images, CLIP-normalised, NCHW float32."""
    rs = np.random.RandomState(seed)
    u = rs.random_sample(size=(batch, 3, resolution, resolution)).astype(np.float32)
    mean = np.asarray(CLIP_MEAN, dtype=np.float32)[None, :, None, None]
    std = np.asarray(CLIP_STD, dtype=np.float32)[None, :, None, None]
    return ((u - mean) / std).astype(np.float32)


def make_labels(batch: int, n_cls: int, seed: int = 2) -> np.ndarray:
    rs = np.random.RandomState(seed)
    return rs.randint(0, n_cls, size=(batch,)).astype(np.int64)


def synthetic_classnames(n_cls: int):
    return [f"class{i}" for i in range(n_cls)]


def make_ctx(n_ctx: int, width: int, n_cls: int | None = None, seed: int = 3) -> np.ndarray:
    """Context vectors ~ N(0, 0.02) (coop.py:228-234), [n_ctx,W] or [C,n_ctx,W] (CSC)."""
    rs = np.random.RandomState(seed)
    shape = (n_ctx, width) if n_cls is None else (n_cls, n_ctx, width)
    return (rs.standard_normal(size=shape) * 0.02).astype(np.float32)


def make_meta_net(vis_dim: int, ctx_dim: int, seed: int = 4) -> dict:
    """Meta-Net params (cocoop.py:139-143) ~ U(-1/sqrt(fan_in), 1/sqrt(fan_in))."""
    rs = np.random.RandomState(seed)
    hid = vis_dim // 16

    def u(shape, fan_in):
        b = 1.0 / np.sqrt(fan_in)
        return rs.uniform(-b, b, size=shape).astype(np.float32)

    return {
        "meta_net.linear1.weight": u((hid, vis_dim), vis_dim),
        "meta_net.linear1.bias": u((hid,), vis_dim),
        "meta_net.linear2.weight": u((ctx_dim, hid), hid),
        "meta_net.linear2.bias": u((ctx_dim,), hid),
    }
