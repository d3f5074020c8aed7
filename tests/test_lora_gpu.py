"""GPU: the LoRA encoders and trainer end to end against torch on the CPU.

Reference: oracle/clip_oracle.py in fp64 on p' = lora_util.lora_params(p, adapters, ...) (in_proj
weights W0 + s B A from autograd leaves A, B), the trainer's head (cosine logits at CLIP's logit
scale, CE) on top. Cases: the tiny synthetic CLIP ("tiny4": 4 layers, width 128) and one
ViT-B/32-width model of 2 layers (vision width 768, text width 512), C = 5 classes, B = 3 images,
adapters with B != 0 so that dA and dB are both exercised.

Gates: those tests/test_deep_gpu.py applies to its prompt gradients. PREC fp32 and fp32s (the fp32
class, tests/test_parity_gpu.py): loss rel <= 1e-4, gradients rel <= 1e-3 (parity_util.rel_err: max
abs difference over max |ref|); PREC fp16: |d loss| <= 0.05, 1 - cos(grad) <= 5e-3.
"""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity_util import rel_err, state_dict
from lora_util import lora_params, tiny_adapters

pytestmark = pytest.mark.gpu

C, B = 5, 3
RANK, ALPHA = 2, 1
_SD = {}
_REF = {}


def cos_err(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(1 - a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def arch_sd(name):
    """(ClipArch, state dict) of a case: "tiny4" or "b32x2" (ViT-B/32 widths, 2 layers each)."""
    from fsp_amd.clip import synth
    if name == "tiny4":
        return synth.ARCHS["tiny4"], state_dict("tiny4")
    if name not in _SD:
        a = synth.ClipArch(512, 224, 2, 768, 32, 77, 49408, 512, 8, 2)
        _SD[name] = (a, synth.make_state_dict(a, seed=0))
    return _SD[name]


def make_cfg(arch, prec, **lora):
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (arch.image_resolution, arch.image_resolution)
    cfg.TRAINER.LORA.PREC = prec
    cfg.TRAINER.LORA.RANK, cfg.TRAINER.LORA.ALPHA = RANK, ALPHA
    for k, v in lora.items():
        cfg.TRAINER.LORA[k] = v
    return cfg


def build(name, prec, dev, adapters=None, encoder="both", position="all", params=("q", "k", "v")):
    """(LoraCLIP, adapters module, images, labels) with the adapters' values set."""
    from fsp_amd.clip import synth
    from fsp_amd.clip.model import build_model
    from fsp_amd.trainers import lora as L
    arch, sd = arch_sd(name)
    cfg = make_cfg(arch, prec, ENCODER=encoder, POSITION=position, PARAMS=list(params))
    sec = cfg.TRAINER.LORA
    t_on, v_on = encoder in ("both", "text"), encoder in ("both", "vision")
    clip = build_model(sd, prec=prec, device=dev, text_grad=t_on, vision_grad=v_on,
                       text_lora=L.lora_spec(sec, arch.transformer_layers) if t_on else None,
                       vision_lora=L.lora_spec(sec, arch.vision_layers) if v_on else None)
    ad = L.LoraAdapters(arch, RANK).to(dev)
    if adapters is not None:
        with torch.no_grad():
            for side in ("text", "visual"):
                getattr(ad, side).lora_A.copy_(adapters[side][0])
                getattr(ad, side).lora_B.copy_(adapters[side][1])
    ad.text.requires_grad_(t_on)
    ad.visual.requires_grad_(v_on)
    model = L.LoraCLIP(cfg, synth.synthetic_classnames(C), clip, ad)
    img = torch.from_numpy(synth.make_images(B, arch.image_resolution, seed=1)).to(dev)
    lbl = torch.from_numpy(synth.make_labels(B, C, seed=2)).to(dev)
    return model, ad, img, lbl


def reference(name):
    """fp64 oracle: loss and the gradients of the four adapter tensors (computed once per case)."""
    if name in _REF:
        return _REF[name]
    from oracle import clip_oracle as O
    from fsp_amd.clip import synth
    from fsp_amd.clip.tokenizer import tokenize
    from fsp_amd.trainers import lora as L
    arch, sd = arch_sd(name)
    p = {k: v.double() for k, v in O.as_torch_sd(sd).items()}
    ad = {s: tuple(t.double().requires_grad_(True) for t in ab) for s, ab in tiny_adapters(arch, RANK, seed=7).items()}
    masks = {"text": L.layer_mask("all", arch.transformer_layers), "visual": L.layer_mask("all", arch.vision_layers)}
    q = lora_params(p, ad, ALPHA / RANK, 7, masks)
    tok = torch.from_numpy(tokenize(["a photo of a {}.".format(c) for c in synth.synthetic_classnames(C)])
                           .astype(np.int64))
    Lr = int(tok.argmax(-1).max()) + 1
    txt = O.encode_text(q, O.token_embed(q, tok)[:, :Lr], tok)
    img = O.encode_image(q, torch.from_numpy(synth.make_images(B, arch.image_resolution, seed=1)).double())
    logits = torch.exp(p["logit_scale"]) * O.normalize(img) @ O.normalize(txt).t()
    loss = F.cross_entropy(logits, torch.from_numpy(synth.make_labels(B, C, seed=2)))
    loss.backward()
    grads = {f"{s}.lora_{n}": t.grad.numpy() for s, ab in ad.items() for n, t in zip("AB", ab)}
    _REF[name] = (float(loss.detach()), grads)
    return _REF[name]


@pytest.mark.parametrize("prec", ["fp32", "fp32s", "fp16"])
@pytest.mark.parametrize("name", ["tiny4", "b32x2"])
def test_loss_and_adapter_gradients_match_the_oracle(dev, name, prec):
    arch, _ = arch_sd(name)
    ref_loss, ref_g = reference(name)
    model, ad, img, lbl = build(name, prec, dev, tiny_adapters(arch, RANK, seed=7))
    model.train()
    loss = model(img, lbl)
    loss.backward()
    grads = {k: p.grad.float().cpu().numpy() for k, p in ad.named_parameters()}
    assert set(grads) == set(ref_g)
    loss = float(loss.detach())
    report = {"loss_abs": abs(loss - ref_loss)}
    for k, g in grads.items():
        assert np.abs(ref_g[k]).max() > 0
        report[k] = rel_err(g, ref_g[k]) if prec != "fp16" else cos_err(g, ref_g[k])
    print("lora", name, prec, report)
    if prec != "fp16":
        assert rel_err(loss, ref_loss) <= 1e-4
        for k in grads:
            assert report[k] <= 1e-3, (k, report[k])
    else:
        assert report["loss_abs"] <= 0.05
        for k in grads:
            assert report[k] <= 5e-3, (k, report[k])


@pytest.mark.parametrize("prec", ["fp32", "fp32s", "fp16"])
def test_zero_b_features_are_those_of_the_plain_encoders(dev, prec):
    """B = 0 (the initial adapters): W' = cast(W0), so the features are bitwise those of the same
    encoder classes built without LoRA on the same plain path (no LayerNorm fold, plain text rows,
    the prompted ViT's calls with no prompt rows)."""
    from fsp_amd.clip.model import build_model, TextEncodeFn
    model, ad, img, _ = build("tiny4", prec, dev)
    assert not ad.text.lora_B.any() and not ad.visual.lora_B.any() and ad.text.lora_A.any()
    base = build_model(state_dict("tiny4"), prec=prec, device=dev, text_grad=True, vision_grad=True, ln_fold=False)
    with torch.no_grad():
        model.merge()
        txt = model.text_features()
        imf = model.image_features(img)
        W = model.x0.shape[-1]
        txt0 = TextEncodeFn.apply(model.x0.reshape(-1, W), base.text, model._shape(0, C))
        imf0, _ = base.visual.forward_prompted(img, torch.zeros(0, base.visual.width, device=dev))
    assert torch.equal(txt, txt0)
    assert torch.equal(imf, imf0)
    assert torch.isfinite(txt).all() and float(txt.abs().max()) > 0


def test_error_paths(dev):
    from fsp_amd import _native as N, ops
    from fsp_amd.clip import synth
    from fsp_amd.clip.model import build_model
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.trainers.deep import VLPromptLearner
    lib = N.load()
    EINVAL = -1
    model, ad, img, _ = build("tiny4", "fp16", dev)
    text, vis = model.clip.text, model.clip.visual
    A, Bm = ad.text.lora_A.detach(), ad.text.lora_B.detach()
    # a LayerNorm fold and LoRA exclude each other, whichever comes first
    folded = build_model(state_dict("tiny4"), prec="fp16", device=dev)
    for h in (folded.text.handle, folded.visual.handle):
        assert lib.clipk_encoder_set_lora(h, RANK, 7, 0xf, 0.5, ops._p(A), ops._p(Bm), None, None) == EINVAL
    some = (ctypes.c_void_p * (6 * 4))(*([A.data_ptr()] * 24))
    assert lib.clipk_encoder_set_ln_fold(text.handle, some) == EINVAL
    assert lib.clipk_encoder_set_ln_fold(vis.handle, some) == EINVAL
    # deep prompts and LoRA exclude each other
    rows = torch.zeros(C, dtype=torch.int32, device=dev)
    deep = torch.zeros(1, 1, 128, device=dev)
    assert lib.clipk_encoder_set_deep_prompts(text.handle, 1, 1, C, ops._p(rows), ops._p(deep), None) == EINVAL
    plain = build_model(state_dict("tiny4"), prec="fp32", device=dev)  # (fp32: no fold)
    assert lib.clipk_encoder_set_deep_prompts(plain.text.handle, 1, 1, C, ops._p(rows), ops._p(deep), None) == 0
    assert lib.clipk_encoder_set_lora(plain.text.handle, RANK, 7, 0xf, 0.5, ops._p(A), ops._p(Bm), None, None) == EINVAL
    assert lib.clipk_encoder_set_deep_prompts(plain.text.handle, 0, 0, 0, None, None, None) == 0
    # bad arguments
    for rank, pm, lm in ((17, 7, 0xf), (2, 0, 0xf), (2, 8, 0xf), (2, 7, 0x10)):
        assert lib.clipk_encoder_set_lora(plain.text.handle, rank, pm, lm, 0.5, ops._p(A), ops._p(Bm), None, None) \
            == EINVAL, (rank, pm, lm)
    # the packed entry points while LoRA is set: a packed call that runs on the plain encoder
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    s = cfg.TRAINER.IVLP
    s.N_CTX_TEXT, s.CTX_INIT = 4, "a photo of a"
    pl = VLPromptLearner(s, synth.synthetic_classnames(6), plain, cfg)
    x0, shape = pl.assemble().detach(), pl.layout.shape(1)
    assert shape.packed
    assert torch.isfinite(plain.text.forward(x0, shape, save=False)[0]).all()
    lora32, _, _, _ = build("tiny4", "fp32", dev)
    with pytest.raises(N.ClipkError, match="clipk_text_forward_packed.*status -1"):
        lora32.clip.text.forward(x0, shape, save=False)
    # prompt rows on a LoRA ViT
    with pytest.raises(N.ClipkError, match="status -1"):
        lora32.clip.visual.forward_prompted(img, torch.zeros(2, 128, device=dev))
    # rank 0 clears: the fold setter is accepted again
    assert lib.clipk_encoder_set_lora(text.handle, 0, 0, 0, 0.0, None, None, None, None) == 0
    assert lib.clipk_encoder_set_deep_prompts(text.handle, 1, 1, C, ops._p(rows), ops._p(deep), None) == 0
    assert lib.clipk_encoder_set_deep_prompts(text.handle, 0, 0, 0, None, None, None) == 0


@pytest.mark.parametrize("encoder", ["text", "vision"])
def test_one_sided_adapters(dev, encoder):
    """ENCODER text / vision: the other encoder is the frozen one, its adapters get no gradient."""
    arch, _ = arch_sd("tiny4")
    model, ad, img, lbl = build("tiny4", "fp32", dev, tiny_adapters(arch, RANK, seed=7), encoder=encoder)
    model.train()
    model(img, lbl).backward()
    on, off = (ad.text, ad.visual) if encoder == "text" else (ad.visual, ad.text)
    assert off.lora_A.grad is None and off.lora_B.grad is None
    for p in (on.lora_A, on.lora_B):
        assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    assert (model.clip.text.lora is None) == (encoder == "vision")
    assert (model.clip.visual.lora is None) == (encoder == "text")


def test_position_top3_and_params(dev):
    """POSITION top3 on 4 layers: layer 0 has no adapters, its gradients are exactly zero; PARAMS
    q, v: the k slices are exactly zero."""
    arch, _ = arch_sd("tiny4")
    model, ad, img, lbl = build("tiny4", "fp32", dev, tiny_adapters(arch, RANK, seed=7), position="top3",
                                params=("q", "v"))
    model.train()
    model(img, lbl).backward()
    for side in (ad.text, ad.visual):
        for p in (side.lora_A, side.lora_B):
            g = p.grad
            assert not g[0].any(), "masked-off layer"
            assert not g[:, 1].any(), "disabled projection"
            for l in (1, 2, 3):
                for j in (0, 2):
                    assert float(g[l, j].abs().max()) > 0, (l, j)


def _trainer(outdir, dev, n_test_batches=3, **lora):
    """A registry-built LoRA trainer on tiny4 with an in-memory data manager: one training batch
    per epoch, six epochs."""
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.clip import synth
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    arch, _ = arch_sd("tiny4")
    cfg = make_cfg(arch, "fp32", **lora)
    cfg.MODEL.BACKBONE.NAME = "tiny4"
    cfg.OUTPUT_DIR = str(outdir)
    cfg.OPTIM.NAME = "adamw"
    cfg.OPTIM.LR = 5e-3
    cfg.OPTIM.MAX_EPOCH = 6
    cfg.TEST.NO_TEST = True
    cfg.TRAINER.NAME = "LoRA"
    names = synth.synthetic_classnames(C)
    imgs = torch.from_numpy(synth.make_images(9, 32, seed=3)).to(dev)
    lbls = torch.from_numpy(synth.make_labels(9, C, seed=4)).to(dev)

    class DM:
        class dataset:
            classnames = names
            lab2cname = {i: n for i, n in enumerate(names)}
        train_loader_x = [{"img": imgs[:8], "label": lbls[:8]}]
        test_loader = [{"img": imgs[3 * i:3 * i + 3], "label": lbls[3 * i:3 * i + 3]} for i in range(n_test_batches)]
        val_loader = None
        num_classes = C

    with contextlib.redirect_stdout(io.StringIO()):
        return TRAINER_REGISTRY.get("LoRA")(cfg, dm=DM()), imgs


def test_trainer_trains_saves_and_reloads(dev, tmp_path, monkeypatch):
    from fsp_amd import ops
    from fsp_amd.engine.optim import FusedAdam
    tr, imgs = _trainer(tmp_path / "out", dev)
    assert isinstance(tr.optim, FusedAdam)
    assert tr.get_model_names() == ["adapters"]
    before = {k: p.detach().clone() for k, p in tr.adapters.named_parameters()}
    losses = []
    fb = tr.forward_backward
    tr.forward_backward = lambda b: losses.append(float(fb(b)["loss"])) or {"loss": losses[-1]}
    merges = []
    real = ops.lora_merge
    monkeypatch.setattr(ops, "lora_merge", lambda *a, **k: merges.append(1) or real(*a, **k))
    for tr.epoch in range(tr.max_epoch):
        tr.run_epoch()
        tr.after_epoch()
    print("lora trainer losses", losses)
    assert len(losses) == 6 and all(np.isfinite(losses))
    assert losses[5] < losses[0]
    assert len(merges) == 2 * 6, "one merge per encoder and optimizer step"
    for k, p in tr.adapters.named_parameters():
        assert not torch.equal(p.detach(), before[k]), k
    # the checkpoint holds the adapters and nothing else
    ck = tr.load_checkpoint(os.path.join(str(tmp_path / "out"), "adapters", "model.pth.tar-6"))
    assert set(ck["state_dict"]) == {"text.lora_A", "text.lora_B", "visual.lora_A", "visual.lora_B"}
    # eval: one merge per encoder for the whole test set, not one per batch
    del merges[:]
    with contextlib.redirect_stdout(io.StringIO()):
        y_true, y_pred = tr.test(return_pred=True)
    assert len(y_true) == len(y_pred) == 9
    assert len(merges) == 2, merges
    with contextlib.redirect_stdout(io.StringIO()):
        tr.test()
    assert len(merges) == 2, "unchanged parameters: no further merge"
    tr.set_model_mode("eval")
    with torch.no_grad():
        logits = tr.model_inference(imgs)
    # a reloaded trainer scores bitwise the same
    tr2, _ = _trainer(tmp_path / "out2", dev)
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.load_model(str(tmp_path / "out"), epoch=6)
    for k, p in tr2.adapters.named_parameters():
        assert torch.equal(p.detach(), dict(tr.adapters.named_parameters())[k].detach()), k
    tr2.set_model_mode("eval")
    with torch.no_grad():
        logits2 = tr2.model_inference(imgs)
    assert torch.equal(logits, logits2)


def test_trainer_refuses_dropout_and_other_projections(dev, tmp_path):
    with pytest.raises(ValueError, match="DROPOUT_RATE"):
        _trainer(tmp_path / "a", dev, DROPOUT_RATE=0.1)
    with pytest.raises(ValueError, match="o projection"):
        _trainer(tmp_path / "b", dev, PARAMS=["q", "o"])
