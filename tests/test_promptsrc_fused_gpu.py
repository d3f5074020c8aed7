"""GPU: PromptSRC with NATIVE.FUSED_SRC (the head as one clipk_src_head call) and
TRAINER.PROMPTSRC.LOSS_TYPE.

Fixture parity: the fused step against the REFERENCE's own loss and gradients (promptsrc_tiny4), at
the gates tests/test_deep_gpu.py holds the unfused path to. On against off: the registry-built
trainer, as test_deep_gpu._trainer builds it, trains with both settings from the same seed.
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import test_deep_gpu as TD
from parity_util import GOLDEN, rel_err
from deep_util import grad_of
from oracle import clip_oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_fused_step_matches_reference(dev, prec):
    name = "promptsrc_tiny4"
    assert os.path.exists(os.path.join(GOLDEN, name + ".npz"))
    meta, ref, model, params, img, lbl = TD.build(name, prec, dev)
    model.train()
    out = {"want_logits": True}
    loss = model.fused_loss(img, lbl, 25, 10, 1.0, out)
    assert loss is not None, "the fused path must take the fixture's inputs"  # (fp16: features arrive as fp32)
    loss.backward()
    logits = out["logits"].cpu().numpy()
    report = {"logit_abs": float(np.abs(logits - ref["logits"]).max()),
              "loss_abs": abs(float(loss.detach()) - float(ref["loss"]))}
    grads = {k: params[k].grad.float().cpu().numpy() for k in meta["trainable"]}
    for k, g in grads.items():
        r, rows = grad_of(ref, k)
        report[k] = rel_err(g[rows], r) if prec == "fp32" else TD.cos_err(g[rows], r)
    print("fused promptsrc", prec, report)
    if prec == "fp32":
        assert report["logit_abs"] <= 1e-3
        assert rel_err(float(loss.detach()), ref["loss"]) <= 1e-4
        for k in grads:
            assert report[k] <= TD.grad_tol(k), (k, report[k])
    else:
        assert report["logit_abs"] <= 0.05
        assert report["loss_abs"] <= 0.05
        for k in grads:
            assert report[k] <= 5e-3, (k, report[k])


def _trainer(outdir, dev, fused, loss_type="ce", shots=None):
    """test_deep_gpu._trainer("PromptSRC", ...) with the keys under test set, from a fixed seed."""
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.clip import synth
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    cfg.MODEL.BACKBONE.NAME = "tiny4"
    cfg.OUTPUT_DIR = str(outdir)
    cfg.OPTIM.MAX_EPOCH = 2
    cfg.OPTIM.WARMUP_EPOCH = 1
    cfg.OPTIM.WARMUP_TYPE = "constant"
    cfg.TEST.NO_TEST = True
    cfg.TRAINER.NAME = "PromptSRC"
    s = cfg.TRAINER.PROMPTSRC
    s.PREC = "fp32"
    s.PROMPT_DEPTH_TEXT = s.PROMPT_DEPTH_VISION = 3
    s.LOSS_TYPE = loss_type
    cfg.NATIVE.FUSED_SRC = fused
    if shots is not None:
        cfg.DATASET.PER_CLASS_SHOTS = shots
    names = synth.synthetic_classnames(6)
    imgs = torch.from_numpy(synth.make_images(8, 32, seed=3)).to(dev)
    lbls = torch.from_numpy(synth.make_labels(8, 6, seed=4)).to(dev)

    class DM:
        class dataset:
            classnames = names
            lab2cname = {i: n for i, n in enumerate(names)}
        train_loader_x = [{"img": imgs[:4], "label": lbls[:4]}, {"img": imgs[4:], "label": lbls[4:]}]
        test_loader = [{"img": imgs, "label": lbls}]
        val_loader = None
        num_classes = 6

    torch.manual_seed(11)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tr = TRAINER_REGISTRY.get("PromptSRC")(cfg, dm=DM())
    tr.build_log = buf.getvalue()
    return tr


def _train(tr, monkeypatch, expect_calls):
    """Two epochs of two batches; returns the step losses. Counts ops.src_head calls."""
    from fsp_amd import ops
    calls = []
    real = ops.src_head

    def counted(*a, **k):
        calls.append(1)
        if expect_calls == 0:
            raise AssertionError("ops.src_head called with NATIVE.FUSED_SRC off")
        return real(*a, **k)

    monkeypatch.setattr(ops, "src_head", counted)
    before = {k: p.detach().clone() for k, p in tr.model.named_parameters() if p.requires_grad}
    assert before
    losses = []
    fb = tr.forward_backward
    tr.forward_backward = lambda b: losses.append(float(fb(b)["loss"])) or {"loss": losses[-1]}
    for tr.epoch in range(tr.max_epoch):
        tr.run_epoch()
        tr.after_epoch()
    monkeypatch.setattr(ops, "src_head", real)
    assert len(losses) == 4 and all(np.isfinite(losses))
    assert len(calls) == expect_calls
    moved = [k for k, p in tr.model.named_parameters() if k in before and not torch.equal(p.detach(), before[k])]
    assert moved, "no prompt parameter changed"
    # the GPA average was loaded after the last epoch
    assert tr.step_counter == tr.model.total_epochs + 1
    sd = tr.model.state_dict()
    for k, v in tr.previous_model_gpa.items():
        assert torch.equal(sd[k], v), k
    return losses, before


def _on_against_off(dev, tmp_path, monkeypatch, **kw):
    off = _trainer(tmp_path / "off", dev, False, **kw)
    on = _trainer(tmp_path / "on", dev, True, **kw)
    for (k, p), (k2, p2) in zip(off.model.named_parameters(), on.model.named_parameters()):
        assert k == k2 and torch.equal(p, p2)  # the same start
    l_off, _ = _train(off, monkeypatch, 0)
    l_on, before = _train(on, monkeypatch, 4)
    print("promptsrc step losses off", l_off, "on", l_on, kw)
    assert rel_err(l_on[0], l_off[0]) <= 1e-4
    return on, before


def test_fused_trainer_against_unfused(dev, tmp_path, monkeypatch):
    on, before = _on_against_off(dev, tmp_path, monkeypatch)
    saved = {k: p.detach().clone() for k, p in on.model.named_parameters()}
    tr2 = _trainer(tmp_path / "on2", dev, True)
    tr2.load_model(str(tmp_path / "on"), epoch=on.max_epoch)
    for k, p in tr2.model.named_parameters():
        if k in before:
            assert torch.equal(p.detach(), saved[k]), k
    assert "fixed_n" not in " ".join(on.model.state_dict()) and "_fixed_nq" not in " ".join(on.model.state_dict())


SHOTS = [16, 16, 16, 1, 1, 1]


def test_loss_type_focal(dev, tmp_path, monkeypatch):
    from fsp_amd.trainers.losses import focal_alpha
    alpha = focal_alpha(SHOTS, 6, zero_guard=True)
    for fused in (False, True):
        tr = _trainer(tmp_path / f"m{int(fused)}", dev, fused, "focal", SHOTS)
        assert ">> Use Focal Loss!" in tr.build_log
        batch = tr.dm.train_loader_x[0]
        img, lbl = batch["img"], batch["label"]
        tr.model.train()
        if fused:
            out = {"want_logits": True}
            s = tr.sec
            tr.model.fused_loss(img, lbl, s.TEXT_LOSS_WEIGHT, s.IMAGE_LOSS_WEIGHT, s.LOGITS_LOSS_WEIGHT, out)
            ce, logits = out["parts"][1], out["logits"]
        else:
            ce, _, _, _, _, _, logits = tr.model(img, lbl)
        ce, lg64, y = ce.detach(), logits.detach().double().cpu(), lbl.cpu()
        want = float(O.focal_loss(lg64, y, alpha, 2.0))
        plain = float(torch.nn.functional.cross_entropy(lg64, y))
        print(f"promptsrc focal (fused {fused}): ce term {float(ce):.6f} focal64 {want:.6f} plain CE {plain:.6f}")
        assert rel_err(float(ce), want) <= 1e-5
        assert abs(float(ce) - plain) > 1e-3 * abs(plain)
    _on_against_off(dev, tmp_path, monkeypatch, loss_type="focal", shots=SHOTS)


def test_loss_type_unknown_raises(dev, tmp_path):
    with pytest.raises(ValueError):
        _trainer(tmp_path / "x", dev, False, "nope")
