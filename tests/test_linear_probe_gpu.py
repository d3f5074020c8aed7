"""GPU: the LinearProbeCLIP trainer (trainers/linear_probe.py) -- its zero-shot initialisation
against a ZeroshotCLIP-style score, NATIVE.FUSED_PROBE on against off from one seed, the frozen CLIP,
the checkpoint, LOSS_TYPE focal, and the feature cache (CACHE_FEATURES / CACHE_SHUFFLE).

The trainer is built as test_promptsrc_fused_gpu._trainer builds PromptSRC: backbone "tiny4" at
32 px, 6 synthetic classes, two batches of 4, PREC fp32, torch.manual_seed(11).
"""
import contextlib
import io
import math
import os

import numpy as np
import pytest
import torch

from parity_util import rel_err

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
SHOTS = [4, 1, 1, 1, 1, 1]


def _trainer(outdir, dev, fused, loss_type="ce", shots=None, init="zeroshot", cache=False, shuffle=True, epochs=2):
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.clip import synth
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    cfg.MODEL.BACKBONE.NAME = "tiny4"
    cfg.OUTPUT_DIR = str(outdir)
    cfg.OPTIM.MAX_EPOCH = epochs
    cfg.OPTIM.WARMUP_EPOCH = 1
    cfg.OPTIM.WARMUP_TYPE = "constant"
    cfg.OPTIM.LR = 0.01
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 4
    cfg.TEST.NO_TEST = True
    cfg.TRAINER.NAME = "LinearProbeCLIP"
    s = cfg.TRAINER.LINEAR_PROBE
    s.PREC = "fp32"
    s.LOSS_TYPE = loss_type
    s.INIT = init
    s.CACHE_FEATURES = cache
    s.CACHE_SHUFFLE = shuffle
    cfg.NATIVE.FUSED_PROBE = fused
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
        tr = TRAINER_REGISTRY.get("LinearProbeCLIP")(cfg, dm=DM())
    tr.build_log = buf.getvalue()
    return tr


def _train(tr, monkeypatch, expect_calls=None, seen=None):
    """All epochs of two batches; returns the step losses. Counts ops.probe_head calls (each must
    carry labels: the training form); seen (a list) receives every batch the steps were given."""
    from fsp_amd import ops
    calls = []
    real = ops.probe_head

    def counted(feat, w, bias, labels, *a, **k):
        calls.append(1)
        assert expect_calls != 0, "ops.probe_head called with NATIVE.FUSED_PROBE off"
        assert labels is not None
        return real(feat, w, bias, labels, *a, **k)

    monkeypatch.setattr(ops, "probe_head", counted)
    losses = []
    fb = tr.forward_backward

    def step(batch):
        if seen is not None:
            seen.append((tr.epoch, batch))
        losses.append(float(fb(batch)["loss"]))
        return {"loss": losses[-1]}

    tr.forward_backward = step
    for tr.epoch in range(tr.max_epoch):
        tr.run_epoch()
        tr.after_epoch()
    monkeypatch.setattr(ops, "probe_head", real)
    tr.forward_backward = fb
    assert len(losses) == 2 * tr.max_epoch and all(np.isfinite(losses))
    if expect_calls is not None:
        assert len(calls) == expect_calls
    return losses


@pytest.mark.parametrize("fused", [False, True])
def test_zeroshot_init_scores_as_zeroshot_clip(dev, tmp_path, fused):
    from fsp_amd.trainers._fns import CosineLogitsFn
    tr = _trainer(tmp_path / "z", dev, fused)
    m = tr.model
    assert m.classifier.weight.dtype == torch.float32 and not m.classifier.bias.any()
    img = tr.dm.test_loader[0]["img"]
    tr.set_model_mode("eval")
    with torch.no_grad():
        got = tr.model_inference(img)
        imf = m.clip_model.visual(img).float()
        imf = imf / imf.norm(dim=-1, keepdim=True)
        want = CosineLogitsFn.apply(imf, m.classifier.weight.detach().contiguous(), m.scale, 0, 6)
    err = float((got - want).abs().max())
    print(f"zeroshot init (fused {fused}): scale {m.scale:.4f} |logits - zero-shot| {err:.3e} "
          f"(bound {16 * ULP * m.scale:.3e})")
    assert got.shape == (8, 6) and m.scale == m.clip_model.logit_scale_value
    assert err <= 16 * ULP * m.scale


@pytest.mark.parametrize("fused", [False, True])
def test_zeros_init_first_loss_is_log_c(dev, tmp_path, monkeypatch, fused):
    tr = _trainer(tmp_path / "0", dev, fused, init="zeros")
    assert not tr.model.classifier.weight.any() and not tr.model.classifier.bias.any()
    losses = _train(tr, monkeypatch)
    print(f"zeros init (fused {fused}): first loss {losses[0]!r} log 6 {math.log(6)!r}")
    assert abs(losses[0] - math.log(6)) <= 16 * ULP * math.log(6)


def _on_against_off(dev, tmp_path, monkeypatch, **kw):
    off = _trainer(tmp_path / "off", dev, False, **kw)
    on = _trainer(tmp_path / "on", dev, True, **kw)
    for (k, p), (k2, p2) in zip(off.model.named_parameters(), on.model.named_parameters()):
        assert k == k2 and torch.equal(p, p2)  # the same start
    frozen = {k: v.detach().clone() for k, v in on.model.clip_model.state_dict().items()}
    frozen.update({"param." + k: p.detach().clone() for k, p in on.model.clip_model.named_parameters()})
    start = {k: p.detach().clone() for k, p in on.model.named_parameters() if p.requires_grad}
    assert sorted(start) == ["classifier.bias", "classifier.weight"]
    l_off = _train(off, monkeypatch, 0)
    l_on = _train(on, monkeypatch, 4)
    print("linear probe step losses off", l_off, "on", l_on, kw)
    assert rel_err(l_on[0], l_off[0]) <= 1e-4
    for k, p in on.model.named_parameters():
        if k in start:
            assert not torch.equal(p.detach(), start[k]), k  # it moved
    assert frozen
    now = dict(on.model.clip_model.state_dict())
    now.update({"param." + k: p for k, p in on.model.clip_model.named_parameters()})
    assert sorted(now) == sorted(frozen)
    for k, v in frozen.items():
        assert torch.equal(now[k].detach(), v), k
    return on


def test_fused_trainer_against_unfused_and_checkpoint(dev, tmp_path, monkeypatch):
    on = _on_against_off(dev, tmp_path, monkeypatch)
    path = os.path.join(str(tmp_path / "on"), "classifier", "model.pth.tar-2")
    assert os.path.exists(path)
    assert on.get_model_names() == ["classifier"]
    ck = on.load_checkpoint(path)
    assert sorted(ck["state_dict"]) == ["bias", "weight"]
    tr2 = _trainer(tmp_path / "on2", dev, True)
    assert not torch.equal(tr2.model.classifier.weight, on.model.classifier.weight)
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.load_model(str(tmp_path / "on"), epoch=2)
        acc = tr2.test()
    assert torch.equal(tr2.model.classifier.weight, on.model.classifier.weight)
    assert torch.equal(tr2.model.classifier.bias, on.model.classifier.bias)
    assert np.isfinite(acc) and 0.0 <= acc <= 100.0


def test_loss_type_focal(dev, tmp_path, monkeypatch):
    from fsp_amd.trainers.losses import focal_alpha
    on = _on_against_off(dev, tmp_path, monkeypatch, loss_type="focal", shots=SHOTS)
    assert ">> Use Focal Loss!" in on.build_log
    assert on.model.focal and on.model.gamma == 2.0
    assert on.model.alpha.tolist() == pytest.approx(focal_alpha(SHOTS, 6, zero_guard=True))


def test_unknown_keys_raise(dev, tmp_path):
    with pytest.raises(ValueError):
        _trainer(tmp_path / "x", dev, False, loss_type="x")
    with pytest.raises(ValueError):
        _trainer(tmp_path / "y", dev, False, init="x")


def _count_encoder(tr):
    """Wrap the model's feature method: the epochs in which the image encoder ran."""
    ran = []
    real = tr.model.image_features

    def counted(image):
        ran.append(tr.epoch)
        return real(image)

    tr.model.image_features = counted
    return ran


@pytest.mark.parametrize("fused", [False, True])
def test_feature_cache_replays_the_first_epoch(dev, tmp_path, monkeypatch, fused):
    plain = _trainer(tmp_path / "p", dev, fused, epochs=3)
    cached = _trainer(tmp_path / "c", dev, fused, cache=True, shuffle=False, epochs=3)
    ran_plain, ran = _count_encoder(plain), _count_encoder(cached)
    l_plain = _train(plain, monkeypatch, 6 if fused else 0)
    seen = []
    l_cached = _train(cached, monkeypatch, 6 if fused else 0, seen=seen)
    print(f"feature cache (fused {fused}): uncached {l_plain} cached {l_cached}")
    assert ran_plain == [0, 0, 1, 1, 2, 2]
    assert ran == [0, 0]  # 2 batches in epoch 0, none afterwards
    assert len(cached.bank) == 8 and cached.bank.num_stored_batches == 2
    assert [("feat" in b) for _, b in seen] == [False, False, True, True, True, True]
    assert len(l_cached) == 6
    for a, b in zip(l_cached, l_plain):
        assert rel_err(a, b) <= 1e-4


def test_feature_cache_shuffle_consumes_every_row_once(dev, tmp_path, monkeypatch):
    tr = _trainer(tmp_path / "s", dev, True, cache=True, shuffle=True, epochs=3)
    ran = _count_encoder(tr)
    seen = []
    _train(tr, monkeypatch, 6, seen=seen)
    assert ran == [0, 0] and len(tr.bank) == 8
    stored = torch.cat([f for f, _ in tr.bank.batches(4, False, False)])
    labels = torch.cat([y for _, y in tr.bank.batches(4, False, False)])
    assert len({tuple(r.tolist()) for r in stored}) == 8  # the rows are distinguishable
    for epoch in (1, 2):
        rows = []
        for e, b in seen:
            if e != epoch:
                continue
            assert b["feat"].shape == (4, stored.shape[1])
            for f, y in zip(b["feat"], b["label"]):
                hit = [i for i in range(8) if torch.equal(f, stored[i])]
                assert len(hit) == 1 and int(y) == int(labels[hit[0]])
                rows.append(hit[0])
        assert sorted(rows) == list(range(8)), (epoch, rows)
