"""GPU: SimCLR training from the loader to the optimizer step with NATIVE.FUSED_SIMCLR.

* the reference-written fixture coop_tiny_end_simclr through the fused path (native NT-Xent, one
  text encode for both views) at the gates tests/test_parity_gpu.py applies to it;
* the registry-built CoOp trainer on SyntheticDataManager(two_views=True) and IVLP with
  SIMCLR_ALPHA: key on against key off at the project's gate for fp32 re-orderings
  (loss / parameters rel <= 1e-4, gradients rel <= 1e-3);
* two-view preprocessing: one upload and one resample launch give exactly the two per-view
  preprocess_batch results; GpuLoader(views=2) batches.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

from parity_util import load_fixture, make_cfg, rel_err, state_dict

pytestmark = pytest.mark.gpu

FIXTURE = "coop_tiny_end_simclr"


def _count_text_encodes(monkeypatch):
    from fsp_amd.trainers import coop as C
    calls = []
    orig = C.CustomCLIP.text_features

    def counting(self):
        calls.append(1)
        return orig(self)

    monkeypatch.setattr(C.CustomCLIP, "text_features", counting)
    return calls


def _run_fixture(prec, fused, dev, monkeypatch):
    """tests/parity_util.py run_native's training half for the SimCLR fixture, with the key."""
    from fsp_amd.clip import synth
    from fsp_amd.clip.model import build_model
    from fsp_amd.engine.optim import FusedSGD
    from fsp_amd.trainers import coop as C
    meta, ref = load_fixture(FIXTURE)
    assert meta["loss_type"] == "simclr"
    a = synth.ARCHS[meta["arch"]]
    cfg = make_cfg(meta, prec)
    cfg.NATIVE.FUSED_SIMCLR = fused
    clip = build_model(state_dict(meta["arch"]), prec=prec, device=str(dev))
    with contextlib.redirect_stdout(io.StringIO()):
        model = C.CustomCLIP(cfg, synth.synthetic_classnames(meta["n_cls"]), clip)
    pl = model.prompt_learner
    with torch.no_grad():
        pl.ctx.copy_(torch.from_numpy(ref["ctx0"]).to(dev))
    for n, p in model.named_parameters():
        p.requires_grad_("prompt_learner" in n)
    B = meta["batch"]
    img = torch.from_numpy(synth.make_images(B, a.image_resolution, seed=1)).to(dev)
    img2 = torch.from_numpy(synth.make_images(B, a.image_resolution, seed=5)).to(dev)
    model.train()
    calls = _count_text_encodes(monkeypatch)
    loss = model(img, None, img2)
    n_encodes = len(calls)
    loss.backward()
    out = {"loss": float(loss.item()), "grad_ctx": pl.ctx.grad.detach().cpu().numpy(), "text_encodes": n_encodes}
    FusedSGD([p for p in pl.parameters() if p.requires_grad], lr=0.002, momentum=0.9, weight_decay=5e-4).step()
    out["ctx_after_step"] = pl.ctx.detach().cpu().numpy()
    return ref, out


@pytest.mark.parametrize("prec", ["fp32", "fp32s"])
def test_fixture_through_the_fused_path(dev, prec, monkeypatch):
    ref, out = _run_fixture(prec, True, dev, monkeypatch)
    report = {"loss": rel_err(out["loss"], ref["loss"]), "grad_ctx": rel_err(out["grad_ctx"], ref["grad_ctx"]),
              "step": rel_err(out["ctx_after_step"], ref["ctx_after_step"])}
    print(FIXTURE, prec, "fused", report)
    assert out["text_encodes"] == 1  # both views scored against one encode of the class prompts
    assert report["loss"] <= 1e-4
    assert report["grad_ctx"] <= 1e-3
    assert report["step"] <= 1e-4


def test_unfused_path_encodes_the_prompts_per_view(dev, monkeypatch):
    _, out = _run_fixture("fp32", False, dev, monkeypatch)
    assert out["text_encodes"] == 2  # the reference's two forward_once calls, unchanged


def _coop_trainer(outdir, fused, dev):
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.data.synthetic import SyntheticDataManager
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.OUTPUT_DIR = str(outdir)
    cfg.OPTIM.MAX_EPOCH = 2
    cfg.TEST.NO_TEST = True
    cfg.TRAINER.NAME = "CoOp"
    c = cfg.TRAINER.COOP
    c.N_CTX, c.PREC, c.LOSS_TYPE = 4, "fp32", "simclr"
    cfg.NATIVE.FUSED_SIMCLR = fused
    dm = SyntheticDataManager(5, 32, 4, n_batches=2, device=dev, two_views=True)
    with contextlib.redirect_stdout(io.StringIO()):
        return TRAINER_REGISTRY.get("CoOp")(cfg, dm=dm)


def test_coop_trainer_simclr_fused_matches_unfused(dev, tmp_path):
    from fsp_amd.clip import synth
    assert synth.ARCHS["tiny"].image_resolution == 32
    runs = {}
    ctx0 = None
    for fused in (False, True):
        tr = _coop_trainer(tmp_path / f"out{int(fused)}", fused, dev)
        pl = tr.model.prompt_learner
        with torch.no_grad():
            if ctx0 is None:
                ctx0 = pl.ctx.detach().clone()
            else:
                pl.ctx.copy_(ctx0)
        losses = []
        fb = tr.forward_backward
        tr.forward_backward = lambda b, fb=fb, losses=losses: losses.append(float(fb(b)["loss"])) or {"loss": losses[-1]}
        with contextlib.redirect_stdout(io.StringIO()):
            for tr.epoch in range(tr.max_epoch):
                tr.run_epoch()
                tr.after_epoch()
        runs[fused] = (np.asarray(losses), pl.ctx.detach().cpu().numpy())
    (l0, c0), (l1, c1) = runs[False], runs[True]
    print("coop simclr trainer: loss off", l0, "on", l1, "rel", rel_err(l1, l0), "ctx rel", rel_err(c1, c0))
    for losses in (l0, l1):
        assert len(losses) == 4 and np.isfinite(losses).all()
        assert len(set(losses.tolist())) > 1  # the loss changes across steps
    assert not np.array_equal(c0, ctx0.cpu().numpy())  # ... and the prompts move
    assert rel_err(l1, l0) <= 1e-4
    assert rel_err(c1, c0) <= 1e-4


def _ivlp_model(fused, dev):
    from fsp_amd.clip import synth
    from fsp_amd.clip.model import build_model
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.trainers import deep as D
    a = synth.ARCHS["tiny4"]
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (a.image_resolution, a.image_resolution)
    cfg.TRAINER.NAME = "IVLP"
    cfg.NATIVE.FUSED_SIMCLR = fused
    s = cfg.TRAINER.IVLP
    s.PREC, s.SIMCLR_ALPHA = "fp32", 0.5
    s.PROMPT_DEPTH_TEXT = s.PROMPT_DEPTH_VISION = 3
    clip = build_model(state_dict("tiny4"), prec="fp32", device=str(dev), vision_grad=True)
    torch.manual_seed(11)  # the prompts' random init, the same for both models
    with contextlib.redirect_stdout(io.StringIO()):
        model = D.IVLPCustomCLIP(cfg, synth.synthetic_classnames(6), clip, s).to(dev)
    for k, p in model.named_parameters():
        p.requires_grad_(("prompt_learner" in k) or ("VPT" in k))
    return model, a


def test_ivlp_simclr_fused_matches_unfused(dev, monkeypatch):
    from fsp_amd import ops
    from fsp_amd.clip import synth
    native_calls = []
    orig = ops.ntxent_loss
    monkeypatch.setattr(ops, "ntxent_loss", lambda *a, **k: native_calls.append(1) or orig(*a, **k))
    out = {}
    for fused in (False, True):
        model, a = _ivlp_model(fused, dev)
        img1 = torch.from_numpy(synth.make_images(4, a.image_resolution, seed=1)).to(dev)
        img2 = torch.from_numpy(synth.make_images(4, a.image_resolution, seed=5)).to(dev)
        lbl = torch.from_numpy(synth.make_labels(4, 6, seed=2)).to(dev)
        model.train()
        before = len(native_calls)
        loss = model(img1, lbl, img2)
        loss.backward()
        assert len(native_calls) - before == (1 if fused else 0)
        grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if p.requires_grad}
        assert grads and all(np.isfinite(g).all() for g in grads.values())
        out[fused] = (float(loss.item()), grads,
                      {k: p.detach().cpu().numpy() for k, p in model.named_parameters() if p.requires_grad})
    (l0, g0, p0), (l1, g1, p1) = out[False], out[True]
    assert all(np.array_equal(p0[k], p1[k]) for k in p0)  # the same initial prompts
    report = {k: rel_err(g1[k], g0[k]) for k in g0}
    print("ivlp simclr: loss off", l0, "on", l1, "grad rel", report)
    assert np.isfinite(l0) and rel_err(l1, l0) <= 1e-4
    for k, r in report.items():
        assert r <= 1e-3, (k, r)


def _images():
    rs = np.random.RandomState(21)
    return [rs.randint(0, 256, size=(int(rs.randint(60, 301)), int(rs.randint(60, 301)), 3), dtype=np.uint8)
            for _ in range(6)]


def _transform(seed, dev):
    from fsp_amd.data.preprocess import GpuTransform
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (64, 64)
    g = torch.Generator()
    g.manual_seed(seed)
    return GpuTransform(cfg, is_train=True, device=dev, generator=g)


def test_two_view_preprocessing_equals_per_view_calls(dev):
    from fsp_amd.data.preprocess import preprocess_batch
    images = _images()
    t = _transform(5, dev)
    x1, x2 = t(images, views=2)
    ref_t = _transform(5, dev)
    plans = ref_t.plans([(im.shape[1], im.shape[0]) for im in images], views=2)
    r1 = preprocess_batch(images, plans[0::2], ref_t.mean, ref_t.std, dev)
    r2 = preprocess_batch(images, plans[1::2], ref_t.mean, ref_t.std, dev)
    assert x1.shape == x2.shape == (6, 3, 64, 64)
    assert torch.equal(x1, r1) and torch.equal(x2, r2)
    assert not torch.equal(x1, x2)
    base = x1._base
    assert base is not None and x2._base is base and base.shape == (12, 3, 64, 64)
    assert x1.data_ptr() == base.data_ptr() and x2.data_ptr() == base.data_ptr() + x1.numel() * 4
    # one view: unchanged
    assert torch.equal(_transform(9, dev)(images), preprocess_batch(
        images, _transform(9, dev).plans([(im.shape[1], im.shape[0]) for im in images]), t.mean, t.std, dev))


def test_preprocess_src_index_validates_against_the_source_image(dev):
    from fsp_amd.data.preprocess import Plan, preprocess_batch
    small = np.zeros((60, 60, 3), np.uint8)
    big = np.zeros((200, 200, 3), np.uint8)
    p = Plan(0, 0, 150, 150, 64, 64, 0, 0, 64, False)  # fits `big` only
    assert preprocess_batch([small, big], [p, p], device=dev, src_index=[1, 1]).shape == (2, 3, 64, 64)
    with pytest.raises(ValueError):
        preprocess_batch([small, big], [p, p], device=dev, src_index=[0, 1])
    with pytest.raises(ValueError):
        preprocess_batch([small, big], [p, p], device=dev, src_index=[1, 2])


def test_gpu_loader_two_views(dev):
    from fsp_amd.data.manager import GpuLoader
    images = _images()
    host = [{"img": images[:3], "label": torch.tensor([0, 1, 2]), "index": torch.tensor([0, 1, 2]), "n_global": 3,
             "n_local": 3},
            {"img": images[3:], "label": torch.tensor([3, 4, 0]), "index": torch.tensor([3, 4, 5]), "n_global": 3,
             "n_local": 3}]
    batches = list(GpuLoader(host, _transform(5, dev), dev, views=2))
    assert len(batches) == 2
    for b, h in zip(batches, host):
        assert {"img", "img1", "img2", "label", "index", "n_global", "n_local"} <= set(b)
        assert b["img"] is b["img1"]
        assert b["img1"].shape == b["img2"].shape == (3, 3, 64, 64) and b["img1"].device.type == "cuda"
        assert not torch.equal(b["img1"], b["img2"])
        assert b["label"].device.type == "cuda" and torch.equal(b["label"].cpu(), h["label"])
    one = list(GpuLoader(host, _transform(5, dev), dev))
    assert all("img1" not in b and "img2" not in b for b in one)
