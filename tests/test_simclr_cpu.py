"""CPU: the host side of end-to-end SimCLR training -- the NT-Xent kernel's C-ABI registration,
which configurations train on two views, the order of the two-view augmentation draws, the
synthetic two-view batches and the NATIVE.FUSED_SIMCLR default."""
import os
import re

import torch

from fsp_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntxent_symbols_are_registered():
    hdr = open(os.path.join(ROOT, "include", "clipk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("clipk_ntxent_loss", "clipk_ntxent_ws_bytes"):
        assert name in _native.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert len(_native.SIGNATURES["clipk_ntxent_loss"][1]) == 11
    assert "csrc/ntxent.hip" in [rel for rel, _ in _native.source_files()]


def test_ntxent_ws_bytes_on_the_host():
    """The workspace size is host arithmetic: positive inside the supported range, 0 outside."""
    lib = _native.load()
    for n, D in [(1, 8), (3, 5), (32, 1000), (512, 1030)]:
        N = 2 * n
        assert lib.clipk_ntxent_ws_bytes(n, D) >= 4 * (2 * N * N + 3 * N)
    for n, D in [(0, 8), (513, 8), (4, 0)]:
        assert lib.clipk_ntxent_ws_bytes(n, D) == 0


def test_two_views_selects_the_simclr_configurations():
    from fsp_amd.data.manager import two_views
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    assert not two_views(cfg)
    for name in ("CoOp", "CoCoOp", "IVLP", "MaPLe", "PromptSRC", "ZeroshotCLIP"):
        cfg = get_cfg_default()
        cfg.TRAINER.NAME = name
        assert not two_views(cfg), name  # the default losses
        cfg.TRAINER.COOP.LOSS_TYPE = "simclr"
        assert two_views(cfg) == (name == "CoOp"), name
        cfg.TRAINER.COOP.LOSS_TYPE = "focal"
        cfg.TRAINER.IVLP.SIMCLR_ALPHA = 0.5
        assert two_views(cfg) == (name == "IVLP"), name
        cfg.TRAINER.IVLP.SIMCLR_ALPHA = 0.0
        assert not two_views(cfg), name


def _transform(seed):
    from fsp_amd.data.preprocess import GpuTransform
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (64, 64)
    g = torch.Generator()
    g.manual_seed(seed)
    return GpuTransform(cfg, is_train=True, device="cpu", generator=g)


def _key(p):
    return (p.x0, p.y0, p.w, p.h, p.rw, p.rh, p.ox, p.oy, p.S, p.flip)


def test_two_view_plans_are_drawn_image_major():
    sizes = [(120, 90), (64, 200), (300, 300), (77, 131)]  # (w, h)
    two = _transform(7).plans(sizes, views=2)
    t = _transform(7)
    ref = [t.plan(w, h) for w, h in sizes for _ in range(2)]  # eight successive draws
    assert [_key(p) for p in two] == [_key(p) for p in ref]
    for k in range(len(sizes)):
        assert _key(two[2 * k]) != _key(two[2 * k + 1]), k  # the views of an image differ
    # one view: the stream the transform always drew
    one = _transform(7).plans(sizes)
    t = _transform(7)
    assert [_key(p) for p in one] == [_key(t.plan(w, h)) for w, h in sizes]


def test_synthetic_two_view_batches():
    from fsp_amd.data.synthetic import SyntheticDataManager
    dm = SyntheticDataManager(5, 32, 4, n_batches=2, device="cpu", two_views=True)
    plain = SyntheticDataManager(5, 32, 4, n_batches=2, device="cpu")
    assert len(dm.train_loader_x) == 2
    for b, p in zip(dm.train_loader_x, plain.train_loader_x):
        assert {"img", "img1", "img2", "label"} <= set(b)
        assert b["img1"] is b["img"]
        assert b["img2"].shape == b["img1"].shape and b["img2"].dtype == b["img1"].dtype
        assert not torch.equal(b["img2"], b["img1"])
        assert set(p) == {"img", "label"}  # the default batches are unchanged
        assert torch.equal(p["img"], b["img"]) and torch.equal(p["label"], b["label"])
    assert not torch.equal(dm.train_loader_x[0]["img2"], dm.train_loader_x[1]["img2"])


def test_fused_simclr_defaults_off():
    from fsp_amd.engine.config import get_cfg_default
    assert get_cfg_default().NATIVE.FUSED_SIMCLR is False


def test_fused_loss_falls_back_to_the_composition_off_device():
    """fused=True only takes CUDA fp32 inputs; CPU tensors run the unchanged torch composition."""
    from fsp_amd.trainers.losses import LogitsNTXentLoss
    from oracle import clip_oracle as O
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(3, 5, generator=g), torch.randn(3, 5, generator=g)
    want = O.ntxent_logits_loss(a, b)
    assert torch.equal(LogitsNTXentLoss(fused=True)(a, b), want)
    assert torch.equal(LogitsNTXentLoss()(a, b), want)
