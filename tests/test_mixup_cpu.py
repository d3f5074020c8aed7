"""CPU: the host side of IVLP mixup training -- the two kernels' C-ABI registration, which
configurations mix their training batches, the loader's mixed batches (stub transform, CPU tensors),
the seeded Beta draw, the synthetic mixed batches and ops.mixup_images' host validation."""
import os
import re

import numpy as np
import pytest
import torch

from fsp_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixup_symbols_are_registered():
    hdr = open(os.path.join(ROOT, "include", "clipk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("clipk_mixup_images", 10), ("clipk_ce_loss_mix", 15)):
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == nargs
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(_native.load(), name)
    assert "csrc/mixup.hip" in [rel for rel, _ in _native.source_files()]


def test_native_mixup_defaults_off():
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    assert cfg.NATIVE.MIXUP is False
    assert cfg.TRAINER.IVLP.USE_MIXUP is True and cfg.TRAINER.IVLP.MIXUP_ALPHA == 1.0


def test_mixup_truth_table():
    from fsp_amd.data.manager import mixup, two_views
    from fsp_amd.engine.config import get_cfg_default
    assert not mixup(get_cfg_default())
    for name in ("CoOp", "CoCoOp", "IVLP", "MaPLe", "PromptSRC", "ZeroshotCLIP"):
        for use in (False, True):
            for native in (False, True):
                for simclr in (0.0, 0.5):
                    cfg = get_cfg_default()
                    cfg.TRAINER.NAME = name
                    cfg.TRAINER.IVLP.USE_MIXUP = use
                    cfg.NATIVE.MIXUP = native
                    cfg.TRAINER.IVLP.SIMCLR_ALPHA = simclr
                    want = name == "IVLP" and use and native and simclr == 0.0
                    assert mixup(cfg) == want, (name, use, native, simclr)
                    assert not (mixup(cfg) and two_views(cfg))  # the SimCLR batch form wins
    cfg = get_cfg_default()  # CoOp's SimCLR does not turn IVLP's mixing off, nor on for CoOp
    cfg.TRAINER.COOP.LOSS_TYPE = "simclr"
    cfg.NATIVE.MIXUP = True
    cfg.TRAINER.NAME = "CoOp"
    assert not mixup(cfg)
    cfg.TRAINER.NAME = "IVLP"
    assert mixup(cfg)


class _StubTransform:
    """Stands in for GpuTransform on CPU tensors: one 'crop' draw per image from its generator, then
    the stacked images."""

    def __init__(self, seed):
        self.generator = torch.Generator()
        self.generator.manual_seed(seed)
        self.crops = []

    def __call__(self, images):
        self.crops.append([float(torch.rand(1, generator=self.generator)) for _ in images])
        return torch.stack(images)


def _host_batches():
    g = torch.Generator().manual_seed(3)
    out = []
    for k, n in enumerate((5, 4)):
        out.append({"img": [torch.randn(3, 6, 5, generator=g) for _ in range(n)],
                    "label": torch.randint(0, 7, (n,), generator=g), "index": torch.arange(n) + 10 * k,
                    "n_global": n, "n_local": n})
    return out


def test_gpu_loader_mixes_cpu_batches():
    from fsp_amd.data.manager import GpuLoader, draw_mix
    host = _host_batches()
    batches = list(GpuLoader(host, _StubTransform(5), "cpu", mixup_alpha=1.0))
    again = list(GpuLoader(host, _StubTransform(5), "cpu", mixup_alpha=1.0))
    other = list(GpuLoader(host, _StubTransform(6), "cpu", mixup_alpha=1.0))
    # the stream the loader must have drawn: per batch the crops, then lam, then the permutation
    ref_t = _StubTransform(5)
    assert len(batches) == 2
    for b, b2, h in zip(batches, again, host):
        x = ref_t(h["img"])
        lam, perm = draw_mix(1.0, len(h["img"]), ref_t.generator)
        assert {"img", "label", "y_a", "y_b", "lam", "index", "n_global", "n_local"} <= set(b)
        assert "img1" not in b and "img2" not in b
        assert type(b["lam"]) is float and 0.0 < b["lam"] < 1.0 and b["lam"] == lam
        assert torch.equal(b["label"], h["label"]) and torch.equal(b["y_a"], h["label"])
        assert sorted(perm.tolist()) == list(range(len(perm)))
        assert torch.equal(b["y_b"], h["label"][perm])
        assert b["img"].dtype == torch.float32 and b["img"].shape == x.shape
        assert torch.equal(b["img"], lam * x + (1 - lam) * x[perm])  # bitwise the torch expression
        assert not torch.equal(b["img"], x)
        # the same seed: the same mix
        assert b2["lam"] == b["lam"] and torch.equal(b2["y_b"], b["y_b"]) and torch.equal(b2["img"], b["img"])
    assert batches[0]["lam"] != batches[1]["lam"]
    assert [b["lam"] for b in other] != [b["lam"] for b in batches]
    # no mixup_alpha: the batches every loader gave so far
    plain = list(GpuLoader(host, _StubTransform(5), "cpu"))
    for b, h in zip(plain, host):
        assert not {"y_a", "y_b", "lam"} & set(b)
        assert torch.equal(b["img"], torch.stack(h["img"]))
    with pytest.raises(ValueError):
        GpuLoader(host, _StubTransform(5), "cpu", views=2, mixup_alpha=1.0)


@pytest.mark.parametrize("alpha", [0.0, -1.0])
def test_gpu_loader_alpha_not_positive_leaves_the_batch_unmixed(alpha):
    from fsp_amd.data.manager import GpuLoader
    host = _host_batches()
    for b, h in zip(GpuLoader(host, _StubTransform(5), "cpu", mixup_alpha=alpha), host):
        assert b["lam"] == 1.0 and type(b["lam"]) is float
        assert torch.equal(b["img"], torch.stack(h["img"]))
        assert torch.equal(b["y_a"], h["label"]) and b["y_b"].shape == h["label"].shape
        assert sorted(b["y_b"].tolist()) == sorted(h["label"].tolist())


@pytest.mark.parametrize("alpha", [1.0, 0.2])
def test_lam_draws_follow_beta(alpha):
    """2,000 seeded draws: Beta(alpha, alpha) has mean 1/2 and variance 1 / (4 (2 alpha + 1))."""
    from fsp_amd.data.manager import draw_mix
    g = torch.Generator().manual_seed(1234)
    lams = np.array([draw_mix(alpha, 4, g)[0] for _ in range(2000)])
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    print("alpha", alpha, "mean", lams.mean(), "var", lams.var(), "want", 0.5, var)
    assert ((lams >= 0.0) & (lams <= 1.0)).all()
    assert abs(lams.mean() - 0.5) <= 0.03
    assert abs(lams.var() - var) <= 0.10 * var
    g2 = torch.Generator().manual_seed(1234)
    assert [draw_mix(alpha, 4, g2)[0] for _ in range(5)] == lams[:5].tolist()


def test_mixup_images_host_validation(monkeypatch):
    from fsp_amd import ops
    calls = []
    monkeypatch.setattr(_native, "call", lambda *a: calls.append(a))
    x = torch.randn(4, 3, 2, 2)
    good = torch.tensor([1, 0, 3, 2])
    for perm in (torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2, 3, 0]), torch.tensor([0, 1, 2, 4]),
                 torch.tensor([-1, 1, 2, 3]), torch.tensor([[0, 1, 2, 3]]), torch.tensor([0.0, 1.0, 2.0, 3.0]), None):
        with pytest.raises(_native.ClipkError):
            ops.mixup_images(x, perm, 0.3)
    for bad in (x.double(), x.half(), x.long()):
        with pytest.raises(_native.ClipkError):
            ops.mixup_images(bad, good, 0.3)
    with pytest.raises(_native.ClipkError):
        ops.mixup_images(x, good, 0.3, labels=torch.tensor([0, 1, 2]))
    with pytest.raises(_native.ClipkError):
        ops.mixup_images(x, good, 0.3, labels=torch.tensor([0, 1, 2, 3], dtype=torch.int32))
    assert not calls
    # ... and what passes evaluates the torch expression on CPU tensors, still without a call
    lab = torch.tensor([5, 6, 7, 8])
    mixed, y_b = ops.mixup_images(x, good, 0.3, lab)
    assert torch.equal(mixed, 0.3 * x + (1 - 0.3) * x[good]) and torch.equal(y_b, lab[good])
    mixed, y_b = ops.mixup_images(x, good.int(), 1.0)
    assert torch.equal(mixed, x) and y_b is None
    assert not calls


def test_synthetic_mixed_batches():
    from fsp_amd.data.synthetic import SyntheticDataManager
    dm = SyntheticDataManager(5, 32, 4, n_batches=2, device="cpu", mixup_alpha=1.0)
    same = SyntheticDataManager(5, 32, 4, n_batches=2, device="cpu", mixup_alpha=1.0)
    plain = SyntheticDataManager(5, 32, 4, n_batches=2, device="cpu")
    assert len(dm.train_loader_x) == 2
    for b, s, p in zip(dm.train_loader_x, same.train_loader_x, plain.train_loader_x):
        assert set(p) == {"img", "label"}  # the default batches are unchanged
        assert set(b) == {"img", "label", "y_a", "y_b", "lam"}
        assert type(b["lam"]) is float and 0.0 < b["lam"] < 1.0
        assert torch.equal(b["label"], p["label"]) and torch.equal(b["y_a"], p["label"])
        # y_b is a permutation of the labels and img the matching mix of the plain images
        perms = [q for q in torch.tensor(_perms(4)) if torch.equal(p["label"][q], b["y_b"])]
        lam = b["lam"]
        assert any(torch.equal(b["img"], lam * p["img"] + (1 - lam) * p["img"][q]) for q in perms)
        assert b["lam"] == s["lam"] and torch.equal(b["img"], s["img"]) and torch.equal(b["y_b"], s["y_b"])
    assert dm.train_loader_x[0]["lam"] != dm.train_loader_x[1]["lam"]
    unmixed = SyntheticDataManager(5, 32, 4, n_batches=1, device="cpu", mixup_alpha=0.0).train_loader_x[0]
    assert unmixed["lam"] == 1.0 and torch.equal(unmixed["img"], plain.train_loader_x[0]["img"])
    with pytest.raises(ValueError):
        SyntheticDataManager(5, 32, 4, device="cpu", two_views=True, mixup_alpha=1.0)


def _perms(n):
    import itertools
    return list(itertools.permutations(range(n)))
