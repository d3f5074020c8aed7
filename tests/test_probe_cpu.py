"""CPU: the host side of the linear probe -- the C-ABI registration of clipk_probe_head, the config
defaults and the trainer's registration, the closed-form gradient the kernels implement (pinned
against autograd through the fp64 reference), ops.probe_head's refusal of CPU tensors, and the
FeatureBank.

clipk_probe_head takes 19 arguments as include/clipk.h declares it (3 sizes, feat, w, bias, labels,
alpha, gamma, focal, normalize, scale, grad_scale, loss, logits, 2 gradients, ws, stream)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from fsp_amd import _native
from probe_util import inputs, reference, MODES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_probe_head_symbols_are_registered():
    hdr = open(os.path.join(ROOT, "include", "clipk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("clipk_probe_head", 19), ("clipk_probe_head_ws_bytes", 3)):
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == nargs
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs  # the header's own count
        assert hasattr(_native.load(), name)
    assert "csrc/probe.hip" in [rel for rel, _ in _native.source_files()]


def test_config_defaults_and_registry():
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd import ops
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    cfg = get_cfg_default()
    assert dict(cfg.TRAINER.LINEAR_PROBE) == {
        "PREC": "fp16", "LOSS_TYPE": "ce", "NORMALIZE": True, "BIAS": True, "INIT": "zeroshot", "LOGIT_SCALE": 0.0,
        "CACHE_FEATURES": False, "CACHE_SHUFFLE": True}
    assert cfg.NATIVE.FUSED_PROBE is False
    assert ops.PROBE_HEAD_MAX_B == 512
    assert "LinearProbeCLIP" in TRAINER_REGISTRY.registered_names()
    from fsp_amd.trainers.linear_probe import LinearProbeCLIP, LinearProbeModel  # noqa: F401
    assert TRAINER_REGISTRY.get("LinearProbeCLIP") is LinearProbeCLIP


def closed_form(feat, w, bias, y, normalize, scale, alpha=None, focal=False, gamma=2.0):
    """The gradient clipk_probe_head documents (include/clipk.h), restated in fp64 torch without
    autograd: (d_w, d_bias or None)."""
    f, w = feat.double(), w.double()
    B, C = f.shape[0], w.shape[0]
    u = f / f.norm(dim=-1, keepdim=True).clamp_min(1e-12) if normalize else f
    s = scale * u @ w.t()
    if bias is not None:
        s = s + bias.double()
    p = torch.softmax(s, dim=1)
    onehot = F.one_hot(y, C).double()
    wgt = torch.ones(B, dtype=torch.float64)
    if focal:
        ce = -torch.log_softmax(s, dim=1)[torch.arange(B), y]
        pt = torch.exp(-ce)
        a = alpha.double()[y] if alpha is not None else 1.0
        wgt = a * ((1 - pt) ** gamma + gamma * pt * (1 - pt) ** (gamma - 1) * ce)
    G = wgt[:, None] / B * (p - onehot)
    return scale * G.t() @ u, (G.sum(0) if bias is not None else None)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("focal", [False, True])
@pytest.mark.parametrize("normalize,scale", MODES)
def test_closed_form_gradient_equals_autograd_through_the_reference(normalize, scale, focal, with_bias):
    feat, w, bias, y, alpha = inputs(3, 7, 64)
    b = bias if with_bias else None
    a = alpha if focal else None
    _, d_w64, d_b64, _ = reference(feat, w, b, y, normalize, scale, a, focal)
    d_w, d_b = closed_form(feat, w, b, y, normalize, scale, a, focal)
    e_w = float((d_w - d_w64).abs().max())
    print(f"closed form (3, 7, 64) normalize {normalize} scale {scale} focal {focal} bias {with_bias}: "
          f"|d_w| max {float(d_w64.abs().max()):.3e} err {e_w:.3e}")
    assert float(d_w64.abs().max()) > 1e-3
    assert e_w <= 1e-12
    if with_bias:
        assert float(d_b64.abs().max()) > 1e-3
        assert float((d_b - d_b64).abs().max()) <= 1e-12
    else:
        assert d_b is None and d_b64 is None


def test_probe_head_refuses_cpu_tensors():
    from fsp_amd import ops
    from fsp_amd.trainers._fns import probe_head_fused_ok
    feat, w, bias, y, _ = inputs(2, 3, 37)
    with pytest.raises(_native.ClipkError):
        ops.probe_head(feat, w, bias, y, None, 0.0, False, True, 100.0)
    with pytest.raises(_native.ClipkError):
        ops.probe_head(feat, w, bias, None, None, 0.0, False, True, 100.0)  # scoring only
    assert not probe_head_fused_ok(feat, w, bias)


def _bank(sizes=(4, 4, 3), E=5):
    from fsp_amd.data.feature_bank import FeatureBank
    bank = FeatureBank()
    stored, row = [], 0
    for n in sizes:
        # row i is recognisable: feat[i] = i everywhere, label = i
        f = torch.arange(row, row + n, dtype=torch.float32)[:, None].repeat(1, E)
        y = torch.arange(row, row + n)
        bank.add(f, y)
        stored.append((f, y))
        row += n
    return bank, stored, row


def test_feature_bank_shuffle_visits_every_row_once():
    bank, _, n = _bank()
    assert len(bank) == n == 11
    torch.manual_seed(5)
    orders = []
    for _ in range(3):
        rows = []
        batches = list(bank.batches(4, shuffle=True, drop_last=False))
        assert [f.shape[0] for f, _ in batches] == [4, 4, 3] and len(batches) == bank.num_batches(4, True, False)
        for f, y in batches:
            assert f.shape == (y.shape[0], 5) and torch.equal(f[:, 0].long(), y)  # rows stay with their labels
            rows += y.tolist()
        assert sorted(rows) == list(range(n))
        orders.append(rows)
    assert orders[0] != orders[1] or orders[1] != orders[2]  # a new permutation every epoch


def test_feature_bank_drop_last():
    bank, _, n = _bank()
    batches = list(bank.batches(4, shuffle=True, drop_last=True))
    assert [f.shape[0] for f, _ in batches] == [4, 4] and bank.num_batches(4, True, True) == 2
    seen = [i for _, y in batches for i in y.tolist()]
    assert len(set(seen)) == 8
    # the loader's rule as the trainer applies it: drop_last exactly when a full batch exists
    for bs, want in ((4, True), (11, True), (12, False)):
        assert (len(bank) >= bs) is want
    assert [f.shape[0] for f, _ in bank.batches(12, shuffle=True, drop_last=False)] == [11]
    assert list(bank.batches(12, shuffle=True, drop_last=True)) == []


def test_feature_bank_same_seed_same_order():
    bank, _, _ = _bank()
    runs = []
    for _ in range(2):
        torch.manual_seed(123)
        runs.append([y.tolist() for _ in range(2) for _, y in bank.batches(4, shuffle=True, drop_last=False)])
    assert runs[0] == runs[1]


def test_feature_bank_replays_stored_batches():
    bank, stored, _ = _bank()
    for _ in range(2):
        out = list(bank.batches(2, shuffle=False, drop_last=True))  # neither argument applies
        assert len(out) == len(stored) == bank.num_batches(2, False, True)
        for (f, y), (f0, y0) in zip(out, stored):
            assert torch.equal(f, f0) and torch.equal(y, y0)
    # the bank holds copies: changing the caller's tensors afterwards does not reach it
    stored[0][0].zero_()
    assert float(next(iter(bank.batches(4, False, False)))[0].abs().sum()) > 0
