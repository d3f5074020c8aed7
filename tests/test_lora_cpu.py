"""CPU: the LoRA trainer's host side -- config defaults, registry name, the POSITION -> layer_mask
table, the refusals (dropout, the o projection / MLP), the four C-ABI exports, the checkpoint key
set, and the reference helper (tests/lora_util.py) against the hand-written dA / dB formula of
include/clipk.h in fp64."""
import os
import re

import pytest
import torch

from fsp_amd import _native
from lora_util import merged_weight, wgrad_reference, wgrad_inputs, ln_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = (("clipk_lora_merge", 14), ("clipk_lora_wgrad_ws_bytes", 3), ("clipk_lora_wgrad", 20),
           ("clipk_encoder_set_lora", 9))


def _cfg():
    from fsp_amd.engine.config import get_cfg_default
    return get_cfg_default()


def test_config_defaults_and_registry():
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    assert dict(_cfg().TRAINER.LORA) == {
        "RANK": 2, "ALPHA": 1, "PARAMS": ["q", "k", "v"], "ENCODER": "both", "POSITION": "all", "DROPOUT_RATE": 0.0,
        "PREC": "fp16", "LOSS_TYPE": "ce"}
    assert "LoRA" in TRAINER_REGISTRY.registered_names()
    from fsp_amd.trainers.lora import LoRA
    assert TRAINER_REGISTRY.get("LoRA") is LoRA


def _bits(*ranges):
    return sum(1 << l for lo, hi in ranges for l in range(lo, hi))


POSITION_TABLE = {
    # CLIP-LoRA's layer sets: thirds, halves, the last three
    12: {"all": _bits((0, 12)), "bottom": _bits((0, 4)), "mid": _bits((4, 8)), "up": _bits((8, 12)),
         "half-bottom": _bits((0, 6)), "half-up": _bits((6, 12)), "top3": _bits((9, 12))},
    24: {"all": _bits((0, 24)), "bottom": _bits((0, 8)), "mid": _bits((8, 16)), "up": _bits((16, 24)),
         "half-bottom": _bits((0, 12)), "half-up": _bits((12, 24)), "top3": _bits((21, 24))},
}


@pytest.mark.parametrize("layers", [12, 24])
def test_position_to_layer_mask(layers):
    from fsp_amd.trainers.lora import layer_mask, POSITIONS
    assert set(POSITIONS) == set(POSITION_TABLE[layers])
    for pos, want in POSITION_TABLE[layers].items():
        assert layer_mask(pos, layers) == want, pos
    with pytest.raises(ValueError):
        layer_mask("top1", layers)


def test_small_encoders_and_empty_sets():
    from fsp_amd.trainers.lora import layer_mask
    assert layer_mask("all", 4) == 0b1111 and layer_mask("top3", 4) == 0b1110 and layer_mask("top3", 2) == 0b11
    assert layer_mask("bottom", 2) == 0b01 and layer_mask("mid", 2) == 0b10
    with pytest.raises(ValueError):
        layer_mask("up", 2)  # names no layer
    with pytest.raises(ValueError):
        layer_mask("all", 33)


def test_refusals():
    from fsp_amd.trainers.lora import lora_spec, proj_mask
    assert proj_mask(["q"]) == 1 and proj_mask(["q", "v"]) == 5 and proj_mask(["q", "k", "v"]) == 7
    for bad in (["o"], ["q", "o"], ["mlp"], []):
        with pytest.raises(ValueError):
            proj_mask(bad)
    sec = _cfg().TRAINER.LORA
    spec = lora_spec(sec, 12)
    assert (spec.rank, spec.scale, spec.proj_mask, spec.layer_mask) == (2, 0.5, 7, 0xfff)
    sec.DROPOUT_RATE = 0.25
    with pytest.raises(ValueError, match="DROPOUT_RATE"):
        lora_spec(sec, 12)
    sec.DROPOUT_RATE = 0.0
    sec.PARAMS = ["q", "k", "v", "o"]
    with pytest.raises(ValueError, match="o projection"):
        lora_spec(sec, 12)
    sec.PARAMS = ["q"]
    sec.ENCODER = "image"
    with pytest.raises(ValueError, match="ENCODER"):
        lora_spec(sec, 12)
    sec.ENCODER = "both"
    sec.RANK = 17
    with pytest.raises(ValueError, match="rank"):
        lora_spec(sec, 12)


def test_lora_symbols_are_registered():
    hdr = open(os.path.join(ROOT, "include", "clipk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in EXPORTS:
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == nargs
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs  # the header's own count
        assert hasattr(_native.load(), name)
    assert "csrc/lora.hip" in [rel for rel, _ in _native.source_files()]
    mk = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\blora\.hip\b", mk, flags=re.M)


def test_checkpoint_key_set():
    from fsp_amd.clip import synth
    from fsp_amd.trainers.lora import LoraAdapters
    a = synth.ARCHS["ViT-B/16"]
    ad = LoraAdapters(a, 2)
    sd = ad.state_dict()
    assert set(sd) == {"text.lora_A", "text.lora_B", "visual.lora_A", "visual.lora_B"}
    assert tuple(sd["text.lora_A"].shape) == (12, 3, 2, 512) and tuple(sd["text.lora_B"].shape) == (12, 3, 512, 2)
    assert tuple(sd["visual.lora_A"].shape) == (12, 3, 2, 768) and tuple(sd["visual.lora_B"].shape) == (12, 3, 768, 2)
    # kaiming_uniform(a = sqrt 5) on [r, W]: U(-1 / sqrt W, 1 / sqrt W); B = 0
    for side, W in (("text", 512), ("visual", 768)):
        A = sd[side + ".lora_A"]
        assert float(A.abs().max()) <= W ** -0.5 and float(A.abs().max()) > 0.9 * W ** -0.5
        assert abs(float(A.mean())) < 0.01 * W ** -0.5 * 10
        assert not sd[side + ".lora_B"].any()
    assert all(v.dtype == torch.float32 for v in sd.values())


@pytest.mark.parametrize("proj_mask", [1, 5, 7])
@pytest.mark.parametrize("r", [1, 2, 16])
def test_helper_gradients_equal_the_hand_written_formula(r, proj_mask):
    """Autograd through merged_weight (what lora_params feeds the oracle) on y = LN1(X) W'^T + b
    against dA / dB of include/clipk.h, fp64."""
    rows, W, s = 37, 64, 0.5
    X, gamma, beta, dY, A, B = (t.double() for t in wgrad_inputs(rows, W, r, seed=11 * r + proj_mask))
    mean, rstd = (t.double() for t in ln_stats(X.float()))
    w0 = torch.randn(3 * W, W, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 0.05
    A.requires_grad_(True)
    B.requires_grad_(True)
    xn = (X - mean[:, None]) * rstd[:, None] * gamma + beta
    y = xn @ merged_weight(w0, A, B, s, proj_mask).t()
    (y * dY).sum().backward()
    dA, dB = wgrad_reference(X, mean, rstd, gamma, beta, dY, A.detach(), B.detach(), s, proj_mask)
    assert float(dA.abs().max()) > 1e-6 and float(dB.abs().max()) > 1e-6
    assert float((A.grad - dA).abs().max()) <= 1e-12 * max(1.0, float(dA.abs().max()))
    assert float((B.grad - dB).abs().max()) <= 1e-12 * max(1.0, float(dB.abs().max()))
    for p in range(3):
        if not (proj_mask >> p) & 1:
            assert not dA[p].any() and not dB[p].any() and not A.grad[p].any() and not B.grad[p].any()


def test_ops_refuse_cpu_tensors():
    from fsp_amd import ops
    X, gamma, beta, dY, A, B = wgrad_inputs(4, 64, 2, seed=1)
    mean, rstd = ln_stats(X)
    with pytest.raises(_native.ClipkError):
        ops.lora_wgrad(X, mean, rstd, gamma, beta, dY, A, B, 7, 0.5)
    w0 = [torch.zeros(192, 64)]
    with pytest.raises(_native.ClipkError):
        ops.lora_merge(w0, A[None], B[None], 7, 1, 0.5, [torch.zeros(192, 64)])
