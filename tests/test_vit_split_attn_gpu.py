"""PREC fp32s encoders on unpacked rows take the split attention forward (attn_fwd_split; knob
CLIPK_VIT_SPLIT_ATTN, default on, read at every call): the frozen ViT's forward-only clipk_vit_forward
-- in split mode 2 with o handed to out_proj pre-split -- and the saving forwards of the prompted ViT,
which keep an fp32 o for their backward."""
import numpy as np
import pytest
import torch

from parity_util import state_dict
from test_kernels_gpu import TOL

pytestmark = pytest.mark.gpu

KNOB = "CLIPK_VIT_SPLIT_ATTN"


@pytest.mark.parametrize("arch,fp16_values", [("ViT-B/32", True), ("ViT-B/32", False), ("ViT-B/16", True)])
def test_vit_forward_both_knob_settings_in_one_process(dev, monkeypatch, arch, fp16_values):
    """clipk_vit_forward under PREC fp32s (2 images; fp16-valued weights: split mode 2, the pre-split o;
    else mode 1, fp32 o): finite with the knob off and on, different bits (the new kernel ran), the
    knob-off path reproducible, and the two within the fp32-class distance the split GEMMs already have."""
    from fsp_amd.clip import synth
    from fsp_amd.clip.model import build_model
    a = synth.ARCHS[arch]
    clip = build_model(state_dict(arch, fp16_values=fp16_values), prec="fp32s", device=dev, vision_grad=False)
    assert clip.visual.split_mode == (2 if fp16_values else 1)
    img = torch.from_numpy(synth.make_images(2, a.image_resolution, seed=5)).to(dev)
    monkeypatch.setenv(KNOB, "0")
    off = clip.visual(img).clone()
    off2 = clip.visual(img).clone()
    monkeypatch.delenv(KNOB)
    on = clip.visual(img).clone()
    on2 = clip.visual(img).clone()
    assert torch.isfinite(off).all() and torch.isfinite(on).all()
    assert torch.equal(off, off2) and torch.equal(on, on2)
    assert not torch.equal(on, off), "the knob selects another attention kernel"
    d = float((on - off).abs().max() / off.abs().max())
    print(f"vit split attn {arch} mode {clip.visual.split_mode}: max |d feature| / max |feature| = {d:.3e}")


@pytest.mark.parametrize("name", ["ivlp_tiny4", "maple_vitb32_c3"])
def test_prompted_vit_backward_keeps_fp32_o(dev, monkeypatch, name):
    """A prompted-ViT forward + backward under fp32s (ivlp_tiny4: the smallest deep-prompt case of
    tests/test_deep_gpu.py, 9 rows per image, so the exact short kernel; maple_vitb32_c3: 50 + n rows, the
    split kernel). The choice made for a backward is to KEEP an fp32 o -- a saving forward never stores the
    pre-split form, so clipk_attention_bwd reads fp32 values -- and its logits, loss and gradients match the
    knob-off run under TOL[torch.float32] (relative to each tensor's max)."""
    from test_deep_gpu import run
    monkeypatch.setenv(KNOB, "0")
    _, _, lg0, loss0, g0 = run(name, "fp32s", dev)
    monkeypatch.delenv(KNOB)
    meta, _, lg1, loss1, g1 = run(name, "fp32s", dev)
    rel = lambda x, y: float(np.abs(np.asarray(x, np.float64) - y).max() / (np.abs(y).max() + 1e-30))
    report = {"logits": rel(lg1, lg0), "loss": abs(loss1 - loss0) / abs(loss0)}
    report.update({k: rel(g1[k], g0[k]) for k in meta["trainable"]})
    print("prompted vit split attn", name, report)
    assert all(np.isfinite(v).all() for v in g1.values())
    for k, v in report.items():
        assert v <= TOL[torch.float32], (k, v)
