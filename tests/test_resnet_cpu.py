"""CPU: the ModifiedResNet (RN50 / RN101) model layer -- the shape inferred from a state dict, the
synthetic state dicts' keys and shapes, the plain-torch restatement the GPU tests use as their
reference (tests/resnet_util.py) against itself and against torch's own multi-head attention, the
C ABI's new symbols, and the refusal of the trainers that need a ViT."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_util as R
from fsp_amd.clip import synth
from fsp_amd.clip.model import VIT_ONLY_TRAINERS, arch_from_state_dict, require_vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# blocks, w, embed_dim, text W, text heads, text layers, resolution
TABLE = {
    "RN50": ((3, 4, 6, 3), 64, 1024, 512, 8, 12, 224),
    "RN101": ((3, 4, 23, 3), 64, 512, 512, 8, 12, 224),
    "RN-tiny": ((1, 1, 1, 1), 64, 128, 128, 2, 2, 64),
    "RN-tiny-96": ((2, 1, 1, 1), 64, 128, 128, 2, 2, 96),
}


def _shapes(arch):
    """{key: shape} without drawing the values (the specs make_state_dict draws from)."""
    a = synth.ARCHS[arch]
    out = {k: tuple(shape) for k, shape, _, _ in synth._param_specs(a)}
    out["logit_scale"] = ()
    return out


def _expected_visual(blocks, w, embed, res):
    bn = lambda key, c: {f"{key}.{n}": ((c,) if n != "num_batches_tracked" else ())
                         for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    exp = {}
    for i, (co, ci) in enumerate(((w // 2, 3), (w // 2, w // 2), (w, w // 2)), 1):
        exp[f"visual.conv{i}.weight"] = (co, ci, 3, 3)
        exp.update(bn(f"visual.bn{i}", co))
    inpl = w
    for l, n in enumerate(blocks):
        planes = w * 2 ** l
        for i in range(n):
            p = f"visual.layer{l + 1}.{i}."
            exp[p + "conv1.weight"] = (planes, inpl, 1, 1)
            exp.update(bn(p + "bn1", planes))
            exp[p + "conv2.weight"] = (planes, planes, 3, 3)
            exp.update(bn(p + "bn2", planes))
            exp[p + "conv3.weight"] = (4 * planes, planes, 1, 1)
            exp.update(bn(p + "bn3", 4 * planes))
            if i == 0:
                exp[p + "downsample.0.weight"] = (4 * planes, inpl, 1, 1)
                exp.update(bn(p + "downsample.1", 4 * planes))
            inpl = 4 * planes
    C, S = 32 * w, res // 32
    exp["visual.attnpool.positional_embedding"] = (S * S + 1, C)
    for n, o in (("q_proj", C), ("k_proj", C), ("v_proj", C), ("c_proj", embed)):
        exp[f"visual.attnpool.{n}.weight"] = (o, C)
        exp[f"visual.attnpool.{n}.bias"] = (o,)
    return exp


@pytest.mark.parametrize("arch", sorted(TABLE))
def test_arch_from_state_dict_resnet(arch):
    blocks, w, embed, tw, th, tl, res = TABLE[arch]
    sd = {k: torch.empty(s, device="meta") for k, s in _shapes(arch).items()}
    a = arch_from_state_dict(sd)
    assert a == synth.ARCHS[arch]
    assert a.vision_layers == blocks and isinstance(a.vision_layers, tuple)
    assert (a.vision_width, a.embed_dim, a.image_resolution) == (w, embed, res)
    assert (a.transformer_width, a.transformer_heads, a.transformer_layers) == (tw, th, tl)
    assert a.vision_patch_size is None and a.is_resnet and a.vision_heads == 32 * w // 64
    assert (a.context_length, a.vocab_size) == (77, 49408)


@pytest.mark.parametrize("arch", sorted(TABLE))
def test_synthetic_keys_and_shapes(arch):
    blocks, w, embed, _, _, _, res = TABLE[arch]
    got = {k: s for k, s in _shapes(arch).items() if k.startswith("visual.")}
    assert got == _expected_visual(blocks, w, embed, res)


def test_synthetic_values():
    sd = synth.make_state_dict("RN-tiny", seed=0)
    assert {k: tuple(np.shape(v)) for k, v in sd.items()} == _shapes("RN-tiny")
    for k, v in sd.items():
        if k.endswith("running_var"):
            assert v.dtype == np.float32 and 0.5 <= v.min() and v.max() < 1.5
        if re.search(r"bn\d\.weight$|downsample\.1\.weight$", k):
            assert abs(v.mean() - 1.0) < 0.05
        if k.endswith("num_batches_tracked"):
            assert v.dtype == np.int64 and v.shape == ()
    h = synth.make_state_dict("RN-tiny", seed=0, fp16_values=True)
    for k, v in h.items():
        if v.dtype == np.float32 and k != "logit_scale":
            assert np.array_equal(v, v.astype(np.float16).astype(np.float32)), k
    assert synth.state_dict_digest(sd) == synth.state_dict_digest(synth.make_state_dict("RN-tiny", seed=0))


def test_vit_arch_unchanged():
    for name in ("tiny", "tiny-p8", "tiny4"):
        a = arch_from_state_dict(synth.make_state_dict(name, seed=0))
        assert a == synth.ARCHS[name] and not a.is_resnet and isinstance(a.vision_layers, int)
    assert synth.ARCHS["ViT-B/16"] == synth.ClipArch(512, 224, 12, 768, 16, 77, 49408, 512, 8, 12)
    assert synth.ARCHS["ViT-B/16"].vision_heads == 12
    with pytest.raises(KeyError):
        arch_from_state_dict({"visual.conv1.weight": torch.zeros(4, 3, 3, 3)})


def test_restatement_fp32_against_fp64():
    _, _, f64, f32 = R.reference("RN-tiny", 2)
    assert f64.dtype == torch.float64 and f32.dtype == torch.float32 and f64.shape == (2, 128)
    assert bool(torch.isfinite(f64).all())
    scale = float(f64.abs().max())
    err = float((f32.double() - f64).abs().max())
    print(f"RN-tiny restatement: max |feat| {scale:.3e}, fp32 vs fp64 {err:.3e}")
    # 18 layers of fp32 sums over K <= 2048: 2^-24 sqrt(K) per layer is ~ 3e-6 relative; 1e-4 leaves room
    assert 0.05 < scale < 50.0
    assert err <= 1e-4 * scale


def test_restatement_attnpool_is_multi_head_attention():
    g = torch.Generator().manual_seed(5)
    B, HW, C, E, heads = 2, 9, 128, 64, 2
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    p = {"visual.attnpool.positional_embedding": r(HW + 1, C) * C ** -0.5}
    for n, o in (("q_proj", C), ("k_proj", C), ("v_proj", C), ("c_proj", E)):
        p[f"visual.attnpool.{n}.weight"] = r(o, C) * C ** -0.5
        p[f"visual.attnpool.{n}.bias"] = r(o) * 0.1
    x = r(B, HW, C)
    got = R.attnpool(p, x, heads)
    # model.py:70-90
    t = x.permute(1, 0, 2)
    t = torch.cat([t.mean(0, keepdim=True), t], 0) + p["visual.attnpool.positional_embedding"][:, None, :]
    g_ = lambda n: p["visual.attnpool." + n]
    want, _ = F.multi_head_attention_forward(
        query=t[:1], key=t, value=t, embed_dim_to_check=C, num_heads=heads, q_proj_weight=g_("q_proj.weight"),
        k_proj_weight=g_("k_proj.weight"), v_proj_weight=g_("v_proj.weight"), in_proj_weight=None,
        in_proj_bias=torch.cat([g_("q_proj.bias"), g_("k_proj.bias"), g_("v_proj.bias")]), bias_k=None, bias_v=None,
        add_zero_attn=False, dropout_p=0.0, out_proj_weight=g_("c_proj.weight"), out_proj_bias=g_("c_proj.bias"),
        use_separate_proj_weight=True, training=False, need_weights=False)
    assert float((got - want.squeeze(0)).abs().max()) <= 1e-12 * float(want.abs().max())


NEW_SYMBOLS = ["clipk_conv2d_nhwc", "clipk_im2col_3x3s2", "clipk_avgpool2_nhwc", "clipk_attnpool_ws_bytes",
               "clipk_attnpool", "clipk_resnet_create", "clipk_resnet_destroy", "clipk_resnet_ws_bytes",
               "clipk_resnet_forward"]


def test_new_symbols_declared():
    from fsp_amd import _native as N
    with open(os.path.join(ROOT, "include", "clipk.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in N.SIGNATURES, name
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m, name
        args = m.group(1).strip()
        n_args = 0 if args in ("", "void") else args.count(",") + 1
        assert n_args == len(N.SIGNATURES[name][1]), name
    for flag, val in (("CLIPK_CONV_RES", N.CONV_RES), ("CLIPK_CONV_RELU", N.CONV_RELU),
                      ("CLIPK_CONV_OUT_F32", N.CONV_OUT_F32)):
        assert re.search(flag + r" = " + str(val) + r"\b", header), flag
    from fsp_amd import ops
    for fn in ("conv2d_nhwc", "avgpool2_nhwc", "attnpool", "im2col_3x3s2"):
        assert callable(getattr(ops, fn))


def test_resnet_refusal_helper():
    assert set(VIT_ONLY_TRAINERS) == {"IVLP", "MaPLe", "PromptSRC", "LoRA"}
    for trainer in VIT_ONLY_TRAINERS:
        for name in ("RN50", "RN101"):
            with pytest.raises(ValueError, match=name):
                require_vit(trainer, name, synth.ARCHS[name])
        require_vit(trainer, "ViT-B/16", synth.ARCHS["ViT-B/16"])  # a ViT passes
