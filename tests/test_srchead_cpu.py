"""CPU: the host side of the PromptSRC head (clipk_src_head) -- the C-ABI registration, the config
default, the closed-form gradient the kernels implement (pinned against autograd through the oracle
in fp64) and ops.src_head's refusal of CPU tensors.

clipk_src_head takes 23 arguments as include/clipk.h declares it (3 sizes, 5 feature arrays, labels,
alpha, gamma, focal, scale, 3 weights, grad_scale, loss, logits, 2 gradients, ws, stream)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from fsp_amd import _native
from srchead_util import inputs, reference, W_TEXT, W_IMAGE, W_LOGITS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_src_head_symbols_are_registered():
    hdr = open(os.path.join(ROOT, "include", "clipk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("clipk_src_head", 23), ("clipk_src_head_ws_bytes", 3)):
        assert name in _native.SIGNATURES
        assert len(_native.SIGNATURES[name][1]) == nargs
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs  # the header's own count
        assert hasattr(_native.load(), name)
    assert "csrc/srchead.hip" in [rel for rel, _ in _native.source_files()]


def test_fused_src_defaults_off():
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    assert cfg.NATIVE.FUSED_SRC is False
    assert cfg.TRAINER.PROMPTSRC.LOSS_TYPE == "ce"


def closed_form(img, txt, zs, fixed_n, fixed_q, y, scale, alpha=None, focal=False, gamma=2.0):
    """The gradient clipk_src_head documents (include/clipk.h), restated in fp64 torch without
    autograd: (d_img, d_txt) of the total loss with respect to the raw img / txt."""
    img, txt, zs, fn, fq = (a.double() for a in (img, txt, zs, fixed_n, fixed_q))
    B, E = img.shape
    C = txt.shape[0]
    ni = img.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    nt = txt.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u, t, z = img / ni, txt / nt, F.normalize(zs, dim=-1)
    s = scale * u @ t.t()
    q = scale * z @ fq.t()
    ps, pq = torch.softmax(s, dim=1), torch.softmax(q, dim=1)
    onehot = F.one_hot(y, C).double()
    wgt = torch.ones(B, dtype=torch.float64)
    if focal:
        ce = -torch.log_softmax(s, dim=1)[torch.arange(B), y]
        p = torch.exp(-ce)
        a = alpha.double()[y] if alpha is not None else 1.0
        wgt = a * ((1 - p) ** gamma + gamma * p * (1 - p) ** (gamma - 1) * ce)
    G = wgt[:, None] / B * (ps - onehot) + W_LOGITS / (B * C) * (ps - pq)
    g_u = scale * G @ t + W_IMAGE / (B * E) * torch.sign(u - z)
    g_t = scale * G.t() @ u + W_TEXT / (C * E) * torch.sign(t - fn)
    d_img = (g_u - (g_u * u).sum(-1, keepdim=True) * u) / ni
    d_txt = (g_t - (g_t * t).sum(-1, keepdim=True) * t) / nt
    return d_img, d_txt


@pytest.mark.parametrize("focal", [False, True])
@pytest.mark.parametrize("scale", [14.285714, 100.0])
def test_closed_form_gradient_equals_autograd_through_the_oracle(scale, focal):
    img, txt, zs, fixed_n, fixed_q, y, alpha = inputs(3, 7, 64)
    a = alpha if focal else None
    _, d_img64, d_txt64, _ = reference(img, txt, zs, fixed_n, fixed_q, y, scale, a, focal)
    d_img, d_txt = closed_form(img, txt, zs, fixed_n, fixed_q, y, scale, a, focal)
    e_img = float((d_img - d_img64).abs().max())
    e_txt = float((d_txt - d_txt64).abs().max())
    print(f"closed form (3, 7, 64) scale {scale} focal {focal}: |d_img| max {float(d_img64.abs().max()):.3e} "
          f"err {e_img:.3e}  |d_txt| max {float(d_txt64.abs().max()):.3e} err {e_txt:.3e}")
    assert float(d_img64.abs().max()) > 1e-3 and float(d_txt64.abs().max()) > 1e-3
    assert e_img <= 1e-12 and e_txt <= 1e-12


def test_src_head_refuses_cpu_tensors():
    from fsp_amd import ops
    img, txt, zs, fixed_n, fixed_q, y, alpha = inputs(2, 3, 37)
    with pytest.raises(_native.ClipkError):
        ops.src_head(img, txt, zs, fixed_n, fixed_q, y, None, 0.0, False, 100.0, W_TEXT, W_IMAGE, W_LOGITS)


def test_src_head_fused_ok_refuses_what_the_kernel_does_not_take():
    from fsp_amd.trainers._fns import src_head_fused_ok
    img, txt, zs, fixed_n, fixed_q, _, _ = inputs(2, 3, 37)
    assert not src_head_fused_ok(img, txt, zs, fixed_n, fixed_q)  # CPU tensors
