"""Shared by test_srchead_cpu.py and test_srchead_gpu.py: the seeded inputs of a shape and the fp64
reference of the PromptSRC head (oracle.promptsrc_loss with the fp64 normalisations in front)."""
import math

import torch
import torch.nn.functional as F

from oracle import clip_oracle as O

W_TEXT, W_IMAGE, W_LOGITS = 25.0, 10.0, 1.0  # the config defaults


def inputs(B, C, E):
    """(img, txt, zs, fixed_n, fixed_q, y, alpha), all on the CPU, fp32 / int64."""
    g = torch.Generator().manual_seed(1000003 * B + 1009 * C + E)

    def r(*shape):
        return torch.randn(*shape, dtype=torch.float64, generator=g)

    fixed_n = F.normalize(r(C, E), dim=-1).float()
    txt = (3 * (fixed_n.double() + 0.5 * r(C, E) / math.sqrt(E))).float()
    zs = (2 * r(B, E)).float()
    img = (2.5 * (F.normalize(zs.double(), dim=-1) + 0.5 * r(B, E) / math.sqrt(E))).float()
    y = torch.randint(0, C, (B,), generator=g)
    alpha = (0.25 + 4 * torch.rand(C, dtype=torch.float64, generator=g)).float()
    fixed_q = fixed_n.half().float()
    return img, txt, zs, fixed_n, fixed_q, y, alpha


def reference(img, txt, zs, fixed_n, fixed_q, y, scale, alpha=None, focal=False, grad=True):
    """fp64 on the CPU: (parts [5] = total, ce, kl, l1_text, l1_image; d_img; d_txt; logits)."""
    i64 = img.double().requires_grad_(grad)
    t64 = txt.double().requires_grad_(grad)
    u, t, z = F.normalize(i64, dim=-1), F.normalize(t64, dim=-1), F.normalize(zs.double(), dim=-1)
    fn, fq = fixed_n.double(), fixed_q.double()
    s = scale * u @ t.t()
    q = scale * z @ fq.t()
    total = O.promptsrc_loss(s, y, t, fn, u, z, q, W_TEXT, W_IMAGE, W_LOGITS)
    ce = F.cross_entropy(s, y)
    if focal:
        fl = O.focal_loss(s, y, alpha, 2.0)
        total = total - ce + fl
        ce = fl
    kl = F.kl_div(F.log_softmax(s, dim=1), F.log_softmax(q, dim=1), reduction="sum",
                  log_target=True) / s.numel() * W_LOGITS
    lt = F.l1_loss(t, fn) * W_TEXT
    li = F.l1_loss(u, z) * W_IMAGE
    parts = torch.stack([total, ce, kl, lt, li]).detach()
    if not grad:
        return parts, None, None, s.detach()
    total.backward()
    return parts, i64.grad, t64.grad, s.detach()
