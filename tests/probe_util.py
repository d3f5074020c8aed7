"""Shared by test_probe_cpu.py and test_probe_head_gpu.py: the seeded inputs of a shape and the
fp64 reference of the linear-probe head (F.normalize, F.linear, F.cross_entropy or
oracle.focal_loss, autograd)."""
import torch
import torch.nn.functional as F

from oracle import clip_oracle as O

# (normalize, scale): CLIP's two usual logit scales on normalised features, and a plain Linear
MODES = [(True, 14.285714), (True, 100.0), (False, 1.0)]


def inputs(B, C, E):
    """(feat, w, bias, y, alpha), all on the CPU, fp32 / int64."""
    g = torch.Generator().manual_seed(1000003 * B + 1009 * C + E)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)  # noqa: E731
    feat = (2 * r(B, E)).float()
    w = (F.normalize(r(C, E), dim=-1) * (1 + 0.1 * r(C, 1))).float()
    bias = (0.5 * r(C)).float()
    y = torch.randint(0, C, (B,), generator=g)
    alpha = (0.25 + 4 * torch.rand(C, dtype=torch.float64, generator=g)).float()
    return feat, w, bias, y, alpha


def reference(feat, w, bias, y, normalize, scale, alpha=None, focal=False, grad=True):
    """fp64 on the CPU: (loss, d_w, d_bias, logits); d_bias None without a bias, both None when not
    grad."""
    f64 = feat.double()
    w64 = w.double().requires_grad_(grad)
    b64 = bias.double().requires_grad_(grad) if bias is not None else None
    u = F.normalize(f64, dim=-1) if normalize else f64
    s = scale * F.linear(u, w64)
    if b64 is not None:
        s = s + b64
    loss = O.focal_loss(s, y, alpha, 2.0) if focal else F.cross_entropy(s, y)
    if not grad:
        return loss.detach(), None, None, s.detach()
    loss.backward()
    return loss.detach(), w64.grad, (b64.grad if b64 is not None else None), s.detach()
