"""Helpers shared by the LoRA tests: the torch reference (oracle/clip_oracle.py is functional over a
parameter dict, so LoRA is the unchanged oracle on p' with in_proj_weight = W0 + s B A built from
autograd leaves A, B), the hand-written adapter gradients, and seeded inputs."""
import torch

STEMS = {"text": "transformer.resblocks.", "visual": "visual.transformer.resblocks."}


def merged_weight(w0, A, B, scale, proj_mask):
    """W' [3W, W] = W0 + scale * B_p A_p on the projections of proj_mask (A [3, r, W], B [3, W, r])."""
    W = w0.shape[1]
    parts = []
    for p in range(3):
        blk = w0[p * W:(p + 1) * W]
        parts.append(blk + scale * (B[p] @ A[p]) if (proj_mask >> p) & 1 else blk)
    return torch.cat(parts, 0)


def lora_params(p, adapters, scale, proj_mask, layer_masks):
    """p' for the oracle: adapters = {"text": (A, B), "visual": (A, B)} (A [layers, 3, r, W], B
    [layers, 3, W, r]; a missing side stays frozen), layer_masks = {"text": m, "visual": m}."""
    q = dict(p)
    for side, (A, B) in adapters.items():
        for l in range(A.shape[0]):
            if (layer_masks[side] >> l) & 1:
                k = f"{STEMS[side]}{l}.attn.in_proj_weight"
                q[k] = merged_weight(p[k], A[l], B[l], scale, proj_mask)
    return q


def wgrad_reference(X, mean, rstd, gamma, beta, dY, A, B, scale, proj_mask):
    """The adapter gradients of one layer by hand (the dtype of the inputs; include/clipk.h):
    xn = (X - mean) rstd gamma + beta, P_p = xn A_p^T, dU_p = s dY_p B_p, dB_p = s dY_p^T P_p,
    dA_p = dU_p^T xn; zeros for the projections outside proj_mask."""
    W = X.shape[1]
    xn = (X - mean[:, None]) * rstd[:, None] * gamma + beta
    dA, dB = torch.zeros_like(A), torch.zeros_like(B)
    for p in range(3):
        if not (proj_mask >> p) & 1:
            continue
        dYp = dY[:, p * W:(p + 1) * W]
        P = xn @ A[p].t()
        dU = scale * (dYp @ B[p])
        dB[p] = scale * (dYp.t() @ P)
        dA[p] = dU.t() @ xn
    return dA, dB


def wgrad_inputs(rows, W, r, seed):
    """fp32 CPU inputs of clipk_lora_wgrad: X, its LayerNorm statistics, gamma, beta, dY, A, B."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(rows, W, generator=g) * 1.5 + 0.3
    gamma = 1.0 + 0.2 * torch.randn(W, generator=g)
    beta = 0.1 * torch.randn(W, generator=g)
    dY = torch.randn(rows, 3 * W, generator=g) * 1e-2
    A = (torch.rand(3, r, W, generator=g) * 2 - 1) / W ** 0.5
    B = torch.randn(3, W, r, generator=g) * 0.05
    return X, gamma, beta, dY, A, B


def ln_stats(X):
    """(mean, rstd) of the rows of X (eps 1e-5) in fp32, from fp64."""
    x = X.double()
    mu = x.mean(-1)
    var = ((x - mu[:, None]) ** 2).mean(-1)
    return mu.float(), (1.0 / torch.sqrt(var + 1e-5)).float()


def tiny_adapters(arch, rank, seed, b_std=0.05):
    """Seeded non-trivial adapters (B != 0, so both gradients are exercised) for both encoders, fp32
    CPU: {"text": (A, B), "visual": (A, B)}."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for side, nl, W in (("text", arch.transformer_layers, arch.transformer_width),
                        ("visual", arch.vision_layers, arch.vision_width)):
        A = (torch.rand(nl, 3, rank, W, generator=g) * 2 - 1) / W ** 0.5
        B = torch.randn(nl, 3, W, rank, generator=g) * b_std
        out[side] = (A, B)
    return out
