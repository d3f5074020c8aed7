"""Plain torch restatements of the csrc/prompt.hip kernels (patch / ViT embedding with ln_pre, prompt
assembly and its context gradient, cosine logits, CE / focal loss, Meta-Net), evaluated in fp64 on the
fp32 inputs as given. A helper module for test_prompt_ref_cpu.py and test_prompt_kernels_gpu.py.

Every function that sums also returns S, the fp64 magnitude its rounding error scales with (the sum
of the absolute values of its terms, carried to the output through the first-order error
propagation of the formula), so that a test can gate element i at A 2^-24 S_i + 2^-24 |ref_i|.
``dt=torch.float32`` runs the same formula in fp32 (the restatement whose own error against fp64
calibrates A where a path goes through exp / log / rsqrt / pow).
"""
import torch

U = 2.0 ** -24  # one fp32 rounding, relative


# ---------------------------------------------------------------- ViT embedding + ln_pre
def vit_embed_ln(patch, cls, pos, vpt, gamma, beta, dt=torch.float64):
    """patch [B, L-1, D], cls [D], pos [L, D], vpt [n_vpt, D] or None -> (x [B, L + n_vpt, D], S).
    x = LayerNorm(cat(cls, patch) + pos, then the vpt rows without pos), eps 1e-5.
    S = |gamma| rstd (|v| + mean|v|) + |beta|: the error of v - mean, scaled like the output."""
    B, D = patch.shape[0], patch.shape[-1]
    v = torch.cat([cls.to(dt).expand(B, 1, D), patch.to(dt)], 1) + pos.to(dt)
    if vpt is not None and vpt.shape[0]:
        v = torch.cat([v, vpt.to(dt).expand(B, -1, -1)], 1)
    mu = v.mean(-1, keepdim=True)
    d = v - mu
    rs = (d * d).mean(-1, keepdim=True).add(1e-5).rsqrt()
    x = d * rs * gamma.to(dt) + beta.to(dt)
    S = gamma.to(dt).abs() * rs * (v.abs() + v.abs().mean(-1, keepdim=True)) + beta.to(dt).abs()
    return x, S


# ---------------------------------------------------------------- prompt assembly / context gradient
def prompt_assemble(B, src_map, emb, ctx, sb, sc, bias, pos, dt=torch.float64):
    """src_map [C, L] (>= 0: row of the class's token embedding, < 0: context slot -1 - m),
    emb [C, 77, W], ctx a flat buffer read at b * sb + c * sc + slot * W, bias [B, W] or None,
    pos [>= L, W] -> x0 [B, C, L, W] = (row + pos) + bias, in that order (bias on context slots
    only). With dt = fp32 the sums round as the kernel's do."""
    C, L = src_map.shape
    W = emb.shape[-1]
    flat = ctx.reshape(-1).to(dt)
    x0 = torch.empty(B, C, L, W, dtype=dt)
    for b in range(B):
        for c in range(C):
            for t in range(L):
                m = int(src_map[c, t])
                if m >= 0:
                    x0[b, c, t] = emb[c, m].to(dt) + pos[t].to(dt)
                else:
                    o = b * sb + c * sc + (-1 - m) * W
                    r = flat[o:o + W] + pos[t].to(dt)
                    x0[b, c, t] = r + bias[b].to(dt) if bias is not None else r
    return x0


def ctx_grad(dx0, ctx_pos, csc, dt=torch.float64):
    """dx0 [B, C, L, W], ctx_pos [C, n_ctx] -> (d [B * (C if csc else 1) * n_ctx, W], S):
    d[(b, group, k)] = sum over the group's classes of dx0[b, c, ctx_pos[c, k]]; S = sum of |.|."""
    B, C, L, W = dx0.shape
    n_ctx = ctx_pos.shape[1]
    idx = ctx_pos.long()  # [C, n_ctx]
    g = dx0.to(dt)[:, torch.arange(C)[:, None], idx]  # [B, C, n_ctx, W]
    if csc:
        return g.reshape(B * C * n_ctx, W), g.abs().reshape(B * C * n_ctx, W)
    return g.sum(1).reshape(B * n_ctx, W), g.abs().sum(1).reshape(B * n_ctx, W)


# ---------------------------------------------------------------- cosine logits
def cosine_logits(imf, txt, scale, per_image, C, dt=torch.float64):
    """imf [B, E], txt [B * C or C, E] -> (logits [B, C], inv_t [rows], inv_i [B], S_logits).
    logits = scale (imf . txt) inv_t inv_i; S = scale sum|imf txt| inv_t inv_i. inv_t / inv_i are
    one-signed sums: their S is the value itself."""
    B, E = imf.shape
    a, t = imf.to(dt), txt.to(dt)
    it = (t * t).sum(-1).rsqrt()
    iv = (a * a).sum(-1).rsqrt()
    if per_image:
        t3 = t.view(B, C, E)
        d = torch.einsum("be,bce->bc", a, t3)
        m = torch.einsum("be,bce->bc", a.abs(), t3.abs())
        itb = it.view(B, C)
    else:
        d = a @ t.t()
        m = a.abs() @ t.abs().t()
        itb = it[None, :]
    return scale * d * itb * iv[:, None], it, iv, scale * m * itb * iv[:, None]


def cosine_logits_bwd(imf, txt, inv_t, inv_i, dl, scale, per_image, dt=torch.float64):
    """dtxt[row] = inv_t (dy - y (y . dy)), y = txt inv_t, dy = scale sum_b dl[b, c] inv_i[b] imf[b]
    (the sum over the one image of the row when per_image). inv_t / inv_i as given.
    -> (dtxt, S) with S = inv_t (Sdy + |y| sum|y| Sdy), Sdy the |.| sum of dy's terms."""
    B, C = dl.shape
    E = imf.shape[1]
    a, t, g = imf.to(dt), txt.to(dt), dl.to(dt)
    it, iv = inv_t.to(dt)[:, None], inv_i.to(dt)
    w = scale * g * iv[:, None]  # [B, C]
    if per_image:
        dy = (w[:, :, None] * a[:, None, :]).reshape(B * C, E)
        sdy = dy.abs()
    else:
        dy = w.t() @ a
        sdy = w.abs().t() @ a.abs()
    y = t * it
    yd = (y * dy).sum(-1, keepdim=True)
    syd = (y.abs() * sdy).sum(-1, keepdim=True)
    return it * (dy - y * yd), it * (sdy + y.abs() * syd)


# ---------------------------------------------------------------- CE / focal loss
def _onehot(y, C):
    return torch.zeros(y.shape[0], C, dtype=torch.bool).scatter_(1, y[:, None], True)


def ce_focal(z, y, alpha=None, gamma=2.0, focal=False, grad_scale=1.0):
    """fp64 row loss and dlogits in a form that does not saturate:
        ce = log1p(sum_{c != y} exp(z_c - z_y)) through a max-shifted sum,
        p = exp(-ce), om = -expm1(-ce), softmax_c = exp(z_c - z_y - ce), softmax_y - 1 = expm1(-ce),
        wgt = a (om^g + g p om^(g-1) ce), the second term 0 where om == 0,
        loss = a om^g ce (focal) or ce, dlogits = grad_scale wgt (softmax - onehot).
    -> (loss [B], dlogits [B, C], S_loss [B], S_dl [B, C]).
    The S are first-order bounds for an fp32 evaluation of ce = (max + log sum exp(z - max)) - z_y:
        S_ce = |max| + |log sum| + |z_y| + 1   (the 1: a relative error of the sum is absolute in its log)
        S_loss = a wgt S_ce + |loss|           (d loss / d ce = a wgt)
        S_dl = grad_scale a (|d wgt / d ce| S_ce |softmax - onehot|
                             + wgt (softmax (|z_c| + |lse| + S_ce) + softmax + onehot + 2^-102))
    (2^-102 = 2^-126 / 2^-24: a softmax below the smallest normal fp32 may be flushed to 0, an absolute
    error of 2^-126 whatever its size)."""
    z = z.double()
    B, C = z.shape
    oh = _onehot(y, C)
    zy = z.gather(1, y[:, None])
    d = z - zy
    do = d.masked_fill(oh, float("-inf"))
    m = do.max(1, keepdim=True).values.clamp_min(0.0)
    t = torch.exp(do - m).sum(1, keepdim=True)
    ce = torch.where(m == 0, torch.log1p(t), m + torch.log(torch.exp(-m) + t))
    p = torch.exp(-ce)
    om = -torch.expm1(-ce)
    sm = torch.exp(d - ce)  # softmax
    diff = torch.where(oh, torch.expm1(-ce).expand(B, C), sm)  # softmax - onehot
    lse = zy + ce
    mx = z.max(1, keepdim=True).values
    s_ce = mx.abs() + (lse - mx).abs() + zy.abs() + 1.0
    if focal:
        a = alpha.double()[y][:, None] if alpha is not None else torch.ones(B, 1, dtype=torch.float64)
        g = float(gamma)
        pos = om > 0
        omp = torch.where(pos, om, torch.ones_like(om))  # (no 0^negative below)
        og = torch.pow(om, g)
        t2 = torch.where(pos, g * p * torch.pow(omp, g - 1) * ce, torch.zeros_like(ce))
        wu = og + t2
        dw = torch.where(pos, g * torch.pow(omp, g - 1) * p * (2.0 - ce)
                         + g * (g - 1) * torch.pow(omp, g - 2) * p * p * ce, torch.zeros_like(ce))
        loss = a * og * ce
    else:
        a = torch.ones(B, 1, dtype=torch.float64)
        wu = torch.ones_like(ce)
        dw = torch.zeros_like(ce)
        loss = ce
    dl = grad_scale * a * wu * diff
    s_loss = a.abs() * wu * s_ce + loss.abs()
    zabs = torch.where(sm > 0, z.abs(), torch.zeros_like(z))  # (a -inf logit: softmax 0, no term)
    s_dl = abs(grad_scale) * a.abs() * (dw.abs() * s_ce * diff.abs()
                                        + wu * (sm * (zabs + lse.abs() + s_ce) + sm + oh.double() + 2.0 ** -102))
    return loss[:, 0], dl, s_loss[:, 0], s_dl


def ce_focal_naive(z, y, alpha=None, gamma=2.0, focal=False, grad_scale=1.0, dt=torch.float32, guard=True):
    """The kernels' formula in dtype dt: lse = max + log(sum exp(z - max)), ce = lse - z_y,
    p = exp(-ce), om = 1 - p, wgt = a (om^g + g p om^(g-1) ce) with the second term 0 where g == 0
    or (guard) om == 0. -> (loss [B], dlogits [B, C])."""
    z = z.to(dt)
    B, C = z.shape
    oh = _onehot(y, C)
    mx = z.max(1, keepdim=True).values
    lse = mx + torch.log(torch.exp(z - mx).sum(1, keepdim=True))
    ce = lse - z.gather(1, y[:, None])
    loss, wgt = ce, torch.ones_like(ce)
    if focal:
        a = alpha.to(dt)[y][:, None] if alpha is not None else torch.ones(B, 1, dtype=dt)
        g = float(gamma)
        p = torch.exp(-ce)
        om = 1.0 - p
        og = torch.pow(om, g)
        t2 = g * p * torch.pow(om, g - 1) * ce
        if g == 0:
            t2 = torch.zeros_like(ce)
        elif guard:
            t2 = torch.where(om != 0, t2, torch.zeros_like(ce))
        loss = a * og * ce
        wgt = a * (og + t2)
    dl = grad_scale * wgt * (torch.exp(z - lse) - oh.to(dt))
    return loss[:, 0], dl


# ---------------------------------------------------------------- Meta-Net
def meta_net(x, w1, b1, w2, b2, normalize=False, dt=torch.float64):
    """h = relu(x w1^T + b1), y = h w2^T + b2 (x / |x| first when normalize)
    -> (xn, h, y, S_h, S_y_own, S_y_from_h): the error of y is A_y u S_y_own + A_h u S_y_from_h
    (relu is 1-Lipschitz, so h's error S_h reaches y through |w2|)."""
    x, w1, b1, w2, b2 = (t.to(dt) for t in (x, w1, b1, w2, b2))
    xn = x / x.norm(dim=-1, keepdim=True) if normalize else x
    h = torch.relu(xn @ w1.t() + b1)
    s_h = xn.abs() @ w1.abs().t() + b1.abs()
    y = h @ w2.t() + b2
    return xn, h, y, s_h, h @ w2.abs().t() + b2.abs(), s_h @ w2.abs().t()


def meta_net_bwd(x, h, w2, dy, dt=torch.float64):
    """x and h as given. dh = (dy w2) [h > 0], dw2 = dy^T h, db2 = sum_b dy, dw1 = dh^T x, db1 = sum_b dh
    -> dict of (value, S); dw1 / db1 carry a second S for dh's own error reaching them."""
    x, h, w2, dy = (t.to(dt) for t in (x, h, w2, dy))
    on = (h > 0).to(dt)
    dh = (dy @ w2) * on
    s_dh = (dy.abs() @ w2.abs()) * on
    return {"dh": (dh, s_dh),
            "dw2": (dy.t() @ h, dy.abs().t() @ h.abs()),
            "db2": (dy.sum(0), dy.abs().sum(0)),
            "dw1": (dh.t() @ x, dh.abs().t() @ x.abs(), s_dh.t() @ x.abs()),
            "db1": (dh.sum(0), dh.abs().sum(0), s_dh.sum(0))}


# ---------------------------------------------------------------- loss test rows
KINDS = ("randn4", "uniform100", "equal", "saturated", "antisaturated", "neginf")


def logit_rows(B, C, seed, first=0):
    """fp32 logits [B, C], labels [B] in [0, C) and the kind of each row, cycling through KINDS from
    ``first``: randn * 4; uniform [-100, 100]; all equal; saturated (the label logit 40 above every
    other); anti-saturated (40 below the maximum); -inf at some non-label classes."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, generator=g) * 4
    y = torch.randint(0, C, (B,), generator=g)
    kinds = []
    for b in range(B):
        kind = KINDS[(first + b) % len(KINDS)]
        kinds.append(kind)
        lab = int(y[b])
        others = torch.arange(C) != lab
        if kind == "uniform100":
            z[b] = torch.rand(C, generator=g) * 200 - 100
        elif kind == "equal":
            z[b] = 1.25
        elif kind == "saturated":
            z[b, lab] = (z[b][others].max() if C > 1 else z[b, lab]) + 40
        elif kind == "antisaturated" and C > 1:
            z[b, lab] = z[b][others].max() - 40
        elif kind == "neginf" and C > 1:
            drop = others & (torch.rand(C, generator=g) < 0.5)
            z[b, drop] = float("-inf")
    return z, y, kinds
