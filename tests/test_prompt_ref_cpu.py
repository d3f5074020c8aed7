"""CPU: the fp64 restatements of tests/prompt_ref.py against torch fp64 autograd of the naive
formulas, on inputs where the naive formula is well conditioned (logit margins <= 10): agreement to
1e-12 relative. And the saturated / -inf rows of the GPU tests give finite fp64 references."""
import pytest
import torch
import torch.nn.functional as F

import prompt_ref as PR

RTOL = 1e-12


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("B,L,D,n_vpt", [(1, 2, 4, 0), (3, 5, 36, 0), (2, 3, 260, 3)])
def test_vit_embed_ln(B, L, D, n_vpt):
    g = _g(0)
    patch, cls, pos = torch.randn(B, L - 1, D, generator=g), torch.randn(D, generator=g), torch.randn(L, D, generator=g)
    vpt = torch.randn(n_vpt, D, generator=g) if n_vpt else None
    gam, bet = torch.randn(D, generator=g), torch.randn(D, generator=g)
    x, S = PR.vit_embed_ln(patch, cls, pos, vpt, gam, bet)
    v = torch.cat([cls.double().expand(B, 1, D), patch.double()], 1) + pos.double()
    if n_vpt:
        v = torch.cat([v, vpt.double().expand(B, -1, -1)], 1)  # no positional term
    ref = F.layer_norm(v, (D,), gam.double(), bet.double(), 1e-5)
    assert x.shape == (B, L + n_vpt, D) and _rel(x, ref) <= RTOL
    assert bool((S >= 0).all()) and bool(torch.isfinite(S).all())


@pytest.mark.parametrize("position", ["end", "middle", "front"])
@pytest.mark.parametrize("mode", ["shared", "csc", "per_image"])
def test_prompt_assemble_and_ctx_grad(position, mode):
    """The assembly against its own definition through autograd: d (x0 . dx0) / d ctx is ctx_grad."""
    from fsp_amd.trainers._fns import prompt_layout
    C, n_ctx, W, B = 3, 4, 8, 2
    name_lens = [1, 3, 2]
    eot = [1 + n_ctx + nl + 1 for nl in name_lens]
    src, cpos, L = prompt_layout(C, n_ctx, name_lens, position, eot)
    g = _g(1)
    emb, pos = torch.randn(C, 77, W, generator=g).double(), torch.randn(77, W, generator=g).double()
    bias = torch.randn(B, W, generator=g).double()
    csc = mode == "csc"
    shape = {"shared": (n_ctx, W), "csc": (C, n_ctx, W), "per_image": (B, n_ctx, W)}[mode]
    sb, sc = {"shared": (0, 0), "csc": (0, n_ctx * W), "per_image": (n_ctx * W, 0)}[mode]
    ctx = torch.randn(*shape, generator=g).double().requires_grad_(True)
    x0 = PR.prompt_assemble(B, torch.from_numpy(src), emb, ctx, sb, sc, bias, pos)
    assert x0.shape == (B, C, L, W)
    for b in range(B):
        for c in range(C):
            for t in range(L):
                m = int(src[c, t])
                cv = ctx[c] if mode == "csc" else ctx[b] if mode == "per_image" else ctx
                want = emb[c, m] + pos[t] if m >= 0 else cv[-1 - m] + pos[t] + bias[b]
                assert _rel(x0[b, c, t].detach(), want.detach()) <= RTOL
    dx0 = torch.randn(B, C, L, W, generator=g).double()
    (x0 * dx0).sum().backward()
    d, S = PR.ctx_grad(dx0, torch.from_numpy(cpos), csc)
    if mode == "shared":
        assert _rel(d.view(B, n_ctx, W).sum(0), ctx.grad) <= RTOL
    elif mode == "csc":
        assert _rel(d.view(B, C, n_ctx, W).sum(0), ctx.grad) <= RTOL
    else:
        assert _rel(d.view(B, n_ctx, W), ctx.grad) <= RTOL
    assert bool((S >= d.abs()).all())


@pytest.mark.parametrize("per_image", [0, 1])
def test_cosine_logits(per_image):
    g = _g(2)
    B, C, E, scale = 3, 5, 12, 100.0
    imf = torch.randn(B, E, generator=g)
    txt = torch.randn(B * C if per_image else C, E, generator=g)
    logits, it, iv, S = PR.cosine_logits(imf, txt, scale, per_image, C)
    t = txt.double().requires_grad_(True)
    tn = t / t.norm(dim=-1, keepdim=True)
    an = imf.double() / imf.double().norm(dim=-1, keepdim=True)
    ref = scale * (torch.einsum("be,bce->bc", an, tn.view(B, C, E)) if per_image else an @ tn.t())
    assert _rel(logits, ref.detach()) <= RTOL
    assert _rel(it, 1 / t.detach().norm(dim=-1)) <= RTOL and _rel(iv, 1 / imf.double().norm(dim=-1)) <= RTOL
    assert bool((S >= logits.abs() * (1 - 1e-12)).all())
    dl = torch.randn(B, C, generator=g)
    ref.backward(dl.double())
    # inv_t / inv_i "as given": the fp64 values here, so that the comparison is of the formula
    dtxt, S2 = PR.cosine_logits_bwd(imf, txt, it, iv, dl, scale, per_image)
    assert _rel(dtxt, t.grad) <= RTOL
    assert bool((S2 >= dtxt.abs() * (1 - 1e-12)).all())


def _naive64(z, y, alpha, gamma, focal, gs):
    zr = z.double().requires_grad_(True)
    ce = F.cross_entropy(zr, y, reduction="none")
    if focal:
        a = alpha.double()[y] if alpha is not None else 1.0
        loss = a * (1 - torch.exp(-ce)) ** gamma * ce
    else:
        loss = ce
    (gs * loss.sum()).backward()
    return loss.detach(), zr.grad


@pytest.mark.parametrize("C", [1, 2, 37])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 5.0])
def test_ce_focal_against_autograd(C, gamma):
    """Margins <= 10: logits uniform in [-5, 5]."""
    g = _g(3 + C)
    B = 6
    z = torch.rand(B, C, generator=g) * 10 - 5
    y = torch.randint(0, C, (B,), generator=g)
    alpha = torch.rand(C, generator=g) + 0.5
    alpha[0] = 0.0
    for focal, al in ((False, None), (True, None), (True, alpha)):
        if C == 1 and focal and gamma < 1:
            continue  # ce == 0: the naive formula is 0 * inf there (the closed form is checked below)
        loss, dl, sl, sd = PR.ce_focal(z, y, al, gamma, focal, 0.25)
        rl, rd = _naive64(z, y, al, gamma, focal, 0.25)
        assert float((loss - rl).abs().max()) <= RTOL * max(float(rl.abs().max()), 1e-300)
        assert float((dl - rd).abs().max()) <= RTOL * max(float(rd.abs().max()), 1e-300)
        assert bool((sl >= loss.abs()).all()) and bool((sd >= 0).all())
        # the fp32 restatement of the kernels' formula is the same function
        l32, d32 = PR.ce_focal_naive(z, y, al, gamma, focal, 0.25, dt=torch.float64)
        assert float((l32 - rl).abs().max()) <= 1e-9 * max(float(rl.abs().max()), 1e-300)
        assert float((d32 - rd).abs().max()) <= 1e-9 * max(float(rd.abs().max()), 1e-300)


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 130, 1000])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 5.0])
def test_ce_focal_hard_rows_finite(C, gamma):
    """Every row kind of the GPU tests: finite fp64 references and S; saturated rows at their limit
    (loss and dlogits ~ 0 for gamma > 0); the unguarded fp32 formula is NaN on them for gamma < 1."""
    z, y, kinds = PR.logit_rows(12, C, seed=C, first=0)
    assert set(kinds) == set(PR.KINDS)
    alpha = torch.rand(C, generator=_g(9)) + 0.5
    alpha[0] = 0.0
    for focal, al in ((False, None), (True, None), (True, alpha)):
        out = PR.ce_focal(z, y, al, gamma, focal, 1.0 / 12)
        for t in out:
            assert bool(torch.isfinite(t).all())
        loss, dl = out[0], out[1]
        l32, d32 = PR.ce_focal_naive(z, y, al, gamma, focal, 1.0 / 12)
        assert bool(torch.isfinite(l32).all()) and bool(torch.isfinite(d32).all())
        sat = torch.tensor([k == "saturated" for k in kinds])
        if focal and gamma > 0:
            assert float(loss[sat].abs().max()) <= 1e-12 and float(dl[sat].abs().max()) <= 1e-6
            assert bool((l32[sat] == 0).all()) and bool((d32[sat] == 0).all())
        if focal and 0 < gamma < 1:
            _, dnan = PR.ce_focal_naive(z, y, al, gamma, focal, 1.0 / 12, guard=False)
            assert bool(torch.isnan(dnan[sat]).any())


@pytest.mark.parametrize("normalize", [False, True])
def test_meta_net(normalize):
    g = _g(5)
    B, V, Hd, Wd = 3, 20, 5, 7
    x = torch.randn(B, V, generator=g)
    w1, b1 = torch.randn(Hd, V, generator=g) * 0.3, torch.randn(Hd, generator=g) * 0.3
    w2, b2 = torch.randn(Wd, Hd, generator=g) * 0.3, torch.randn(Wd, generator=g) * 0.3
    xn, h, y, s_h, s_y, s_yh = PR.meta_net(x, w1, b1, w2, b2, normalize)
    p = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    xr = x.double()
    if normalize:
        xr = xr / xr.norm(dim=-1, keepdim=True)
    ref = torch.relu(xr @ p[0].t() + p[1]) @ p[2].t() + p[3]
    assert _rel(y, ref.detach()) <= RTOL and _rel(xn, xr) <= RTOL
    dy = torch.randn(B, Wd, generator=g)
    ref.backward(dy.double())
    out = PR.meta_net_bwd(xn, h, w2, dy)
    for name, r in (("dw1", p[0].grad), ("db1", p[1].grad), ("dw2", p[2].grad), ("db2", p[3].grad)):
        assert _rel(out[name][0], r) <= RTOL, name
        assert bool((out[name][1] >= out[name][0].abs() * (1 - 1e-12)).all()), name
