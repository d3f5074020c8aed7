"""GPU: clipk_src_head (csrc/srchead.hip) against oracle.promptsrc_loss in fp64.

Inputs for shape (B, C, E): srchead_util.inputs (seed 1000003 B + 1009 C + E); weights 25 / 10 / 1.
Reference: srchead_util.reference, fp64 on the CPU, autograd for the gradients with respect to the
raw img / txt (oracle.focal_loss in place of the CE term for focal).

Tolerance: the rule of tests/test_ntxent_gpu.py. The flag-off fp32 torch composition (F.normalize,
the two products, CrossEntropyFn, l1_loss, log_softmax / kl_div, autograd) is measured on the
device against the same reference -- e_loss absolute (of the total), e_grad relative to max |grad64|
over both tensors -- and the kernel must stay within max(8 e_loss, 16 ulp max(1, |loss64|)) for the
total and for each of the four parts against its own fp64 part, and within max(8 e_grad, 32 ulp) for
the gradients, ulp = 2^-24.

Sign elements: the L1 terms' gradient is a sign, and an element with |t - fixed_n| or |u - z| below
fp32 resolution can take the other sign in fp32, which moves that gradient element by
2 w / (rows E). The elements with |diff| < 1e-6 (found in fp64 on the CPU, from the inputs alone)
are left out of the gradient comparison, for the kernel and the composition alike, and the other
elements of a row that holds one get 2 w / (rows E) max|n|^2 / |x| added to their bound (the flip
seen through the projection). At most 1e-3 of a tensor's elements may be masked (asserted).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from srchead_util import inputs, reference, W_TEXT, W_IMAGE, W_LOGITS

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8), (1, 2, 5), (2, 3, 37), (3, 7, 64), (4, 37, 512), (4, 100, 512), (4, 1000, 512), (5, 1030, 768),
          (32, 1000, 512), (33, 65, 130), (128, 10, 512)]
SCALES = [14.285714, 100.0]
ULP = 2.0 ** -24
NAMES = ("total", "ce", "kl", "l1_text", "l1_image")
_CASES = {}


def sign_masks(img, txt, zs, fixed_n):
    """Per tensor: (mask of the elements whose sign fp32 may flip, the extra bound of each row)."""
    u, z = F.normalize(img.double(), dim=-1), F.normalize(zs.double(), dim=-1)
    t = F.normalize(txt.double(), dim=-1)
    out = []
    for n, ref, x, w in ((u, z, img, W_IMAGE), (t, fixed_n.double(), txt, W_TEXT)):
        mask = (n - ref).abs() < 1e-6
        rows, E = n.shape
        extra = 2 * w / (rows * E) * n.abs().max(dim=-1).values ** 2 / x.double().norm(dim=-1).clamp_min(1e-12)
        extra = torch.where(mask.any(dim=-1), extra, torch.zeros_like(extra))
        out.append((mask, extra))
    return out


def grad_err(d_img, d_txt, ref, masks, scale=1.0, extra=True):
    """max over the unmasked elements of (|g - scale g64| - the row's extra bound), relative to
    scale max |grad64| over both tensors."""
    _, di64, dt64, _ = ref
    gmax = scale * max(float(di64.abs().max()), float(dt64.abs().max()))
    worst = 0.0
    for g, g64, (mask, ex) in ((d_img, di64, masks[0]), (d_txt, dt64, masks[1])):
        err = (g.double().cpu() - scale * g64).abs()
        if extra:
            err = err - scale * ex[:, None]
        err = torch.where(mask, torch.zeros_like(err), err)
        worst = max(worst, float(err.max()))
    return max(worst, 0.0) / gmax


def composition(dev, img, txt, zs, fixed_n, fixed_q, y, scale, alpha=None, focal=False, grad=True):
    """The flag-off head of PromptSRCCustomCLIP.forward / PromptSRC.forward_backward in fp32 on the
    device: (parts [5], d_img, d_txt)."""
    from fsp_amd.trainers._fns import CrossEntropyFn
    i = img.to(dev).requires_grad_(grad)
    t = txt.to(dev).requires_grad_(grad)
    fn, fq, yd = fixed_n.to(dev), fixed_q.to(dev), y.to(dev)
    u, tn = F.normalize(i, dim=-1), F.normalize(t, dim=-1)
    logits = scale * u @ tn.t()
    with torch.no_grad():
        z = F.normalize(zs.to(dev), dim=-1)
        zs_logits = scale * z @ fq.t()
    a = alpha.to(dev) if alpha is not None else None
    ce = CrossEntropyFn.apply(logits, yd, a, 2.0 if focal else 0.0, focal)
    lt = F.l1_loss(tn, fn, reduction="mean") * W_TEXT
    li = F.l1_loss(u, z, reduction="mean") * W_IMAGE
    kl = F.kl_div(F.log_softmax(logits, dim=1), F.log_softmax(zs_logits, dim=1), reduction="sum",
                  log_target=True) / logits.numel() * W_LOGITS
    total = ce + (kl + lt + li)
    parts = torch.stack([total, ce, kl, lt, li]).detach()
    if not grad:
        return parts, None, None
    total.backward()
    return parts, i.grad, t.grad


def case(dev, B, C, E, scale, focal=False):
    """Inputs, masks, fp64 reference and the composition's errors of a case, computed once."""
    key = (B, C, E, scale, focal)
    if key not in _CASES:
        x = inputs(B, C, E)
        img, txt, zs, fixed_n, fixed_q, y, alpha = x
        a = alpha if focal else None
        masks = sign_masks(img, txt, zs, fixed_n)
        ref = reference(img, txt, zs, fixed_n, fixed_q, y, scale, a, focal)
        parts, di, dt = composition(dev, img, txt, zs, fixed_n, fixed_q, y, scale, a, focal)
        e_parts = (parts.double().cpu() - ref[0]).abs()
        e_grad = grad_err(di, dt, ref, masks, extra=False)
        _CASES[key] = (x, masks, ref, (float(e_parts[0]), e_grad, e_parts))
    return _CASES[key]


def loss_bound(e_loss, loss64):
    return max(8 * e_loss, 16 * ULP * max(1.0, abs(float(loss64))))


def grad_bound(e_grad):
    return max(8 * e_grad, 32 * ULP)


def head(dev, x, scale, focal=False, **kw):
    from fsp_amd import ops
    img, txt, zs, fixed_n, fixed_q, y, alpha = (t.to(dev) for t in x)
    return ops.src_head(img, txt, zs, fixed_n, fixed_q, y, alpha if focal else None, 2.0 if focal else 0.0, focal,
                        scale, W_TEXT, W_IMAGE, W_LOGITS, **kw)


def check(dev, B, C, E, scale, focal=False, grad_scale=1.0):
    x, masks, ref, (e_loss, e_grad, e_parts) = case(dev, B, C, E, scale, focal)
    for (mask, _), what in zip(masks, ("img", "txt")):
        share = float(mask.double().mean())
        assert share <= 1e-3, (what, share)
    if C > 1:
        assert float(ref[0][1]) >= 0.05  # not at a saturated loss
    loss, logits, d_img, d_txt = head(dev, x, scale, focal, grad_scale=grad_scale)
    assert loss.shape == (5,) and logits is None and d_img.shape == (B, E) and d_txt.shape == (C, E)
    k_parts = (loss.double().cpu() - ref[0]).abs()
    k_grad = grad_err(d_img, d_txt, ref, masks, scale=grad_scale)
    tag = f"src_head ({B}, {C}, {E}) scale {scale:g}{' focal' if focal else ''}"
    print(f"{tag}: loss64 {float(ref[0][0]):.6f}  loss err torch {e_loss:.3e} kernel {float(k_parts[0]):.3e} "
          f"(bound {loss_bound(e_loss, ref[0][0]):.3e})  grad err torch {e_grad:.3e} kernel {k_grad:.3e} "
          f"(bound {grad_bound(e_grad):.3e})  masked {int(masks[0][0].sum())}/{int(masks[1][0].sum())}")
    print("    parts (ce, kl, l1_text, l1_image) err torch " + " ".join(f"{float(v):.2e}" for v in e_parts[1:])
          + "  kernel " + " ".join(f"{float(v):.2e}" for v in k_parts[1:]))
    for k, name in enumerate(NAMES):
        assert float(k_parts[k]) <= loss_bound(e_loss, ref[0][k]), name
    assert k_grad <= grad_bound(e_grad)
    return loss


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,C,E", SHAPES)
def test_src_head_matches_fp64_reference(dev, B, C, E, scale):
    loss = check(dev, B, C, E, scale)
    if C == 1:  # one class: log-softmax of a single logit
        assert float(loss[1]) == 0.0 and float(loss[2]) == 0.0


@pytest.mark.parametrize("B,C,E", [(4, 100, 512), (2, 3, 37)])
def test_src_head_focal_with_alpha(dev, B, C, E):
    check(dev, B, C, E, 100.0, focal=True)


def test_src_head_one_class_gradient_is_the_l1_terms_alone(dev):
    x, _, _, _ = case(dev, 1, 1, 8, 100.0)
    loss, _, d_img, d_txt = head(dev, x, 100.0)
    assert float(loss[1]) == 0.0 and float(loss[2]) == 0.0
    img, txt, zs, fixed_n = (t.double() for t in x[:4])

    def l1_only(a, ref, w):
        n = F.normalize(a, dim=-1)
        g = w / a.numel() * torch.sign(n - ref)
        return (g - (g * n).sum(-1, keepdim=True) * n) / a.norm(dim=-1, keepdim=True)

    want_i = l1_only(img, F.normalize(zs, dim=-1), W_IMAGE)
    want_t = l1_only(txt, fixed_n, W_TEXT)
    gmax = max(float(want_i.abs().max()), float(want_t.abs().max()))
    assert float((d_img.double().cpu() - want_i).abs().max()) <= 32 * ULP * gmax
    assert float((d_txt.double().cpu() - want_t).abs().max()) <= 32 * ULP * gmax


def test_src_head_is_deterministic(dev):
    x = inputs(33, 65, 130)
    first = head(dev, x, 100.0, want_logits=True)
    second = head(dev, x, 100.0, want_logits=True)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    x = inputs(5, 1030, 768)
    for a, b in zip(head(dev, x, 100.0, want_logits=True), head(dev, x, 100.0, want_logits=True)):
        assert torch.equal(a, b)


def test_src_head_forward_only(dev):
    from fsp_amd import _native
    x = inputs(5, 1030, 768)
    loss, _, d_img, d_txt = head(dev, x, 100.0, grad=False)
    assert d_img is None and d_txt is None
    assert torch.equal(loss, head(dev, x, 100.0)[0])
    # the C entry point with null gradients leaves a caller's buffers alone (nothing else to write to)
    lib = _native.load()
    img, txt, zs, fixed_n, fixed_q, y, _ = (t.to(dev) for t in x)
    ws = torch.empty(lib.clipk_src_head_ws_bytes(5, 1030, 768), dtype=torch.uint8, device=dev)
    out = torch.zeros(5, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.clipk_src_head(5, 1030, 768, p(img), p(txt), p(zs), p(fixed_n), p(fixed_q), p(y), None, 0.0, 0, 100.0,
                              W_TEXT, W_IMAGE, W_LOGITS, 1.0, p(out), None, None, None, p(ws), st) == 0
    assert torch.equal(out, loss)


def test_src_head_grad_scale(dev):
    check(dev, 4, 37, 512, 100.0, grad_scale=0.25)


@pytest.mark.parametrize("B,C,E", [(4, 100, 512), (33, 65, 130)])
def test_src_head_logits(dev, B, C, E):
    for scale in SCALES:
        x, _, ref, _ = case(dev, B, C, E, scale)
        _, logits, _, _ = head(dev, x, scale, want_logits=True)
        err = float((logits.double().cpu() - ref[3]).abs().max())
        print(f"src_head logits ({B}, {C}, {E}) scale {scale:g}: err {err:.3e} (bound {16 * ULP * scale:.3e})")
        assert logits.shape == (B, C)
        assert err <= 16 * ULP * scale


def test_src_head_zero_row_forward(dev):
    """An all-zero raw row normalises to zero (the 1e-12 clamp of F.normalize): forward only."""
    img, txt, zs, fixed_n, fixed_q, y, alpha = inputs(3, 7, 64)
    img[1] = 0.0
    txt[2] = 0.0
    x = (img, txt, zs, fixed_n, fixed_q, y, alpha)
    ref = reference(img, txt, zs, fixed_n, fixed_q, y, 100.0, grad=False)
    parts, _, _ = composition(dev, img, txt, zs, fixed_n, fixed_q, y, 100.0, grad=False)
    e_loss = float((parts[0].double().cpu() - ref[0][0]).abs())
    loss = head(dev, x, 100.0, grad=False)[0]
    k = (loss.double().cpu() - ref[0]).abs()
    print(f"src_head zero rows: loss64 {float(ref[0][0]):.6f} err torch {e_loss:.3e} kernel {float(k[0]):.3e}")
    assert torch.isfinite(loss).all()
    for i, name in enumerate(NAMES):
        assert float(k[i]) <= loss_bound(e_loss, ref[0][i]), name


def test_src_head_label_out_of_range_is_nan(dev):
    img, txt, zs, fixed_n, fixed_q, y, alpha = inputs(4, 37, 512)
    for bad in (37, -1, 2 ** 40):
        yb = y.clone()
        yb[1] = bad
        loss, _, d_img, d_txt = head(dev, (img, txt, zs, fixed_n, fixed_q, yb, alpha), 100.0)
        torch.cuda.synchronize()
        assert torch.isnan(loss[0]) and torch.isnan(loss[1])
        assert torch.isfinite(loss[2:]).all()


def test_src_head_fn_through_autograd(dev):
    from fsp_amd.trainers._fns import SRCHeadFn, backward_unit, src_head_fused_ok
    x = inputs(4, 37, 512)
    img0, txt0, zs, fixed_n, fixed_q, y, alpha = (t.to(dev) for t in x)
    assert src_head_fused_ok(img0, txt0, zs, fixed_n, fixed_q)
    assert not src_head_fused_ok(img0.half(), txt0, zs, fixed_n, fixed_q)
    assert not src_head_fused_ok(img0, txt0[:, :8], zs, fixed_n, fixed_q)
    loss0, logits0, d_img, d_txt = head(dev, x, 100.0, focal=True, want_logits=True)
    args = (zs, fixed_n, fixed_q, y, alpha, 2.0, True, 100.0, W_TEXT, W_IMAGE, W_LOGITS)
    for factor in (1.0, 3.0):
        img, txt = img0.clone().requires_grad_(), txt0.clone().requires_grad_()
        out = {"want_logits": True}
        total = SRCHeadFn.apply(img, txt, *args, out)
        assert total.shape == () and torch.equal(total.detach(), loss0[0])
        assert torch.equal(out["parts"], loss0) and torch.equal(out["logits"], logits0)
        if factor == 1.0:
            backward_unit(total)
        else:
            (total * factor).backward()
        assert torch.equal(img.grad, d_img * factor) and torch.equal(txt.grad, d_txt * factor)
    with torch.no_grad():  # no gradient asked for: forward only
        assert torch.equal(SRCHeadFn.apply(img0, txt0, *args), loss0[0])


def test_src_head_rejects_bad_inputs(dev):
    from fsp_amd import ops
    from fsp_amd._native import ClipkError
    img, txt, zs, fixed_n, fixed_q, y, alpha = (t.to(dev) for t in inputs(4, 37, 512))

    def call(img=img, txt=txt, zs=zs, fixed_n=fixed_n, fixed_q=fixed_q, y=y, scale=100.0, focal=False, gamma=0.0):
        return ops.src_head(img, txt, zs, fixed_n, fixed_q, y, None, gamma, focal, scale, W_TEXT, W_IMAGE, W_LOGITS)

    e0 = torch.empty(0, 512, device=dev)
    big = torch.randn(129, 512, device=dev)
    for kw in (dict(img=e0, zs=e0, y=y[:0]),                                     # B = 0
               dict(img=big, zs=big, y=torch.zeros(129, dtype=torch.long, device=dev)),  # B above the range
               dict(img=img.half()), dict(txt=txt.half()), dict(fixed_q=fixed_q.half()),  # fp16 inputs
               dict(txt=txt[:, :500].contiguous()), dict(zs=zs[:, :500].contiguous()),   # mismatched E
               dict(fixed_n=fixed_n[:30]), dict(y=y[:3]), dict(y=y.int()),
               dict(img=img.cpu()), dict(y=y.cpu()),                                # CPU tensors
               dict(scale=0.0), dict(focal=True, gamma=-1.0)):
        with pytest.raises(ClipkError):
            call(**kw)


def test_src_head_c_abi_status_codes(dev):
    """The entry point's own checks (the wrapper refuses these before the call)."""
    from fsp_amd import _native
    lib = _native.load()
    B, C, E = 4, 6, 8
    f = torch.randn(8, E, device=dev)
    y = torch.zeros(B, dtype=torch.long, device=dev)
    out = torch.zeros(5, device=dev)
    d = torch.zeros(8, E, device=dev)
    ws = torch.empty(lib.clipk_src_head_ws_bytes(B, C, E), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.clipk_src_head_ws_bytes(0, C, E) == 0 and lib.clipk_src_head_ws_bytes(129, C, E) == 0
    assert lib.clipk_src_head_ws_bytes(B, 0, E) == 0 and lib.clipk_src_head_ws_bytes(B, C, 0) == 0
    assert lib.clipk_src_head_ws_bytes(B, C, E) > 0 and lib.clipk_src_head_ws_bytes(128, 1, 1) > 0

    def call(B=B, C=C, E=E, img=p(f), txt=p(f), zs=p(f), fn=p(f), fq=p(f), y=p(y), gamma=0.0, focal=0, scale=100.0,
             loss=p(out), d_img=None, d_txt=None, ws=p(ws)):
        return lib.clipk_src_head(B, C, E, img, txt, zs, fn, fq, y, None, gamma, focal, scale, W_TEXT, W_IMAGE,
                                  W_LOGITS, 1.0, loss, None, d_img, d_txt, ws, st)

    assert call() == 0
    for kw in (dict(B=0), dict(B=129), dict(C=0), dict(E=0)):
        assert call(**kw) == -2, kw
    for kw in (dict(img=None), dict(txt=None), dict(zs=None), dict(fn=None), dict(fq=None), dict(y=None),
               dict(loss=None), dict(ws=None), dict(d_img=p(d)), dict(d_txt=p(d)), dict(scale=0.0), dict(scale=-1.0),
               dict(focal=1, gamma=-0.5)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
