"""GPU: clipk_probe_head (csrc/probe.hip) against the fp64 reference of probe_util.

Inputs for shape (B, C, E): probe_util.inputs (seed 1000003 B + 1009 C + E). Modes (normalize,
scale): (True, 14.285714), (True, 100), (False, 1). Reference: probe_util.reference, fp64 on the
CPU, autograd for the gradients of w and bias (oracle.focal_loss in place of CE for focal).

Tolerance: the rule of tests/test_ntxent_gpu.py / test_srchead_gpu.py. The flag-off fp32 torch
composition (F.normalize, scale * F.linear + bias, CrossEntropyFn, autograd) is measured on the
device against the same reference -- e_loss absolute, e_grad relative to max |grad64| over d_w and
d_bias -- and the kernel must stay within max(8 e_loss, 16 ulp max(1, |loss64|)) for the loss and
within max(8 e_grad, 32 ulp) for the gradients, ulp = 2^-24. Logits: within
16 ulp max(scale, max |s64|) of the fp64 logits.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from probe_util import inputs, reference, MODES

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8), (1, 2, 5), (2, 3, 37), (3, 7, 64), (4, 37, 512), (4, 1000, 512), (5, 1030, 768),
          (32, 1000, 512), (33, 65, 130), (128, 10, 512), (257, 100, 96), (512, 1000, 512)]
ULP = 2.0 ** -24
_CASES = {}


def composition(dev, feat, w, bias, y, normalize, scale, alpha=None, focal=False, grad=True):
    """The flag-off head of LinearProbeModel in fp32 on the device: (loss, d_w, d_bias)."""
    from fsp_amd.trainers._fns import CrossEntropyFn
    f = feat.to(dev)
    wd = w.to(dev).requires_grad_(grad)
    bd = bias.to(dev).requires_grad_(grad) if bias is not None else None
    u = F.normalize(f, dim=-1) if normalize else f
    s = scale * F.linear(u, wd)
    if bd is not None:
        s = s + bd
    a = alpha.to(dev) if alpha is not None else None
    loss = CrossEntropyFn.apply(s, y.to(dev), a, 2.0 if focal else 0.0, focal)
    if not grad:
        return loss.detach(), None, None
    loss.backward()
    return loss.detach(), wd.grad, (bd.grad if bd is not None else None)


def grad_err(d_w, d_b, ref, factor=1.0):
    """max |g - factor g64| over d_w and d_bias, relative to factor max |grad64| over both."""
    _, dw64, db64, _ = ref
    gmax = float(dw64.abs().max())
    worst = float((d_w.double().cpu() - factor * dw64).abs().max())
    if db64 is not None:
        gmax = max(gmax, float(db64.abs().max()))
        worst = max(worst, float((d_b.double().cpu() - factor * db64).abs().max()))
    return worst / (factor * gmax) if gmax > 0 else worst


def case(dev, B, C, E, normalize, scale, focal=False, with_bias=True):
    """Inputs, fp64 reference and the composition's errors of a case, computed once."""
    key = (B, C, E, normalize, scale, focal, with_bias)
    if key not in _CASES:
        feat, w, bias, y, alpha = inputs(B, C, E)
        b = bias if with_bias else None
        a = alpha if focal else None
        ref = reference(feat, w, b, y, normalize, scale, a, focal)
        loss, dw, db = composition(dev, feat, w, b, y, normalize, scale, a, focal)
        e_loss = abs(float(loss) - float(ref[0]))
        _CASES[key] = ((feat, w, b, y, a), ref, (e_loss, grad_err(dw, db, ref)))
    return _CASES[key]


def loss_bound(e_loss, loss64):
    return max(8 * e_loss, 16 * ULP * max(1.0, abs(float(loss64))))


def grad_bound(e_grad):
    return max(8 * e_grad, 32 * ULP)


def head(dev, x, normalize, scale, focal=False, **kw):
    from fsp_amd import ops
    feat, w, b, y, a = (t.to(dev) if t is not None else None for t in x)
    return ops.probe_head(feat, w, b, y, a, 2.0 if focal else 0.0, focal, normalize, scale, **kw)


def check(dev, B, C, E, normalize, scale, focal=False, with_bias=True, grad_scale=1.0):
    x, ref, (e_loss, e_grad) = case(dev, B, C, E, normalize, scale, focal, with_bias)
    if C > 1:
        feat, w, b, y, _ = x
        ce64 = float(reference(feat, w, b, y, normalize, scale, grad=False)[0]) if focal else float(ref[0])
        assert ce64 >= 0.02  # not at a saturated loss
    loss, logits, d_w, d_b = head(dev, x, normalize, scale, focal, want_logits=True, grad_scale=grad_scale)
    assert loss.shape == () and logits.shape == (B, C) and d_w.shape == (C, E)
    assert (d_b is None) == (not with_bias) and (d_b is None or d_b.shape == (C,))
    k_loss = abs(float(loss) - float(ref[0]))
    k_grad = grad_err(d_w, d_b, ref, grad_scale)
    s64 = ref[3]
    k_logit = float((logits.double().cpu() - s64).abs().max())
    b_logit = 16 * ULP * max(scale, float(s64.abs().max()))
    tag = (f"probe_head ({B}, {C}, {E}) normalize {int(normalize)} scale {scale:g}{' focal' if focal else ''}"
           f"{'' if with_bias else ' no bias'}{'' if grad_scale == 1.0 else f' grad_scale {grad_scale:g}'}")
    print(f"{tag}: loss64 {float(ref[0]):.6f}  loss err torch {e_loss:.3e} kernel {k_loss:.3e} "
          f"(bound {loss_bound(e_loss, ref[0]):.3e})  grad err torch {e_grad:.3e} kernel {k_grad:.3e} "
          f"(bound {grad_bound(e_grad):.3e})  logits err {k_logit:.3e} (bound {b_logit:.3e})")
    assert k_loss <= loss_bound(e_loss, ref[0])
    assert k_grad <= grad_bound(e_grad)
    assert k_logit <= b_logit
    return loss, logits, d_w, d_b


@pytest.mark.parametrize("normalize,scale", MODES)
@pytest.mark.parametrize("B,C,E", SHAPES)
def test_probe_head_matches_fp64_reference(dev, B, C, E, normalize, scale):
    loss, _, d_w, d_b = check(dev, B, C, E, normalize, scale)
    if C == 1:  # one class: log-softmax of a single logit
        assert float(loss) == 0.0 and not d_w.any() and not d_b.any()


@pytest.mark.parametrize("B,C,E", [(4, 37, 512), (33, 65, 130)])
def test_probe_head_focal_with_alpha(dev, B, C, E):
    for normalize, scale in MODES:
        check(dev, B, C, E, normalize, scale, focal=True)


@pytest.mark.parametrize("B,C,E", [(2, 3, 37), (4, 1000, 512)])
def test_probe_head_without_bias(dev, B, C, E):
    _, _, _, d_b = check(dev, B, C, E, True, 100.0, with_bias=False)
    assert d_b is None


def test_probe_head_grad_scale(dev):
    check(dev, 4, 37, 512, True, 100.0, grad_scale=0.25)
    check(dev, 33, 65, 130, False, 1.0, grad_scale=0.25)


def test_probe_head_one_class_is_exactly_zero(dev):
    for B, E in ((1, 8), (5, 130)):
        for normalize, scale in MODES:
            for focal in (False, True):
                x = inputs(B, 1, E)[:4] + ((inputs(B, 1, E)[4] if focal else None),)
                loss, _, d_w, d_b = head(dev, x, normalize, scale, focal)
                assert float(loss) == 0.0 and not d_w.any() and not d_b.any()


def test_probe_head_is_deterministic(dev):
    for shape in ((33, 65, 130), (512, 1000, 512)):
        x = inputs(*shape)[:4] + (None,)
        first = head(dev, x, True, 100.0, want_logits=True)
        second = head(dev, x, True, 100.0, want_logits=True)
        for a, b in zip(first, second):
            assert torch.equal(a, b)


def _c_call(dev):
    from fsp_amd import _native
    lib = _native.load()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib, p, st


def test_probe_head_forward_only(dev):
    B, C, E = 5, 1030, 768
    x = inputs(B, C, E)[:4] + (None,)
    loss, logits, d_w, d_b = head(dev, x, True, 100.0, grad=False)
    assert logits is None and d_w is None and d_b is None
    assert torch.equal(loss, head(dev, x, True, 100.0)[0])
    # the C entry point with null gradients leaves a caller's buffers alone (nothing else to write to)
    lib, p, st = _c_call(dev)
    feat, w, b, y, _ = (t.to(dev) if t is not None else None for t in x)
    ws = torch.empty(lib.clipk_probe_head_ws_bytes(B, C, E), dtype=torch.uint8, device=dev)
    out = torch.zeros((), device=dev)
    assert lib.clipk_probe_head(B, C, E, p(feat), p(w), p(b), p(y), None, 0.0, 0, 1, 100.0, 1.0, p(out), None, None,
                                None, p(ws), st) == 0
    assert torch.equal(out, loss)


@pytest.mark.parametrize("B,C,E", [(33, 65, 130), (4, 1000, 512)])
def test_probe_head_scoring_only(dev, B, C, E):
    lib, p, st = _c_call(dev)
    for normalize, scale in MODES:
        x = inputs(B, C, E)[:4] + (None,)
        full = head(dev, x, normalize, scale, want_logits=True)[1]
        none, logits, d_w, d_b = head(dev, x[:3] + (None, None), normalize, scale)
        assert none is None and d_w is None and d_b is None
        assert torch.equal(logits, full)
        # without a bias, through the C entry point; no workspace, and no other buffer is given
        feat, w = x[0].to(dev), x[1].to(dev)
        out = torch.empty(B, C, device=dev)
        assert lib.clipk_probe_head(B, C, E, p(feat), p(w), None, None, None, 0.0, 0, int(normalize), scale, 1.0, None,
                                    p(out), None, None, None, st) == 0
        assert torch.equal(out, head(dev, x[:2] + (None, x[3], None), normalize, scale, want_logits=True)[1])
    # a loss buffer is refused in this mode and stays as it was
    loss = torch.full((), 7.0, device=dev)
    assert lib.clipk_probe_head(B, C, E, p(feat), p(w), None, None, None, 0.0, 0, 1, 100.0, 1.0, p(loss), p(out), None,
                                None, None, st) == -1
    assert float(loss) == 7.0


def test_probe_head_zero_row_forward(dev):
    """An all-zero feature row normalises to zero (the 1e-12 clamp of F.normalize): forward only."""
    feat, w, bias, y, _ = inputs(3, 7, 64)
    feat[1] = 0.0
    ref = reference(feat, w, bias, y, True, 100.0, grad=False)
    c_loss, _, _ = composition(dev, feat, w, bias, y, True, 100.0, grad=False)
    e_loss = abs(float(c_loss) - float(ref[0]))
    loss, logits, _, _ = head(dev, (feat, w, bias, y, None), True, 100.0, grad=False, want_logits=True)
    k = abs(float(loss) - float(ref[0]))
    print(f"probe_head zero row: loss64 {float(ref[0]):.6f} err torch {e_loss:.3e} kernel {k:.3e}")
    assert torch.isfinite(loss) and torch.isfinite(logits).all()
    assert torch.equal(logits[1].cpu(), bias)
    assert k <= loss_bound(e_loss, ref[0])


def test_probe_head_label_out_of_range_is_nan(dev):
    feat, w, bias, y, _ = inputs(4, 37, 512)
    for bad in (37, -1, 2 ** 40):
        yb = y.clone()
        yb[1] = bad
        loss, _, d_w, d_b = head(dev, (feat, w, bias, yb, None), True, 100.0)
        torch.cuda.synchronize()
        assert torch.isnan(loss)
        assert torch.isnan(head(dev, (feat, w, bias, yb, None), True, 100.0, grad=False)[0])


def test_probe_head_fn_through_autograd(dev):
    from fsp_amd.trainers._fns import ProbeHeadFn, backward_unit, probe_head_fused_ok
    x = inputs(4, 37, 512)
    feat, w0, b0, y, alpha = (t.to(dev) for t in x)
    assert probe_head_fused_ok(feat, w0, b0) and probe_head_fused_ok(feat, w0, None)
    assert not probe_head_fused_ok(feat.half(), w0, b0)
    assert not probe_head_fused_ok(feat, w0[:, :8], b0)
    assert not probe_head_fused_ok(feat, w0, b0[:5])
    loss0, logits0, d_w, d_b = head(dev, x, True, 100.0, focal=True, want_logits=True)
    args = (y, alpha, 2.0, True, True, 100.0)
    for factor in (1.0, 3.0):
        w, b = w0.clone().requires_grad_(), b0.clone().requires_grad_()
        out = {"want_logits": True}
        loss = ProbeHeadFn.apply(feat, w, b, *args, out)
        assert loss.shape == () and torch.equal(loss.detach(), loss0)
        assert torch.equal(out["logits"], logits0)
        if factor == 1.0:
            backward_unit(loss)
        else:
            (loss * factor).backward()
        assert torch.equal(w.grad, d_w * factor) and torch.equal(b.grad, d_b * factor)
    w = w0.clone().requires_grad_()  # no bias: one gradient
    backward_unit(ProbeHeadFn.apply(feat, w, None, *args))
    assert torch.equal(w.grad, head(dev, x[:2] + (None,) + x[3:], True, 100.0, focal=True)[2])
    with torch.no_grad():  # no gradient asked for: forward only
        assert torch.equal(ProbeHeadFn.apply(feat, w0, b0, *args), loss0)


def test_probe_head_rejects_bad_inputs(dev):
    from fsp_amd import ops
    from fsp_amd._native import ClipkError
    feat, w, bias, y, alpha = (t.to(dev) for t in inputs(4, 37, 512))

    def call(feat=feat, w=w, bias=bias, y=y, scale=100.0, focal=False, gamma=0.0):
        return ops.probe_head(feat, w, bias, y, None, gamma, focal, True, scale)

    e0 = torch.empty(0, 512, device=dev)
    big = torch.randn(513, 512, device=dev)
    for kw in (dict(feat=e0, y=y[:0]),                                              # B = 0
               dict(feat=big, y=torch.zeros(513, dtype=torch.long, device=dev)),   # B above the range
               dict(feat=feat.half()), dict(w=w.half()), dict(bias=bias.half()),    # fp16 inputs
               dict(w=w[:, :500].contiguous()), dict(feat=feat[:, :500].contiguous()),  # mismatched E
               dict(feat=feat.t().contiguous().t()),                                # not contiguous
               dict(bias=bias[:30]), dict(y=y[:3]), dict(y=y.int()),
               dict(feat=feat.cpu()), dict(y=y.cpu()), dict(w=w.cpu()),               # CPU tensors
               dict(scale=0.0), dict(focal=True, gamma=-1.0)):
        with pytest.raises(ClipkError):
            call(**kw)


def test_probe_head_c_abi_status_codes(dev):
    """The entry point's own checks (the wrapper refuses these before the call)."""
    lib, p, st = _c_call(dev)
    B, C, E = 4, 6, 8
    f = torch.randn(8, E, device=dev)
    bias = torch.zeros(8, device=dev)
    y = torch.zeros(B, dtype=torch.long, device=dev)
    out = torch.zeros((), device=dev)
    lg = torch.zeros(8, 8, device=dev)
    d = torch.zeros(8, E, device=dev)
    db = torch.zeros(8, device=dev)
    ws = torch.empty(lib.clipk_probe_head_ws_bytes(B, C, E), dtype=torch.uint8, device=dev)
    size = lib.clipk_probe_head_ws_bytes
    assert size(0, C, E) == 0 and size(513, C, E) == 0 and size(B, 0, E) == 0 and size(B, C, 0) == 0
    assert size(B, C, E) > 0 and size(512, 1, 1) > 0

    def call(B=B, C=C, E=E, feat=p(f), w=p(f), bias=p(bias), y=p(y), gamma=0.0, focal=0, scale=100.0, loss=p(out),
             logits=None, d_w=None, d_bias=None, ws=p(ws)):
        return lib.clipk_probe_head(B, C, E, feat, w, bias, y, None, gamma, focal, 1, scale, 1.0, loss, logits, d_w,
                                    d_bias, ws, st)

    assert call() == 0
    assert call(d_w=p(d), d_bias=p(db)) == 0
    assert call(bias=None, d_w=p(d)) == 0
    assert call(y=None, loss=None, logits=p(lg), ws=None) == 0  # scoring only
    for kw in (dict(B=0), dict(B=513), dict(C=0), dict(E=0)):
        assert call(**kw) == -2, kw
    for kw in (dict(feat=None), dict(w=None), dict(loss=None), dict(ws=None), dict(scale=0.0), dict(scale=-1.0),
               dict(focal=1, gamma=-0.5),
               dict(d_w=p(d)),                          # a bias and d_w without d_bias
               dict(d_bias=p(d)),                       # d_bias without d_w
               dict(bias=None, d_w=p(d), d_bias=p(d)),  # d_bias without a bias
               dict(y=None, loss=None, ws=None),        # scoring only without logits
               dict(y=None, logits=p(lg)),              # ... with a loss
               dict(y=None, loss=None, logits=p(lg), d_w=p(d)),
               dict(y=None, loss=None, logits=p(lg), d_bias=p(d))):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
