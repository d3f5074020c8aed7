"""GPU: the csrc/prompt.hip kernels one by one -- casts, row copies, prompt assembly and its context
gradient, ViT embedding + ln_pre, cosine logits, the CE / focal loss in its three entry points, the
Meta-Net and the guarded SGD step -- per element against tests/prompt_ref.py.

Exact kernels (cast, rows_copy, prompt_assemble, the guarded SGD step) are compared bitwise.
Floating kernels are gated per element at
    |got_i - ref_i| <= A 2^-24 S_i + 2^-24 |ref_i|
with ref and S from the fp64 restatement (S: the |.| sum the rounding error scales with) and A the
count of roundings on the element's path, derived at each test from the kernel's code. Where the
path goes through __expf / __logf / rsqrtf / powf, whose errors the code does not state, A is not
guessed: the same formula runs in torch fp32 on the CPU, its worst err_i / (2^-24 S_i + 2^-24 |ref_i|)
is the restatement's ratio r, and the kernel's ratio must stay within max(8 r, 1) -- the factor 8 of
test_lora_kernels_gpu.py / test_conv_gpu.py / test_resnet_gpu.py (another summation order, fast
intrinsics a few ulp wider than libm), the floor 1 because the gate's own last term grants one rounding
of the output even when the restatement happens to be exact. The kernel's output never enters a bound.

Every output is written into a buffer with canary elements on both sides. A rejected call raises
ClipkError with its documented status and leaves the whole canaried buffer untouched after a
synchronize (the library returns before its launch; nothing else could be observed of one).
"""
import ctypes

import pytest
import torch

import prompt_ref as PR

pytestmark = pytest.mark.gpu

U = PR.U
GUARD = 64  # canary elements on each side (256 B of fp32: the body stays 16-byte aligned)
CAN = -1234.5
BIG = 8192 * 256 + 257  # one element past a wrapped grid-stride loop (grid_for caps at 8192 blocks)


def _mods():
    from fsp_amd import ops, _native as N
    return ops, N


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Keep:
    """Device copies of host tensors as pointers, the copies kept alive with this object: a temporary
    freed before the launch hands its block to the next allocation, and the kernel would read that."""

    def __init__(self, dev):
        self.dev, self.refs = dev, []

    def __call__(self, t):
        if t is None:
            return None
        self.refs.append(t.to(self.dev))
        return ctypes.c_void_p(self.refs[-1].data_ptr())


def _canary(n, dev, dtype=torch.float32, fill=CAN):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _edges_ok(buf, n, fill=CAN):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def _rejected(status, fn, *bufs):
    """fn raises ClipkError with ``status``; every canaried buffer is untouched afterwards."""
    _, N = _mods()
    with pytest.raises(N.ClipkError, match=rf"status {status}\b"):
        fn()
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == CAN).all())


def _ratio(got, ref, S):
    """worst err_i / (2^-24 S_i + 2^-24 |ref_i|); 0 / 0 (an exact zero with no terms) counts as 0."""
    err = (got.double() - ref).abs()
    unit = U * (S + ref.abs())
    r = torch.where(err == 0, torch.zeros_like(err), err / unit.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def _gate(name, got, ref, S, rest=None, A=None):
    """The kernel's ratio against A (derived) or against max(8 x the fp32 restatement's ratio, 1)."""
    assert bool(torch.isfinite(got).all()), name
    k = _ratio(got, ref, S)
    if rest is not None:
        r = _ratio(rest, ref, S)
        print(f"{name}: restatement ratio {r:.3f}, kernel ratio {k:.3f}, gate {max(8 * r, 1.0):.3f}")
        assert k <= max(8 * r, 1.0), (name, k, r)
        return k, r
    print(f"{name}: kernel ratio {k:.3f}, gate A = {A}")
    assert k <= A, (name, k, A)
    return k, None


# ================================================================ exact kernels
def _cast_values(n, dtype):
    g = torch.Generator().manual_seed(n)
    inf, nan = float("inf"), float("nan")
    sp = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),  # bf16 ties, both parities
          1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),  # fp16 ties
          0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 6e-8, 5.9e-5, 2.0 ** -14,  # fp16 subnormals
          1023 * 2.0 ** -24 + 2.0 ** -25, 65504.0, 65519.9, 65520.0, -65520.0, 1e5,  # fp16 overflow
          3.38e38, 3.39e38, 3.4e38, -3.4e38, inf, -inf, nan, 1e-40, -1e-45]  # bf16 overflow, fp32 subnormals
    x = torch.tensor(sp, dtype=torch.float32)
    if n > x.numel():
        m = n - x.numel()
        scales = 10.0 ** torch.randint(-6, 7, (m,), generator=g).float()
        x = torch.cat([x, torch.randn(m, generator=g) * scales])
    else:  # n = 1: one tie of the target type
        x = x[{torch.bfloat16: 1, torch.float16: 5, torch.float32: 0}[dtype]:][:n]
    return x.contiguous()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n", [1, 255, 257, BIG])
def test_cast_bitwise(dev, dtype, n):
    """clipk_cast against CPU tensor.to(dtype) (round to nearest even): bit for bit, NaN by NaN-ness."""
    ops, N = _mods()
    x = _cast_values(n, dtype)
    ref = x.to(dtype)
    buf, body = _canary(n, dev, dtype)
    xd = x.to(dev)
    N.call("clipk_cast", ops.DT[dtype], n, _P(xd), _P(body), ops._stream())
    torch.cuda.synchronize()
    assert _edges_ok(buf, n)
    got = body.cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(bits)[~nan], ref.view(bits)[~nan])
    if n == 257:  # the wrapper is the same launch; a negative length is refused
        y = ops.cast(xd, dtype).cpu()
        assert torch.equal(y.view(bits)[~nan], ref.view(bits)[~nan])
        buf2, body2 = _canary(n, dev, dtype)
        _rejected(-2, lambda: N.call("clipk_cast", ops.DT[dtype], -1, _P(xd), _P(body2), ops._stream()), buf2)
        _rejected(-3, lambda: N.call("clipk_cast", 7, n, _P(xd), _P(body2), ops._stream()), buf2)


ICAN = 0x5A5A5A5A


@pytest.mark.parametrize("row_bytes", [16, 48, 2048])
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("tables", ["none", "src", "dst", "both"])
def test_rows_copy(dev, row_bytes, n, tables):
    """dst row (dst_rows ? dst_rows[i] : i) = src row (src_rows ? src_rows[i] : i), bit for bit; the
    destination rows no entry names keep their canary."""
    ops, N = _mods()
    g = torch.Generator().manual_seed(row_bytes + n)
    w = row_bytes // 4
    Rs, Rd = n + 5, n + 3
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (Rs, w), generator=g, dtype=torch.int64).to(torch.int32)
    sr = torch.randint(0, Rs, (n,), generator=g).to(torch.int32) if tables in ("src", "both") else None
    dr = torch.randperm(Rd, generator=g)[:n].to(torch.int32) if tables in ("dst", "both") else None
    buf = torch.full(((Rd + 2) * w,), ICAN, dtype=torch.int32, device=dev)  # one guard row on each side
    body = buf[w:w + Rd * w].view(Rd, w)
    want = torch.full((Rd, w), ICAN, dtype=torch.int32)
    want[(dr.long() if dr is not None else torch.arange(n))] = src[(sr.long() if sr is not None else torch.arange(n))]
    d = lambda t: None if t is None else t.to(dev)
    srd, drd, srcd = d(sr), d(dr), src.to(dev)
    N.call("clipk_rows_copy", row_bytes, n, _P(srcd), _P(srd), _P(body), _P(drd), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(body.cpu(), want)
    assert bool((buf[:w] == ICAN).all()) and bool((buf[w + Rd * w:] == ICAN).all())


def test_rows_copy_rejections(dev):
    """row_bytes no multiple of 16, a pointer 4 bytes off 16-byte alignment (source or destination) and
    n < 0: CLIPK_ESHAPE (-2), nothing written."""
    ops, N = _mods()
    src = torch.arange(4 * 64, dtype=torch.float32, device=dev)
    buf, body = _canary(4 * 64, dev)
    st = ops._stream()
    _rejected(-2, lambda: N.call("clipk_rows_copy", 24, 4, _P(src), None, _P(body), None, st), buf)
    _rejected(-2, lambda: N.call("clipk_rows_copy", 16, 4, _P(src[1:]), None, _P(body), None, st), buf)
    _rejected(-2, lambda: N.call("clipk_rows_copy", 16, 4, _P(src), None, _P(body[1:]), None, st), buf)
    _rejected(-2, lambda: N.call("clipk_rows_copy", 16, -1, _P(src), None, _P(body), None, st), buf)
    _rejected(-2, lambda: N.call("clipk_rows_copy", 0, 4, _P(src), None, _P(body), None, st), buf)


def _layout(position, C=3, n_ctx=4, name_lens=(1, 3, 2)):
    from fsp_amd.trainers._fns import prompt_layout
    eot = [1 + n_ctx + nl + 1 for nl in name_lens]
    src, cpos, L = prompt_layout(C, n_ctx, list(name_lens), position, eot)
    assert L < 77  # truncated: a wrong embedding row stride (77 against L) shows
    return torch.from_numpy(src), torch.from_numpy(cpos), L


@pytest.mark.parametrize("position", ["end", "middle", "front"])
@pytest.mark.parametrize("W", [36, 512])
def test_prompt_assemble_bitwise(dev, position, W):
    """clipk_prompt_assemble against the restatement rounded in fp32 in the same order, (row + pos) +
    bias: bitwise. Ragged class names, the truncated L, shared / class-specific / per-image context
    strides, bias absent and [B, W]."""
    ops, N = _mods()
    C, n_ctx = 3, 4
    src, _, L = _layout(position)
    g = torch.Generator().manual_seed(W)
    emb = torch.randn(C, 77, W, generator=g)
    pos = torch.randn(77, W, generator=g)
    for B in (1, 3):
        bias = torch.randn(B, W, generator=g)
        for mode, shape, sb, sc in (("shared", (n_ctx, W), 0, 0), ("csc", (C, n_ctx, W), 0, n_ctx * W),
                                    ("per_image", (B, n_ctx, W), n_ctx * W, 0)):
            ctx = torch.randn(*shape, generator=g)
            for bs in (None, bias):
                want = PR.prompt_assemble(B, src, emb, ctx, sb, sc, bs, pos, dt=torch.float32)
                buf, body = _canary(B * C * L * W, dev)
                k = _Keep(dev)
                N.call("clipk_prompt_assemble", B, C, L, W, k(src), k(emb), k(ctx), sb, sc, k(bs), k(pos), _P(body),
                       ops._stream())
                torch.cuda.synchronize()
                assert _edges_ok(buf, B * C * L * W), (B, mode)
                got = body.cpu().view(B, C, L, W)
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (B, mode, bs is not None)
                if mode == "shared":  # the wrapper: the same launch
                    x0 = ops.prompt_assemble(B, C, L, src.to(dev), emb.to(dev), ctx.to(dev), sb, sc,
                                             None if bs is None else bs.to(dev), pos.to(dev))
                    assert torch.equal(x0.cpu().view(B, C, L, W), want)


def test_prompt_assemble_rejections(dev):
    ops, N = _mods()
    C, n_ctx = 3, 4
    src, _, L = _layout("end")
    z = lambda *s: torch.zeros(*s, device=dev)
    for W, Lx in ((6, L), (8, 78)):
        buf, body = _canary(2 * C * Lx * W, dev)
        sm = torch.zeros(C, Lx, dtype=torch.int32, device=dev)
        a = [z(C, 77, W), z(n_ctx, W), z(78, W)]
        _rejected(-2, lambda: N.call("clipk_prompt_assemble", 2, C, Lx, W, _P(sm), _P(a[0]), _P(a[1]), 0, 0, None,
                                     _P(a[2]), _P(body), ops._stream()), buf)


SGD_SIZES = [1000, 17, 4096, 1, 2048, 3, 255, 257, BIG, 64, 65, 5, 1023, 4097, 9, 300]


@pytest.mark.parametrize("gs", [1.0, 0.125], ids=["unscaled", "scaled"])
def test_sgd_step_multi_guard(dev, gs):
    """clipk_sgd_step_multi_if on 16 ragged tensors (one wraps the grid-stride loop): with
    flags & mask != 0 every p and buf is bitwise untouched; with the bit clear, or a mask that misses
    the set bit, the result is bitwise the unguarded update. Two steps (without and with a buffer)."""
    ops, N = _mods()
    assert len(SGD_SIZES) == 16
    g = torch.Generator().manual_seed(11)
    ps = [torch.randn(n, generator=g).to(dev) for n in SGD_SIZES]
    gr = [torch.randn(n, generator=g).to(dev) for n in SGD_SIZES]
    hyp = (0.002, 0.9, 5e-4)
    flag = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)

    def run(guard):
        p, b = [t.clone() for t in ps], [torch.zeros_like(t) for t in ps]
        for step in range(2):
            ops.sgd_step_multi(p, gr, b, *hyp, [step > 0] * 16, grad_scale=gs, guard=guard)
        torch.cuda.synchronize()
        return p, b

    pa, ba = run(None)
    assert not any(torch.equal(a, b) for a, b in zip(pa, ps))  # the unguarded step does move them
    for guard, skipped in (((flag(4), 4), True), ((flag(6), 4), True), ((flag(0), 4), False), ((flag(4), 2), False),
                           ((flag(4), 0), False)):
        p, b = run(guard)
        for k in range(16):
            if skipped:
                assert torch.equal(p[k], ps[k]) and not bool(b[k].any()), (k, guard[1])
            else:
                assert torch.equal(p[k], pa[k]) and torch.equal(b[k], ba[k]), (k, guard[1])


def test_sgd_step_multi_count_17_is_einval(dev):
    ops, N = _mods()
    c = 17
    bufs = [_canary(8, dev) for _ in range(3 * c)]
    bodies = [b for _, b in bufs]
    VP = ctypes.c_void_p * c
    arr = lambda ts: VP(*[t.data_ptr() for t in ts])
    args = (c, arr(bodies[:c]), arr(bodies[c:2 * c]), arr(bodies[2 * c:]), (ctypes.c_long * c)(*[8] * c),
            (ctypes.c_int * c)(*[0] * c), 0.1, 0.9, 0.0)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    full = [b for b, _ in bufs]
    _rejected(-1, lambda: N.call("clipk_sgd_step_multi", *args, ops._stream()), *full)
    _rejected(-1, lambda: N.call("clipk_sgd_step_multi_scaled", *args, 0.5, ops._stream()), *full)
    _rejected(-1, lambda: N.call("clipk_sgd_step_multi_if", *args, 0.5, _P(flags), 1, ops._stream()), *full)
    # ... and the guarded entry point without its guard
    a16 = (16,) + args[1:]
    _rejected(-1, lambda: N.call("clipk_sgd_step_multi_if", *a16, 1.0, None, 1, ops._stream()), *full)


# ================================================================ ViT embedding + ln_pre
VIT_CASES = [(1, 2, 4, 0, False), (3, 5, 36, 0, False), (5, 2, 260, 3, False), (2, 5, 768, 2, False),
             (1, 3, 1024, 1, False), (3, 5, 36, 2, True)]


def _vit_run(dev, name, B, L, D, n_vpt, patch, cls, pos, vpt, gam, bet):
    ops, N = _mods()
    rows = B * (L + n_vpt)
    buf, body = _canary(rows * D, dev)
    d = lambda t: None if t is None else t.to(dev)
    a = [d(t) for t in (patch, cls, pos, vpt, gam, bet)]
    if name == "clipk_vit_embed_ln":
        N.call(name, B, L, D, _P(a[0]), _P(a[1]), _P(a[2]), _P(a[4]), _P(a[5]), _P(body), ops._stream())
    else:
        N.call(name, B, L, n_vpt, D, _P(a[0]), _P(a[1]), _P(a[2]), _P(a[3]), _P(a[4]), _P(a[5]), _P(body),
               ops._stream())
    torch.cuda.synchronize()
    assert _edges_ok(buf, rows * D)
    return body.cpu().view(B, L + n_vpt, D)


@pytest.mark.parametrize("case", VIT_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_vit_embed_ln(dev, case):
    """clipk_vit_embed_ln / _vpt (B, L, D, n_vpt, large-mean rows): the smallest legal shape; a partial
    wave with a row count no multiple of 4; 65 float4s (one past a chunk); a real width; all four
    chunks; rows 100 + 0.01 randn. The path has rsqrtf: gated at max(8 x restatement, 1).
    Prompt rows carry no positional term: they are those of an embedding whose pos is zero.
    Measured on MI355X, restatement / kernel ratio per case in VIT_CASES order: 0.52 / 0.75, 1.31 / 1.12,
    1.52 / 1.30, 1.70 / 1.39, 1.24 / 1.32, 1.56 / 0.94 (gates 4.2 to 13.6)."""
    B, L, D, n_vpt, big_mean = case
    g = torch.Generator().manual_seed(D + L)
    rnd = (lambda *s: 100 + 0.01 * torch.randn(*s, generator=g)) if big_mean else (lambda *s: torch.randn(*s, generator=g))
    patch, cls, pos = rnd(B, L - 1, D), rnd(D), torch.randn(L, D, generator=g)
    vpt = rnd(n_vpt, D) if n_vpt else None
    gam, bet = 1 + 0.2 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    ref, S = PR.vit_embed_ln(patch, cls, pos, vpt, gam, bet)
    rest, _ = PR.vit_embed_ln(patch, cls, pos, vpt, gam, bet, dt=torch.float32)
    got = _vit_run(dev, "clipk_vit_embed_ln_vpt", B, L, D, n_vpt, patch, cls, pos, vpt, gam, bet)
    _gate(f"vit_embed_ln_vpt {case}", got, ref, S, rest=rest)
    if n_vpt == 0:
        got0 = _vit_run(dev, "clipk_vit_embed_ln", B, L, D, 0, patch, cls, pos, None, gam, bet)
        assert torch.equal(got0, got)
    else:
        # the prompt rows: LayerNorm of the vpt rows alone, whatever pos holds
        got2 = _vit_run(dev, "clipk_vit_embed_ln_vpt", B, L, D, n_vpt, patch, cls, pos * 3 + 1, vpt, gam, bet)
        assert torch.equal(got2[:, L:], got[:, L:]) and not torch.equal(got2[:, :L], got[:, :L])
        for b in range(1, B):
            assert torch.equal(got[b, L:], got[0, L:])


def test_vit_embed_ln_rejections(dev):
    ops, N = _mods()
    z = lambda *s: torch.zeros(*s, device=dev)
    st = ops._stream()
    for B, L, D in ((2, 3, 1028), (2, 3, 6), (2, 1, 8)):
        buf, body = _canary(B * (L + 1) * D, dev)
        a = [z(B, max(L - 1, 1), D), z(D), z(L, D), z(1, D), z(D), z(D)]
        _rejected(-2, lambda: N.call("clipk_vit_embed_ln", B, L, D, _P(a[0]), _P(a[1]), _P(a[2]), _P(a[4]), _P(a[5]),
                                     _P(body), st), buf)
        _rejected(-2, lambda: N.call("clipk_vit_embed_ln_vpt", B, L, 1, D, _P(a[0]), _P(a[1]), _P(a[2]), _P(a[3]),
                                     _P(a[4]), _P(a[5]), _P(body), st), buf)
    buf, body = _canary(2 * 3 * 8, dev)
    a = [z(2, 2, 8), z(8), z(3, 8), z(8), z(8)]
    _rejected(-2, lambda: N.call("clipk_vit_embed_ln_vpt", 2, 3, -1, 8, _P(a[0]), _P(a[1]), _P(a[2]), None, _P(a[3]),
                                 _P(a[4]), _P(body), st), buf)
    _rejected(-1, lambda: N.call("clipk_vit_embed_ln_vpt", 2, 3, 1, 8, _P(a[0]), _P(a[1]), _P(a[2]), None, _P(a[3]),
                                 _P(a[4]), _P(body), st), buf)


# ================================================================ context gradient
@pytest.mark.parametrize("position", ["end", "middle", "front"])
@pytest.mark.parametrize("C", [1, 3, 4, 9])
def test_ctx_grad(dev, position, C):
    """clipk_ctx_grad: C leaves waves idle (1, 3), fills the four (4), gives a ragged tail (9); W = 100
    is a partial second 64-column block. A = the number of classes summed: wave v adds classes v, v + 4,
    ... in order, then the four partials are added -- C - 1 roundings at the most, and plain additions
    only. Class-specific context (csc) sums nothing: bitwise the gathered row.
    Measured on MI355X: worst kernel ratio 1.24 over the 54 summed cases, 0.30 of its A at the most."""
    ops, N = _mods()
    n_ctx = 4
    lens = [1, 3, 2, 5, 1, 4, 2, 1, 3][:C]
    _, cpos, L = _layout(position, C, n_ctx, lens)
    g = torch.Generator().manual_seed(C)
    for W in (36, 100, 512):
        for B in (1, 3):
            dx0 = torch.randn(B, C, L, W, generator=g)
            for csc in (0, 1):
                ref, S = PR.ctx_grad(dx0, cpos, csc)
                outs = (B * C if csc else B) * n_ctx
                buf, body = _canary(outs * W, dev)
                k = _Keep(dev)
                N.call("clipk_ctx_grad", B, C, L, W, n_ctx, csc, k(cpos), k(dx0), _P(body), ops._stream())
                torch.cuda.synchronize()
                assert _edges_ok(buf, outs * W)
                got = body.cpu().view(outs, W)
                if csc or C == 1:
                    assert torch.equal(got.double(), ref), (W, B, csc)
                else:
                    _gate(f"ctx_grad {position} C={C} W={W} B={B}", got, ref, S, A=C)
                if W == 100:
                    d = ops.ctx_grad(B, C, L, W, n_ctx, csc, cpos.to(dev), dx0.to(dev))
                    assert torch.equal(d.cpu(), got)


# ================================================================ cosine logits
def _cos_case(dev, tag, B, C, E, per_image, scale, norm, seed):
    """Forward (logits, inv_t, inv_i) and backward (dtxt) at one shape. Forward: rsqrtf on the path,
    gated against the fp32 restatement. Backward (inv_t / inv_i as given: the restatement's fp32
    values go to the kernel and to the reference): plain fp32 arithmetic,
        dy: scale dl inv_i (2 roundings), times imf and the add (2), B terms -> (B + 3) u Sdy
        y = txt inv_t (1); y . dy: ceil(E / 64) terms per lane + 6 butterfly steps
        inv_t (dy - y yd): product, difference, product (3, and y's own)
    so A = B' + ceil(E / 64) + 14 with B' the images summed (1 when per_image)."""
    ops, N = _mods()
    g = torch.Generator().manual_seed(seed)
    rows = B * C if per_image else C
    imf = torch.randn(B, E, generator=g) * (norm / E ** 0.5)
    txt = torch.randn(rows, E, generator=g) * (norm / E ** 0.5)
    ref, it, iv, S = PR.cosine_logits(imf, txt, scale, per_image, C)
    r32, it32, iv32, _ = PR.cosine_logits(imf, txt, scale, per_image, C, dt=torch.float32)
    bl, lo = _canary(B * C, dev)
    bt, t_ = _canary(rows, dev)
    bi, i_ = _canary(B, dev)
    imd, txd = imf.to(dev), txt.to(dev)
    N.call("clipk_cosine_logits_fwd", B, C, E, per_image, scale, _P(imd), _P(txd), _P(lo), _P(t_), _P(i_), ops._stream())
    torch.cuda.synchronize()
    assert _edges_ok(bl, B * C) and _edges_ok(bt, rows) and _edges_ok(bi, B)
    out = []
    out.append(_gate(f"cos fwd logits {tag}", lo.cpu().view(B, C), ref, S, rest=r32))
    # inv norms: one-signed sums, S = the value
    out.append(_gate(f"cos fwd inv_t {tag}", t_.cpu(), it, it, rest=it32))
    out.append(_gate(f"cos fwd inv_i {tag}", i_.cpu(), iv, iv, rest=iv32))
    dl = torch.randn(B, C, generator=g)
    dref, dS = PR.cosine_logits_bwd(imf, txt, it32, iv32, dl, scale, per_image)
    bd, dt_ = _canary(rows * E, dev)
    k = _Keep(dev)
    N.call("clipk_cosine_logits_bwd", B, C, E, per_image, scale, _P(imd), _P(txd), k(it32), k(iv32), k(dl), _P(dt_),
           ops._stream())
    torch.cuda.synchronize()
    assert _edges_ok(bd, rows * E)
    A = (1 if per_image else B) + (E + 63) // 64 + 14
    out.append(_gate(f"cos bwd dtxt {tag}", dt_.cpu().view(rows, E), dref, dS, A=A))
    return out


def _cos_sweep(dev, B, C, E):
    worst = [0.0, 0.0, 0.0]
    for per_image in (0, 1):
        for scale in (1.0, 100.0):
            for norm in (1e-3, 10.0, 1e3):
                tag = f"B={B} C={C} E={E} per_image={per_image} scale={scale} |x|~{norm}"
                o = _cos_case(dev, tag, B, C, E, per_image, scale, norm, seed=E + C + B)
                worst[0] = max(worst[0], o[0][1], o[1][1], o[2][1])
                worst[1] = max(worst[1], o[0][0], o[1][0], o[2][0])
                worst[2] = max(worst[2], o[3][0])
    print(f"cosine B={B} C={C} E={E}: worst restatement ratio {worst[0]:.3f}, worst kernel ratio fwd {worst[1]:.3f}, "
          f"bwd {worst[2]:.3f}")


@pytest.mark.parametrize("E", [4, 64, 260, 512, 640, 768, 1024])
def test_cosine_logits_widths(dev, E):
    """C = 3, B = 5: E = 4 leaves 63 lanes idle, 260 is one float4 past a full wave, 640 / 768 / 1024
    are the CLIP embedding widths. per_image 0 / 1, scale 1 / 100, feature norms 1e-3, 10, 1e3.
    Measured on MI355X over this sweep and test_cosine_logits_shapes (300 runs), worst restatement /
    kernel ratio: logits 2.71 / 1.41, inv_t 1.19 / 1.02, inv_i 1.08 / 0.97 (the kernel at 0.42 of its gate
    at the most); backward worst kernel ratio 2.40 against A >= 16, 0.11 of its A at the most."""
    _cos_sweep(dev, 5, 3, E)


@pytest.mark.parametrize("C", [1, 3, 37])
@pytest.mark.parametrize("B", [1, 5, 33])
def test_cosine_logits_shapes(dev, B, C):
    for E in (64, 512):
        _cos_sweep(dev, B, C, E)


def test_cosine_logits_rejections(dev):
    ops, N = _mods()
    z = lambda *s: torch.zeros(*s, device=dev)
    st = ops._stream()
    B, C = 2, 3
    for E in (1028, 6):
        bl, lo = _canary(B * C, dev)
        bt, t_ = _canary(C, dev)
        bi, i_ = _canary(B, dev)
        a = [z(B, E), z(C, E)]
        _rejected(-2, lambda: N.call("clipk_cosine_logits_fwd", B, C, E, 0, 1.0, _P(a[0]), _P(a[1]), _P(lo), _P(t_),
                                     _P(i_), st), bl, bt, bi)
    bd, d_ = _canary(C * 1028, dev)
    a = [z(B, 1028), z(C, 1028), z(C), z(B), z(B, C)]
    _rejected(-2, lambda: N.call("clipk_cosine_logits_bwd", B, C, 1028, 0, 1.0, *[_P(t) for t in a], _P(d_), st), bd)


# ================================================================ CE / focal loss
GAMMAS = [0.0, 0.5, 1.0, 2.0, 5.0]
FIRST = {1: 3, 4: 0, 5: 1, 9: 0}  # the first row kind per batch size: every kind is met, B = 1 is saturated


def _loss_raw(dev, entry, z, y, alpha, gamma, focal, red, grad=True, lam=0.3):
    """One launch into canaried buffers -> (row losses [B], total or None, dlogits or None)."""
    ops, N = _mods()
    B, C = z.shape
    gs = 1.0 / B if red == "mean" else 1.0
    nrow = 2 * B if entry == "mix" else B
    br, row = _canary(nrow, dev)
    bt, tot = _canary(1, dev)
    bd, dl = _canary(B * C, dev)
    zd, yd, ad = z.to(dev), y.to(dev), None if alpha is None else alpha.to(dev)
    dlp = _P(dl) if grad else None
    st = ops._stream()
    if entry == "rows":
        N.call("clipk_ce_loss", B, C, _P(zd), _P(yd), _P(ad), gamma, int(focal), gs, _P(row), dlp, st)
    elif entry == "reduce":
        N.call("clipk_ce_loss_reduce", B, C, _P(zd), _P(yd), _P(ad), gamma, int(focal), gs, 1 if red == "mean" else 2,
               _P(row), _P(tot), dlp, st)
    else:
        N.call("clipk_ce_loss_mix", B, C, _P(zd), _P(yd), _P(yd), lam, _P(ad), gamma, int(focal), gs,
               1 if red == "mean" else 2, _P(row), _P(tot), dlp, st)
    torch.cuda.synchronize()
    assert _edges_ok(br, nrow) and _edges_ok(bt, 1) and _edges_ok(bd, B * C)
    if not grad:
        assert bool((bd == CAN).all())
    if entry == "rows":
        assert bool((bt == CAN).all())
    return row.cpu(), (tot.cpu()[0] if entry != "rows" else None), (dl.cpu().view(B, C) if grad else None)


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 130, 1000])
def test_ce_focal_losses(dev, C):
    """clipk_ce_loss, clipk_ce_loss_reduce and clipk_ce_loss_mix (y_a = y_b, lam 0.3) per element against
    the fp64 closed form: C around the 64-lane stride and at 1, 2, 1000; B in {1, 4, 5, 9} (the reduce
    kernel strides rows by 4, the mix kernel by 8); gamma in {0, 0.5, 1, 2, 5}; alpha absent and per
    class with one zero weight; mean and sum; rows randn * 4, uniform [-100, 100], all equal, saturated,
    anti-saturated and with -inf logits mixed in a batch.

    The path is __expf / __logf / powf: gated at max(8 x the fp32 restatement of the same formula, 1)
    on S of prompt_ref.ce_focal. The reduced loss adds B roundings of the row-order sum; the mix entry
    point adds the two lam products and their sum to each element (4 roundings of |ref|).
    Every value must be finite; a saturated row under focal with gamma > 0 has loss and dlogits
    exactly 0 (before focal_terms the second term there was inf * 0 = NaN for gamma < 1).
    gamma = 0 without alpha is bitwise the plain CE call; grad=False gives bitwise the same losses.
    Measured on MI355X, worst restatement / kernel ratio per C: 1: 0 / 0 (every value exact), 2: 0.59 / 0.59,
    63: 0.83 / 0.94, 64: 2.49 / 2.49, 65: 1.27 / 1.33, 130: 2.08 / 2.08, 1000: 1.79 / 1.79; the kernel at 0.39
    of its gate at the most, the same in the three entry points (1,848 launches)."""
    worst = [0.0, 0.0]
    for B in (1, 4, 5, 9):
        z, y, kinds = PR.logit_rows(B, C, seed=100 * C + B, first=FIRST[B])
        sat = torch.tensor([k == "saturated" for k in kinds])
        alpha = torch.rand(C, generator=torch.Generator().manual_seed(C)) + 0.5
        alpha[int(y[0]) if C > 1 else 0] = 0.0
        for red in ("mean", "sum"):
            gs = 1.0 / B if red == "mean" else 1.0
            ce_out = {}
            for focal, gamma, al in [(False, 2.0, None)] + [(True, gm, a) for gm in GAMMAS for a in (None, alpha)]:
                tag = f"C={C} B={B} {red} focal={int(focal)} gamma={gamma} alpha={'y' if al is not None else 'n'}"
                rl, rd, sl, sd = PR.ce_focal(z, y, al, gamma, focal, gs)
                l32, d32 = PR.ce_focal_naive(z, y, al, gamma, focal, gs)
                r = max(_ratio(l32, rl, sl), _ratio(d32, rd, sd))
                gate = max(8 * r, 1.0)
                unit_l, unit_d = U * (sl + rl.abs()), U * (sd + rd.abs())
                tot_ref = rl.sum() * gs
                for entry in ("rows", "reduce", "mix"):
                    row, tot, dl = _loss_raw(dev, entry, z, y, al, gamma, focal, red)
                    assert bool(torch.isfinite(row).all()) and bool(torch.isfinite(dl).all()), (tag, entry, kinds)
                    extra = 4.0 if entry == "mix" else 0.0
                    el = (row[:B].double() - rl).abs()
                    ed = (dl.double() - rd).abs()
                    kl = float(((el - extra * U * rl.abs()).clamp_min(0) / unit_l.clamp_min(1e-300)).max())
                    kd = float(((ed - extra * U * rd.abs()).clamp_min(0) / unit_d.clamp_min(1e-300)).max())
                    k = max(kl, kd)
                    worst = [max(worst[0], r), max(worst[1], k)]
                    print(f"{entry} {tag}: restatement ratio {r:.3f}, kernel ratio {k:.3f}, gate {gate:.3f}")
                    assert k <= gate, (tag, entry, k, r)
                    if entry == "mix":
                        assert torch.equal(row[B:], row[:B])
                    if focal and gamma > 0 and bool(sat.any()):
                        assert bool((row[:B][sat] == 0).all()) and bool((dl[sat] == 0).all()), (tag, entry)
                    if tot is not None:
                        bound = gs * (gate * float(unit_l.sum()) + (B + 1 + extra) * U * float(rl.abs().sum())) \
                            + U * abs(float(tot_ref))
                        assert abs(float(tot) - float(tot_ref)) <= bound, (tag, entry, float(tot), float(tot_ref))
                    # grad=False: the same losses, bit for bit, and no dlogits written
                    row0, tot0, _ = _loss_raw(dev, entry, z, y, al, gamma, focal, red, grad=False)
                    assert torch.equal(row0, row) and (tot is None or torch.equal(tot0, tot)), (tag, entry)
                    if not focal:
                        ce_out[entry] = (row, tot, dl)
                    elif gamma == 0.0 and al is None:  # focal with gamma 0: bitwise the CE call
                        cr, ct, cd = ce_out[entry]
                        assert torch.equal(row, cr) and torch.equal(dl, cd), (tag, entry)
                        assert tot is None or torch.equal(tot, ct), (tag, entry)
    print(f"ce / focal C={C}: worst restatement ratio {worst[0]:.3f}, worst kernel ratio {worst[1]:.3f}")


def test_ce_focal_wrappers_saturated(dev):
    """The ops wrappers on a saturated batch with gamma 0.5: finite, exactly zero (was NaN)."""
    ops, N = _mods()
    z, y, _ = PR.logit_rows(4, 37, seed=5, first=3)
    z[:, :] = z[0]
    y[:] = y[0]
    zd, yd = z.to(dev), y.to(dev)
    row, dl = ops.ce_loss(zd, yd, None, 0.5, True)
    loss, dl2 = ops.ce_loss_reduce(zd, yd, None, 0.5, True)
    loss3, dl3 = ops.ce_loss_mix(zd, yd, yd, 0.3, None, 0.5, True)
    for t in (row, dl, loss, dl2, loss3, dl3):
        assert bool((t == 0).all())


def test_focal_negative_gamma_rejected(dev):
    """focal with gamma < 0 or NaN: CLIPK_EINVAL (-1) from the three entry points, nothing written; the
    wrappers raise before the call. Without focal the gamma is not read."""
    ops, N = _mods()
    B, C = 4, 5
    z, y, _ = PR.logit_rows(B, C, seed=1)
    zd, yd = z.to(dev), y.to(dev)
    st = ops._stream()
    for gamma in (-0.5, float("nan")):
        br, row = _canary(2 * B, dev)
        bt, tot = _canary(1, dev)
        bd, dl = _canary(B * C, dev)
        _rejected(-1, lambda: N.call("clipk_ce_loss", B, C, _P(zd), _P(yd), None, gamma, 1, 1.0, _P(row), _P(dl), st),
                  br, bt, bd)
        _rejected(-1, lambda: N.call("clipk_ce_loss_reduce", B, C, _P(zd), _P(yd), None, gamma, 1, 1.0, 1, _P(row),
                                     _P(tot), _P(dl), st), br, bt, bd)
        _rejected(-1, lambda: N.call("clipk_ce_loss_mix", B, C, _P(zd), _P(yd), _P(yd), 0.5, None, gamma, 1, 1.0, 1,
                                     _P(row), _P(tot), _P(dl), st), br, bt, bd)
        for fn in (lambda: ops.ce_loss(zd, yd, None, gamma, True), lambda: ops.ce_loss_reduce(zd, yd, None, gamma, True),
                   lambda: ops.ce_loss_mix(zd, yd, yd, 0.5, None, gamma, True)):
            with pytest.raises(N.ClipkError, match="gamma >= 0"):
                fn()
    row, dl = ops.ce_loss(zd, yd, None, -1.0, False)
    row2, dl2 = ops.ce_loss(zd, yd, None, 2.0, False)
    assert torch.equal(row, row2) and torch.equal(dl, dl2)


# ================================================================ Meta-Net
def _meta_case(B, V, Hd, Wd, seed, b1_shift=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g)
    w1, b1 = torch.randn(Hd, V, generator=g) * V ** -0.5, torch.randn(Hd, generator=g) * 0.1 + b1_shift
    w2, b2 = torch.randn(Wd, Hd, generator=g) * Hd ** -0.5, torch.randn(Wd, generator=g) * 0.1
    return x, w1, b1, w2, b2


def _meta_fwd(dev, x_dev, w1, b1, w2, b2):
    ops, N = _mods()
    B, V = x_dev.shape
    Hd, Wd = w1.shape[0], w2.shape[0]
    bh, h = _canary(B * Hd, dev)
    by, y = _canary(B * Wd, dev)
    k = _Keep(dev)
    N.call("clipk_meta_net_fwd", B, V, Hd, Wd, _P(x_dev), k(w1), k(b1), k(w2), k(b2), _P(h), _P(y), ops._stream())
    torch.cuda.synchronize()
    assert _edges_ok(bh, B * Hd) and _edges_ok(by, B * Wd)
    return h.cpu().view(B, Hd), y.cpu().view(B, Wd)


def _meta_check(tag, x, w1, b1, w2, b2, h, y):
    """h: ceil(V / 64) products per lane (an fma each, or a product and an add), 6 butterfly steps, + b1:
    A_h = 2 ceil(V / 64) + 7. y: at most Hd products in one chain (the generic path; the fast path
    splits them over 4 lanes and adds 2 steps) + b2: A_y = 2 Hd + 3, and h's own error reaches y through
    |w2| (relu is 1-Lipschitz): |err y| <= u (A_y S_y + A_h S_h |w2|^T) + u |y|.
    Measured on MI355X: h at 0.41 (0.03 of A_h) at the most, y at 0.012 of its bound; the backward's dh
    0.38, dw2 0.54, db2 0.40 (A = 2 B: 0.23 of it at the most), dw1 0.14 and db1 0.07 of their bounds."""
    V, Hd = x.shape[1], w1.shape[0]
    _, rh, ry, s_h, s_y, s_yh = PR.meta_net(x, w1, b1, w2, b2)
    A_h, A_y = 2 * ((V + 63) // 64) + 7, 2 * Hd + 3
    _gate(f"meta h {tag}", h, rh, s_h, A=A_h)
    _gate(f"meta y {tag}", y, ry, A_y * s_y + A_h * s_yh, A=1)


@pytest.mark.parametrize("B,V,Hd,Wd", [(1, 512, 32, 512), (3, 512, 3, 65), (2, 1024, 64, 1), (2, 256, 65, 65),
                                       (1, 256, 3, 1)])
def test_meta_net_shapes(dev, B, V, Hd, Wd):
    """Hd = 3 (waves idle), 64 at V = 1024 (all 16 register slots of the fast path), 65 at V = 256 (the
    generic path); Wd = 1 and 65 (one output, one past a 64-output block); B = 1."""
    x, w1, b1, w2, b2 = _meta_case(B, V, Hd, Wd, seed=V + Hd + Wd)
    h, y = _meta_fwd(dev, x.to(dev), w1, b1, w2, b2)
    _meta_check(f"B={B} V={V} Hd={Hd} Wd={Wd}", x, w1, b1, w2, b2, h, y)


def test_meta_net_unaligned_x_falls_back(dev):
    """A contiguous x one float into a larger buffer (4 bytes off 16-byte alignment) at V = 512: the
    float4 fast path must not take it; the result stays within the bound of the aligned call."""
    B, V, Hd, Wd = 2, 512, 32, 512
    x, w1, b1, w2, b2 = _meta_case(B, V, Hd, Wd, seed=3)
    big = torch.zeros(B * V + 8, device=dev)
    xv = big[1:1 + B * V].view(B, V)
    xv.copy_(x.to(dev))
    assert xv.is_contiguous() and xv.data_ptr() % 16 == 4
    h, y = _meta_fwd(dev, xv, w1, b1, w2, b2)
    _meta_check("unaligned x", x, w1, b1, w2, b2, h, y)
    from fsp_amd import ops
    h2, y2 = ops.meta_net(xv, w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev))  # (arguments live through the call)
    assert torch.equal(h2.cpu(), h) and torch.equal(y2.cpu(), y)


@pytest.mark.parametrize("B,V,Hd,Wd", [(1, 512, 32, 65), (3, 256, 65, 1), (2, 96, 6, 80)])
def test_meta_net_bwd_dead_units(dev, B, V, Hd, Wd):
    """Backward with every other hidden unit driven to exactly 0 by b1 = -1e4: dh and the dw1 row
    of a dead unit are exactly 0, db1 too. The rest against fp64, h as the kernel's forward gave it:
        dh: ceil(Wd / 64) products per lane + 6 steps -> A = 2 ceil(Wd / 64) + 6
        dw2 / db2: B products in one chain -> A = 2 B
        dw1 / db1: 2 B of their own, and dh's error through |x|."""
    ops, N = _mods()
    x, w1, b1, w2, b2 = _meta_case(B, V, Hd, Wd, seed=B + V)
    b1[::2] = -1e4
    xd = x.to(dev)
    h, _ = _meta_fwd(dev, xd, w1, b1, w2, b2)
    dead = torch.zeros(Hd, dtype=torch.bool)
    dead[::2] = True
    assert bool((h[:, dead] == 0).all()) and bool((h[:, ~dead] != 0).any())
    dy = torch.randn(B, Wd, generator=torch.Generator().manual_seed(7))
    outs = {n: _canary(k, dev) for n, k in (("dw1", Hd * V), ("db1", Hd), ("dw2", Wd * Hd), ("db2", Wd), ("dh", B * Hd))}
    k = _Keep(dev)
    N.call("clipk_meta_net_bwd", B, V, Hd, Wd, _P(xd), k(h), k(w2), k(dy),
           *[_P(outs[n][1]) for n in ("dw1", "db1", "dw2", "db2", "dh")], ops._stream())
    torch.cuda.synchronize()
    for n, (buf, body) in outs.items():
        assert _edges_ok(buf, body.numel()), n
    got = {"dw1": outs["dw1"][1].cpu().view(Hd, V), "db1": outs["db1"][1].cpu(), "dw2": outs["dw2"][1].cpu().view(Wd, Hd),
           "db2": outs["db2"][1].cpu(), "dh": outs["dh"][1].cpu().view(B, Hd)}
    assert bool((got["dh"][:, dead] == 0).all()) and bool((got["dw1"][dead] == 0).all())
    assert bool((got["db1"][dead] == 0).all()) and bool((got["dw2"][:, dead] == 0).all())
    ref = PR.meta_net_bwd(x, h, w2, dy)
    A_dh = 2 * ((Wd + 63) // 64) + 6
    tag = f"B={B} V={V} Hd={Hd} Wd={Wd}"
    _gate(f"meta bwd dh {tag}", got["dh"], *ref["dh"], A=A_dh)
    _gate(f"meta bwd dw2 {tag}", got["dw2"], *ref["dw2"], A=2 * B)
    _gate(f"meta bwd db2 {tag}", got["db2"], *ref["db2"], A=2 * B)
    for n in ("dw1", "db1"):
        v, s_own, s_dh = ref[n]
        _gate(f"meta bwd {n} {tag}", got[n], v, 2 * B * s_own + A_dh * s_dh, A=1)
    d = ops.meta_net_bwd(xd, h.to(dev), w2.to(dev), dy.to(dev), V, Hd, Wd)
    for a, n in zip(d, ("dw1", "db1", "dw2", "db2")):
        assert torch.equal(a.cpu().view(got[n].shape), got[n]), n


# ================================================================ wrapper argument checks
def test_wrappers_refuse_bad_tensors(dev):
    """cosine_logits, cosine_logits_bwd, meta_net, meta_net_bwd, prompt_assemble, ctx_grad, sgd_step and
    cast: a CPU tensor, a wrong dtype and a non-contiguous slice each raise ClipkError naming the
    argument, before the library is called (a sliced matrix was read as if dense, an fp16 tensor as
    fp32)."""
    ops, N = _mods()
    B, C, E, V, Hd, Wd, W, L, n_ctx = 2, 3, 8, 16, 4, 8, 8, 10, 4
    f = lambda *s: torch.randn(*s, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    calls = {
        "cosine_logits": (lambda a: ops.cosine_logits(a[0], a[1], 1.0, 0, C), [f(B, E), f(C, E)]),
        "cosine_logits_bwd": (lambda a: ops.cosine_logits_bwd(a[0], a[1], a[2], a[3], a[4], 1.0, 0),
                              [f(B, E), f(C, E), f(C), f(B), f(B, C)]),
        "meta_net": (lambda a: ops.meta_net(*a), [f(B, V), f(Hd, V), f(Hd), f(Wd, Hd), f(Wd)]),
        "meta_net_bwd": (lambda a: ops.meta_net_bwd(a[0], a[1], a[2], a[3], V, Hd, Wd),
                         [f(B, V), f(B, Hd), f(Wd, Hd), f(B, Wd)]),
        "prompt_assemble": (lambda a: ops.prompt_assemble(B, C, L, a[0], a[1], a[2], 0, 0, a[3], a[4]),
                            [i32(C, L), f(C, 77, W), f(n_ctx, W), f(B, W), f(77, W)]),
        "ctx_grad": (lambda a: ops.ctx_grad(B, C, L, W, n_ctx, 0, a[0], a[1]), [i32(C, n_ctx), f(B * C * L, W)]),
        "sgd_step": (lambda a: ops.sgd_step(a[0], a[1], a[2], 0.1, 0.9, 0.0, 0), [f(32), f(32), f(32)]),
        "cast": (lambda a: ops.cast(a[0], torch.float16), [f(32)]),
    }
    for name, (fn, args) in calls.items():
        fn(list(args))  # the well-formed call passes
        torch.cuda.synchronize()
        for k, t in enumerate(args):
            wrong = torch.float16 if t.dtype == torch.float32 else torch.int64
            twice = torch.cat([t, t], -1) if t.dim() else t
            bad = {"must be a CUDA": t.cpu(), "must be torch": t.to(wrong),
                   "must be contiguous": twice[..., ::2] if t.dim() else None}
            for msg, b in bad.items():
                if b is None:
                    continue
                assert msg != "must be contiguous" or not b.is_contiguous()
                a2 = list(args)
                a2[k] = b
                with pytest.raises(N.ClipkError, match=msg):
                    fn(a2)
    with pytest.raises(N.ClipkError, match="one size"):
        ops.sgd_step(f(32), f(16), f(32), 0.1, 0.9, 0.0, 0)
    with pytest.raises(N.ClipkError, match="cast"):
        ops.cast(f(32), torch.float64)
