"""GPU: clipk_lora_merge and clipk_lora_wgrad (csrc/lora.hip) against fp64 torch on the CPU.

Merge. out = fma(s, acc, W0), acc an fma chain over r: r + 1 roundings of partial results bounded by
|W0| + |s| sum_j |B||A|, so the fp32 output lies within (r + 2) 2^-24 (|W0| + |s| sum_j |B||A|) of
the fp64 value, elementwise. The 16-bit outputs are that fp32 value rounded once; the transposed
output is the forward one transposed (and cast), bitwise; B = 0, masked-off layers and projections
give cast(W0), bitwise.

Wgrad. Reference: tests/lora_util.wgrad_reference in fp64 on the inputs as the kernel reads them
(fp16 inputs upcast). Bound: the same composition in fp32 torch on the device is measured against
that reference; the kernel's max error may be at most 8 x that error (the margin covers another
summation order over the rows) plus an absolute floor of 1e-7 max |ref|. rows 1 (a single row), 37 (a
ragged 32-row tile), 394 (two ViT images of 197 tokens), 4099 (129 row chunks of 32: the partial
sums and the final reduction)."""
import ctypes

import pytest
import torch

from lora_util import wgrad_inputs, wgrad_reference, ln_stats

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
MASKS = [1, 5, 7]  # {q}, {q, v}, {q, k, v}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
_DEV = {}


def merge_inputs(W, r, layers=2, seed=0):
    g = torch.Generator().manual_seed(1000 * W + 10 * r + seed)
    w0 = [torch.randn(3 * W, W, generator=g) * 0.03 for _ in range(layers)]
    A = (torch.rand(layers, 3, r, W, generator=g) * 2 - 1) / W ** 0.5
    B = torch.randn(layers, 3, W, r, generator=g) * 0.05
    return w0, A, B


def run_merge(dev, w0, A, B, pm, lm, s, act, grad):
    from fsp_amd import ops
    W = w0[0].shape[1]
    out = [torch.full((3 * W, W), float("nan"), device=dev).to(act) for _ in w0]
    outT = [torch.full((W, 3 * W), float("nan"), device=dev).to(grad) for _ in w0]
    key = (id(w0[0]), id(A), id(B))
    if _DEV.get("key") != key:  # the inputs of one test go to the device once
        _DEV.update(key=key, keep=(w0, A, B), t=([w.to(dev) for w in w0], A.to(dev), B.to(dev)))
    w0d, Ad, Bd = _DEV["t"]
    ops.lora_merge(w0d, Ad, Bd, pm, lm, s, out, outT)
    return [o.cpu() for o in out], [o.cpu() for o in outT]


@pytest.mark.parametrize("r", [1, 2, 16])
@pytest.mark.parametrize("W", [64, 512, 768])
def test_merge(dev, W, r):
    w0, A, B = merge_inputs(W, r)
    lm = 0b10  # two layers, layer 0 masked off
    for pm in MASKS:
        for s in (0.5, 8.0):
            out, outT = run_merge(dev, w0, A, B, pm, lm, s, torch.float32, torch.float32)
            assert torch.equal(out[0], w0[0]), "masked-off layer"
            ref = w0[1].double().clone()
            mag = w0[1].double().abs().clone()
            for p in range(3):
                blk = slice(p * W, (p + 1) * W)
                if (pm >> p) & 1:
                    ref[blk] += s * (B[1, p].double() @ A[1, p].double())
                    mag[blk] += abs(s) * (B[1, p].double().abs() @ A[1, p].double().abs())
                else:
                    assert torch.equal(out[1][blk], w0[1][blk]), "masked-off projection"
            err = (out[1].double() - ref).abs()
            bound = (r + 2) * ULP * mag
            worst = float((err / bound).max())
            print(f"merge W {W} r {r} mask {pm} s {s}: max err / bound {worst:.3f}")
            assert worst <= 1.0
            assert float((out[1] - w0[1]).abs().max()) > 0
            for l in range(2):
                assert torch.equal(outT[l], out[l].t()), "transposed output"
            # 16-bit outputs: the fp32 result rounded once, in both layouts, any dtype pairing
            for act, grad in ((torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16),
                              (torch.float16, torch.bfloat16), (torch.float32, torch.float16)):
                o16, oT16 = run_merge(dev, w0, A, B, pm, lm, s, act, grad)
                for l in range(2):
                    assert torch.equal(o16[l], out[l].to(act)), (act, l)
                    assert torch.equal(oT16[l], out[l].t().to(grad)), (grad, l)
                    if act == grad:
                        assert torch.equal(oT16[l], o16[l].t())


@pytest.mark.parametrize("name", ["fp32", "fp16", "bf16"])
def test_merge_with_zero_b_is_the_base_weight(dev, name):
    dt = DTYPES[name]
    for W, r in ((64, 1), (512, 2), (768, 16)):
        w0, A, B = merge_inputs(W, r, seed=1)
        out, outT = run_merge(dev, w0, A, torch.zeros_like(B), 7, 0b11, 8.0, dt, dt)
        for l in range(2):
            assert torch.equal(out[l], w0[l].to(dt))
            assert torch.equal(outT[l], w0[l].t().to(dt))


def test_merge_without_transposes_and_bad_arguments(dev):
    from fsp_amd import ops, _native as N
    w0, A, B = merge_inputs(64, 2)
    w0d = [w.to(dev) for w in w0]
    out = [torch.empty(192, 64, device=dev) for _ in w0]
    ops.lora_merge(w0d, A.to(dev), B.to(dev), 7, 0b11, 0.5, out, None)
    full, _ = run_merge(dev, w0, A, B, 7, 0b11, 0.5, torch.float32, torch.float32)
    assert all(torch.equal(o.cpu(), f) for o, f in zip(out, full))
    lib = N.load()
    VP = ctypes.c_void_p * 2
    ptr = lambda ts: VP(*[t.data_ptr() for t in ts])
    Ad, Bd = A.to(dev), B.to(dev)
    for W, r in ((96, 2), (64, 17), (64, 0)):
        rc = lib.clipk_lora_merge(W, 2, r, 7, 3, 0.5, N.F32, N.F32, ptr(w0d), ops._p(Ad), ops._p(Bd), ptr(out), None,
                                  None)
        assert rc == -1, (W, r, rc)  # CLIPK_EINVAL


def _wgrad_case(dev, rows, W, r, dt, seed):
    X, gamma, beta, dY, A, B = wgrad_inputs(rows, W, r, seed)
    X, dY = X.to(dt), dY.to(dt)  # as the kernel reads them
    mean, rstd = ln_stats(X.float())
    return X, mean, rstd, gamma, beta, dY, A, B


@pytest.mark.parametrize("name", ["fp32", "fp16"])
@pytest.mark.parametrize("W", [64, 512])
@pytest.mark.parametrize("rows", [1, 37, 394, 4099])
def test_wgrad(dev, rows, W, name):
    from fsp_amd import ops
    dt = DTYPES[name]
    s = 0.5
    for r in (1, 2, 16):
        X, mean, rstd, gamma, beta, dY, A, B = _wgrad_case(dev, rows, W, r, dt, seed=rows + W + r)
        d = [t.to(dev) for t in (X, mean, rstd, gamma, beta, dY, A, B)]
        up64 = [t.double() for t in (X, mean, rstd, gamma, beta, dY, A, B)]
        up32 = [t.float() for t in d]
        for pm in MASKS:
            ref = wgrad_reference(*up64, s, pm)
            comp = wgrad_reference(*up32, s, pm)  # the same composition, fp32 torch on the device
            got = ops.lora_wgrad(*d, pm, s)
            again = ops.lora_wgrad(*d, pm, s)
            for nm, g, g2, c, r64 in zip(("dA", "dB"), got, again, comp, ref):
                assert torch.equal(g, g2), f"{nm}: two calls differ"
                e_k = float((g.double().cpu() - r64).abs().max())
                e_t = float((c.double().cpu() - r64).abs().max())
                m = float(r64.abs().max())
                print(f"wgrad rows {rows} W {W} r {r} mask {pm} {name} {nm}: kernel {e_k:.3e} torch fp32 {e_t:.3e} "
                      f"max |ref| {m:.3e}")
                assert m > 0
                assert e_k <= 8 * e_t + 1e-7 * m, (nm, e_k, e_t, m)
                for p in range(3):
                    if not (pm >> p) & 1:
                        assert not g[p].any(), f"{nm}: disabled projection {p} is not zero"


def test_wgrad_mixed_dtypes_and_given_outputs(dev):
    """The ViT's pairing (fp32 residual stream, 16-bit gradients) and bf16; outputs written into the
    caller's buffers, whatever they held."""
    from fsp_amd import ops
    rows, W, r, s, pm = 197, 128, 4, 2.0, 7
    for xdt, gdt in ((torch.float32, torch.float16), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)):
        X, gamma, beta, dY, A, B = wgrad_inputs(rows, W, r, seed=5)
        X, dY = X.to(xdt), dY.to(gdt)
        mean, rstd = ln_stats(X.float())
        ts = (X, mean, rstd, gamma, beta, dY, A, B)
        ref = wgrad_reference(*[t.double() for t in ts], s, pm)
        comp = wgrad_reference(*[t.to(dev).float() for t in ts], s, pm)
        dA = torch.full((3, r, W), float("nan"), device=dev)
        dB = torch.full((3, W, r), float("nan"), device=dev)
        ops.lora_wgrad(*[t.to(dev) for t in ts], pm, s, dA=dA, dB=dB)
        for g, c, r64 in zip((dA, dB), comp, ref):
            e_k = float((g.double().cpu() - r64).abs().max())
            e_t = float((c.double().cpu() - r64).abs().max())
            assert e_k <= 8 * e_t + 1e-7 * float(r64.abs().max()), (xdt, gdt, e_k, e_t)


def test_wgrad_refuses_unsupported_shapes(dev):
    from fsp_amd import ops, _native as N
    lib = N.load()
    X, gamma, beta, dY, A, B = wgrad_inputs(8, 128, 16, seed=2)
    mean, rstd = ln_stats(X)
    d = [t.to(dev) for t in (X, mean, rstd, gamma, beta, dY, A, B)]
    out = torch.empty(2 * 3 * 17 * 128, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)

    def call(W, r):
        return lib.clipk_lora_wgrad(N.F32, N.F32, 8, W, r, 7, 0.5, ops._p(d[0]), ops._p(d[1]), ops._p(d[2]),
                                    ops._p(d[3]), ops._p(d[4]), ops._p(d[5]), ops._p(d[6]), ops._p(d[7]), ops._p(out),
                                    ops._p(out), ops._p(ws), ws.numel(), None)

    assert call(128, 17) == -1 and call(96, 2) == -1 and call(128, 0) == -1  # CLIPK_EINVAL
    assert lib.clipk_lora_wgrad_ws_bytes(8, 128, 17) == 0 and lib.clipk_lora_wgrad_ws_bytes(8, 96, 2) == 0
    assert lib.clipk_lora_wgrad_ws_bytes(8, 128, 16) > 0
