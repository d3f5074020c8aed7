"""GPU: the ModifiedResNet kernels (csrc/conv.hip) one by one against fp64 on the dtype-rounded
inputs -- the implicit-GEMM convolution (1x1 and 3x3, with the BatchNorm / residual / ReLU epilogue),
the stem's stride-2 gather, the 2x2 average pool and the attention pool.

Convolution bound, per output element:
    |err| <= K 2^-24 sum|x||w| |scale| + u |ref|
the first term for the fp32 accumulation of K products, u one rounding of the output dtype
(2^-11 fp16, 2^-8 bf16, 2^-24 fp32). Every output buffer has canary rows before and after it.
"""
import pytest
import torch
import torch.nn.functional as F

import resnet_util as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
IDS = ["fp16", "bf16", "fp32"]
GUARD = 3  # canary rows on each side


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _canary(rows, cols, dtype, dev):
    """[GUARD + rows + GUARD, cols] filled with a pattern no kernel writes; (buffer, body view)."""
    buf = torch.full((rows + 2 * GUARD, cols), -1234.5, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + rows]


def _canary_ok(buf, rows):
    edge = torch.cat([buf[:GUARD], buf[GUARD + rows:]])
    return bool((edge == -1234.5).all())


def _conv_case(dev, dtype, B, H, W, Cin, Cout, ksize, res, relu, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = _rand(g, B, H, W, Cin).to(dtype)
    w = (_rand(g, Cout, Cin, ksize, ksize) * (ksize * ksize * Cin) ** -0.5).to(dtype)
    scale = 1.0 + 0.2 * _rand(g, Cout)
    shift = 0.3 * _rand(g, Cout)
    r = _rand(g, B, H, W, Cout).to(dtype) if res else None
    return x, w, scale, shift, r


def _conv_ref(x, w, scale, shift, r, relu):
    """fp64 on the rounded inputs, NHWC out, and the bound's sum|x||w| |scale|."""
    k = w.shape[-1]
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    acc = F.conv2d(xd, wd, padding=k // 2)
    mag = F.conv2d(xd.abs(), wd.abs(), padding=k // 2) * scale.double().abs()[None, :, None, None]
    y = acc * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    y = y.permute(0, 2, 3, 1)
    if r is not None:
        y = y + r.double()
    if relu:
        y = y.clamp_min(0)
    return y, mag.permute(0, 2, 3, 1)


def _run_conv(dev, x, w, scale, shift, r, relu):
    from fsp_amd import ops
    from fsp_amd.clip.model import conv_pack
    B, H, W, _ = x.shape
    Cout, k = w.shape[0], w.shape[-1]
    buf, body = _canary(B * H * W, Cout, x.dtype, dev)
    wp = conv_pack(w.float()).to(x.dtype).to(dev)
    ops.conv2d_nhwc(x.to(dev), wp, scale.to(dev), shift.to(dev), None if r is None else r.to(dev), relu=relu,
                    ksize=k, out=body)
    torch.cuda.synchronize()
    assert _canary_ok(buf, B * H * W)
    return body.reshape(B, H, W, Cout).cpu()


def _check_conv(name, dtype, got, ref, mag, K):
    bound = K * 2.0 ** -24 * mag + U[dtype] * ref.abs()
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |err| {float(err.max()):.3e}, worst err / bound {ratio:.3f}")
    assert bool(torch.isfinite(got).all())
    assert ratio <= 1.0


CONV1 = [(2, 3, 3, 64, 64, False, True), (2, 7, 7, 256, 64, False, True), (1, 7, 7, 64, 256, True, True),
         (1, 7, 7, 64, 256, False, True), (1, 7, 7, 64, 256, False, False)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CONV1, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_conv1x1(dev, dtype, case):
    B, H, W, Cin, Cout, res, relu = case
    x, w, scale, shift, r = _conv_case(dev, dtype, B, H, W, Cin, Cout, 1, res, relu)
    ref, mag = _conv_ref(x, w, scale, shift, r, relu)
    got = _run_conv(dev, x, w, scale, shift, r, relu)
    _check_conv(f"1x1 {case} {dtype}", dtype, got, ref, mag, Cin)


CONV3 = [(2, 5, 5, 32, 32), (2, 4, 7, 64, 128), (3, 9, 9, 64, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CONV3, ids=lambda c: "x".join(map(str, c)))
def test_conv3x3(dev, dtype, case):
    B, H, W, Cin, Cout = case
    x, w, scale, shift, r = _conv_case(dev, dtype, B, H, W, Cin, Cout, 3, False, True, seed=1)
    ref, mag = _conv_ref(x, w, scale, shift, None, True)
    got = _run_conv(dev, x, w, scale, shift, None, True)
    _check_conv(f"3x3 {case} {dtype}", dtype, got, ref, mag, 9 * Cin)


# The kernel picks its tile by the grid it gives (csrc/conv.hip conv_launch): 128 x 64 when
# ceil(M / 128) * (Cout / 64) >= 512, else 128 x 32 when ceil(M / 128) * (Cout / 32) >= 512, else 64 x 32,
# which every case above takes. One case for each larger tile, M no multiple of 128:
#   1x1 (4, 63, 65, 32, 256): M = 16,380 -> 128 * 4 = 512 blocks of 128 x 64
#   3x3 (2, 127, 129, 32, 64): M = 32,766 -> 256 * 1 < 512, 256 * 2 = 512 blocks of 128 x 32
LARGE = [(4, 63, 65, 32, 256, 1), (2, 127, 129, 32, 64, 3)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", LARGE, ids=lambda c: "x".join(map(str, c)))
def test_conv_large_tiles(dev, dtype, case):
    B, H, W, Cin, Cout, k = case
    x, w, scale, shift, r = _conv_case(dev, dtype, B, H, W, Cin, Cout, k, True, True, seed=8)
    ref, mag = _conv_ref(x, w, scale, shift, r, True)
    got = _run_conv(dev, x, w, scale, shift, r, True)
    _check_conv(f"{k}x{k} {case} {dtype}", dtype, got, ref, mag, k * k * Cin)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conv3x3_impulse(dev, dtype):
    """One nonzero pixel at a corner of image 1 of 3: the output is nonzero inside that image's 3x3
    neighbourhood of the pixel only, and bitwise zero everywhere else (no cross-image halo, zero
    padding)."""
    from fsp_amd import ops
    from fsp_amd.clip.model import conv_pack
    B, H, W, Cin, Cout = 3, 5, 4, 32, 32
    g = torch.Generator().manual_seed(2)
    w = (0.5 + torch.rand(Cout, Cin, 3, 3, generator=g)).to(dtype)  # every tap nonzero, dtype-valued
    wp = conv_pack(w.float()).to(dtype).to(dev)
    bits = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}[dtype]
    for (py, px) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        x = torch.zeros(B, H, W, Cin, dtype=dtype)
        x[1, py, px, 5] = 1.0  # one channel: every output is one product, exact in any dtype
        buf, body = _canary(B * H * W, Cout, dtype, dev)
        ops.conv2d_nhwc(x.to(dev), wp, ksize=3, out=body)
        torch.cuda.synchronize()
        assert _canary_ok(buf, B * H * W)
        out = body.reshape(B, H, W, Cout).cpu()
        inside = torch.zeros(B, H, W, dtype=torch.bool)
        inside[1, max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
        assert bool((out[inside] != 0).all()), (py, px)
        assert bool((out[~inside].view(bits) == 0).all()), (py, px)
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
        assert torch.equal(out.double(), ref), (py, px)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R_", [32, 64])
def test_stem_conv(dev, dtype, R_):
    """conv1 (3 -> 32, 3x3, stride 2, pad 1) as the gather + the 1x1 path, against F.conv2d."""
    from fsp_amd import ops
    from fsp_amd.clip.model import conv_pack
    g = torch.Generator().manual_seed(3)
    B, Cout = 2, 32
    img = _rand(g, B, 3, R_, R_)
    w = (_rand(g, Cout, 3, 3, 3) * 27 ** -0.5).to(dtype)
    scale, shift = 1.0 + 0.2 * _rand(g, Cout), 0.3 * _rand(g, Cout)
    xr = img.to(dtype)  # the gather rounds the image to the act dtype
    cols = ops.im2col_3x3s2(img.to(dev), dtype)
    Ho = R_ // 2
    assert cols.shape == (B * Ho * Ho, 32) and not bool(cols[:, 27:].any())
    buf, body = _canary(B * Ho * Ho, Cout, dtype, dev)
    ops.conv2d_nhwc(cols.reshape(B, Ho, Ho, 32), conv_pack(w.float(), 32).to(dtype).to(dev), scale.to(dev),
                    shift.to(dev), relu=True, ksize=1, out=body)
    torch.cuda.synchronize()
    assert _canary_ok(buf, B * Ho * Ho)
    got = body.reshape(B, Ho, Ho, Cout).cpu()
    acc = F.conv2d(xr.double(), w.double(), stride=2, padding=1)
    mag = F.conv2d(xr.double().abs(), w.double().abs(), stride=2, padding=1) * scale.double().abs()[None, :, None, None]
    ref = (acc * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).clamp_min(0)
    _check_conv(f"stem R={R_} {dtype}", dtype, got, ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1), 27)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [(2, 4, 4, 32), (2, 6, 6, 64)], ids=lambda c: "x".join(map(str, c)))
def test_avgpool(dev, dtype, case):
    """Within one output rounding of the fp64 mean; the fp32 sum of four adds 3 roundings of the
    partial sums, each at most 2^-24 sum|x| (felt only by the fp32 output)."""
    from fsp_amd import ops
    B, H, W, C = case
    x = _rand(torch.Generator().manual_seed(4), B, H, W, C).to(dtype)
    buf, body = _canary(B * (H // 2) * (W // 2), C, dtype, dev)
    ops.avgpool2_nhwc(x.to(dev), out=body)
    torch.cuda.synchronize()
    assert _canary_ok(buf, B * (H // 2) * (W // 2))
    got = body.reshape(B, H // 2, W // 2, C).cpu().double()
    xd = x.double().permute(0, 3, 1, 2)
    ref = F.avg_pool2d(xd, 2).permute(0, 2, 3, 1)
    mag = F.avg_pool2d(xd.abs(), 2).permute(0, 2, 3, 1)
    ratio = float(((got - ref).abs() / (U[dtype] * ref.abs() + 3 * 2.0 ** -24 * mag).clamp_min(1e-300)).max())
    print(f"avgpool {case} {dtype}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("S2", [4, 9, 49])
def test_attnpool(dev, dtype, S2):
    """B = 2, C = 128 (2 heads), out 128 against the restatement in fp64 on the rounded inputs. fp32:
    max |d| <= 8 x the restatement's own fp32-vs-fp64 error + 1e-7 max |ref|; 16-bit: 1 - cos <= 5e-3."""
    from fsp_amd import ops
    g = torch.Generator().manual_seed(6)
    B, C, E, heads = 2, 128, 128, 2
    pre = "visual.attnpool."
    p = {pre + "positional_embedding": _rand(g, S2 + 1, C) * C ** -0.5}
    for n, o in (("q_proj", C), ("k_proj", C), ("v_proj", C), ("c_proj", E)):
        p[pre + n + ".weight"] = (_rand(g, o, C) * C ** -0.5).to(dtype).float()
        p[pre + n + ".bias"] = _rand(g, o) * 0.1
    x = _rand(g, B, S2, C).to(dtype)
    p64 = {k: v.double() for k, v in p.items()}
    ref = R.attnpool(p64, x.double(), heads)
    ref32 = R.attnpool(p, x.float(), heads)
    d = lambda t, dt=dtype: t.to(dt).to(dev).contiguous()
    got = ops.attnpool(x.to(dev), d(p[pre + "positional_embedding"], torch.float32), d(p[pre + "q_proj.weight"]),
                       d(p[pre + "q_proj.bias"], torch.float32),
                       d(torch.cat([p[pre + "k_proj.weight"], p[pre + "v_proj.weight"]])),
                       d(torch.cat([p[pre + "k_proj.bias"], p[pre + "v_proj.bias"]]), torch.float32),
                       d(p[pre + "c_proj.weight"]), d(p[pre + "c_proj.bias"], torch.float32), heads)
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.dtype == torch.float32 and got.shape == (B, E) and bool(torch.isfinite(got).all())
    err = float((got.double() - ref).abs().max())
    own = float((ref32.double() - ref).abs().max())
    cos = R.cos_err(got, ref)
    print(f"attnpool S2={S2} {dtype}: max |d| {err:.3e}, restatement fp32 {own:.3e} (ratio {err / own:.2f}), "
          f"1 - cos {cos:.3e}")
    if dtype == torch.float32:
        assert err <= 8 * own + 1e-7 * float(ref.abs().max())
    else:
        assert cos <= 5e-3


def _einval(fn):
    from fsp_amd import _native as N
    with pytest.raises(N.ClipkError, match=r"status -1\b"):
        fn()


def test_einval_leaves_output_untouched(dev):
    from fsp_amd import ops
    dt = torch.float16
    z = lambda *s: torch.zeros(*s, dtype=dt, device=dev)
    for Cin, Cout, k in ((48, 64, 1), (64, 16, 1), (64, 64, 5)):
        buf, body = _canary(2 * 4 * 4, Cout, dt, dev)
        _einval(lambda: ops.conv2d_nhwc(z(2, 4, 4, Cin), z(Cout, k * k * Cin), ksize=k, out=body))
        torch.cuda.synchronize()
        assert bool((buf == -1234.5).all()), (Cin, Cout, k)
    buf, body = _canary(2 * 2 * 2, 32, dt, dev)
    _einval(lambda: ops.avgpool2_nhwc(z(2, 5, 4, 32), out=body))
    torch.cuda.synchronize()
    assert bool((buf == -1234.5).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_calls_bitwise_equal(dev, dtype):
    x, w, scale, shift, r = _conv_case(dev, dtype, 3, 9, 9, 64, 64, 3, True, True, seed=7)
    a = _run_conv(dev, x, w, scale, shift, r, True)
    b = _run_conv(dev, x, w, scale, shift, r, True)
    assert torch.equal(a, b)
