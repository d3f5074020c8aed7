"""CLIPK_PREFIX_OUT_SPLIT: the split prefix attention forward stores o in the pre-split operand form
(fp16 hi / lo parts per 8 columns) that out_proj reads with CLIPK_A_SPLIT. The parts must be bitwise
those of the fp32 o the same kernel stores without the flag (hi = fp16(o), lo = fp16(o - hi)), lse
must not move, and the out_proj producer on the pre-split o must equal the one on the fp32 o."""
import math

import pytest
import torch

from fsp_amd import ops, _native as N
from test_split_w16_gpu import _w16, split_form

pytestmark = pytest.mark.gpu

SPLIT, OSPLIT, CLS0 = N.PREFIX_SPLIT, N.PREFIX_OUT_SPLIT, N.PREFIX_CLS_GROUP0
G, P, H, QLEN = 2, 5, 8, (1, 6, 11)


def _case(dev):
    from fsp_amd.trainers.prompt_base import attention_tiles
    qlen = torch.tensor(QLEN)
    off = P + torch.cat([torch.zeros(1, dtype=torch.long), qlen.cumsum(0)[:-1]])
    R = int(P + qlen.sum())
    tiles, row_first = attention_tiles(off.numpy(), qlen.numpy(), R)
    tiles = torch.from_numpy(tiles.reshape(-1).copy()).to(dev)
    row_first = torch.from_numpy(row_first).to(dev)
    g = torch.Generator().manual_seed(1611)
    W = H * 64
    # magnitudes over several binades, so o's lo parts carry bits
    qkv = (torch.randn(G * R, 3 * W, generator=g) * torch.exp2(torch.randint(-3, 3, (G * R, 1), generator=g).float()))
    for gg in range(1, G):  # the class rows enter every group with group 0's values (CLS_GROUP0's premise)
        qkv[gg * R + P:(gg + 1) * R] = qkv[P:R]
    return R, W, tiles, row_first, qkv.to(dev)


@pytest.mark.parametrize("cls0", [0, CLS0])
def test_presplit_o_is_the_parts_of_fp32_o(dev, cls0):
    R, W, tiles, row_first, qkv = _case(dev)
    a = (G, P, R, tiles, row_first, H)
    o, lse = ops.attention_prefix(qkv, *a, lse=True, flags=SPLIT | cls0)
    os_, lse_s = ops.attention_prefix(qkv, *a, lse=True, flags=SPLIT | OSPLIT | cls0)
    assert torch.isfinite(o).all() and float(o.abs().max()) > 0
    assert torch.equal(lse_s, lse), "lse moved"
    want = split_form(o).view(torch.int32)
    got = os_.view(torch.int32)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} words differ"
    lo = split_form(o).view(torch.float16).view(G * R, W // 8, 2, 8)[:, :, 1]
    assert int((lo != 0).sum()) > lo.numel() // 2, "the lo parts carry bits"
    # out_proj (the LayerNorm-statistics producer with the next fold's pre-split A) on either form
    g = torch.Generator().manual_seed(7)
    wh = ops.split_hi16(ops.split_pack(_w16((W, W), g, 1 / math.sqrt(W)).to(dev)))
    bias, res = torch.randn(W, generator=g).to(dev), torch.randn(G * R, W, generator=g).to(dev)
    gamma = (1.0 + 0.2 * torch.randn(W, generator=g)).to(dev)
    st1, st2 = torch.empty(G * R, W // 64, 2, device=dev), torch.empty(G * R, W // 64, 2, device=dev)
    x1, xs1 = ops.gemm_ln_stats_split(o, wh, N.EPI_BIAS_RES, bias, st1, res, gamma)
    x2, xs2 = ops.gemm_ln_stats_split(os_, wh, N.EPI_BIAS_RES | N.A_SPLIT, bias, st2, res, gamma)
    assert torch.equal(x1, x2) and torch.equal(st1, st2) and torch.equal(xs1.view(torch.int32), xs2.view(torch.int32))


def test_out_split_flag_refused(dev):
    """Without CLIPK_PREFIX_SPLIT, with a 16-bit dtype, with rows that do not hold whole 8-column
    groups, and in the backward: CLIPK_EINVAL (-1) before any launch."""
    R, W, tiles, row_first, qkv = _case(dev)
    lib, p, st = N.load(), ops._p, ops._stream()
    nt = tiles.numel() // 2
    o = torch.zeros(G * R, W + 4, device=dev)
    lse = torch.zeros(G * R, H, device=dev)
    fwd = lambda did, q, ldo, flags: lib.clipk_attention_prefix_fwd_ex(did, G, P, R, nt, p(tiles), p(row_first), H, p(q),
                                                                     3 * W, p(o), ldo, p(lse), flags, st)
    assert fwd(N.F32, qkv, W, OSPLIT) == -1
    assert fwd(N.F32, qkv, W, OSPLIT | CLS0) == -1
    assert fwd(N.F32, qkv, W + 4, SPLIT | OSPLIT) == -1
    for dt, did in ((torch.float16, N.F16), (torch.bfloat16, N.BF16)):
        assert fwd(did, qkv.to(dt), W, OSPLIT) == -1
        assert fwd(did, qkv.to(dt), W, SPLIT | OSPLIT) == -1
    assert fwd(N.F32, qkv, W, SPLIT | OSPLIT) == 0
    nb = lib.clipk_attention_prefix_ws_bytes(G, nt, H)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    dq = torch.zeros(G * R, 3 * W, device=dev)
    dout = torch.zeros(G * R, W, device=dev)
    for fl in (OSPLIT, SPLIT | OSPLIT):
        assert lib.clipk_attention_prefix_bwd_ex(N.F32, N.F32, G, P, R, nt, p(tiles), p(row_first), H, p(qkv), 3 * W,
                                                 p(o), W, p(dout), W, p(lse), p(dq), 3 * W, p(ws), nb, fl, st) == -1
