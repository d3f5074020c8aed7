"""CLIPK_PREFIX_SPLIT: the fp32 shared-prefix attention on the 16-bit MFMA (every operand as fp16
hi / lo parts, every product hi.hi + hi.lo + lo.hi, fp32 accumulation; attn_prefix_fwd_split /
attn_prefix_bwd_split). Held to the fp32 kernel tolerance TOL[torch.float32] = 2e-5 of max |ref|:
the three-term scheme's own error is ~4e-7 (fp64 emulation), so the bar leaves ~50x room and
fails if the lo parts are lost anywhere."""
import functools
import math

import numpy as np
import pytest
import torch

from fsp_amd import ops, _native as N
from test_kernels_gpu import TOL, attn_prefix_ref, close, prefix_case
from test_split_w16_gpu import _w16, split_form

pytestmark = pytest.mark.gpu

F32 = torch.float32
SPLIT = N.PREFIX_SPLIT
# (G, C, P, H, max_q): P at its maximum; classes that fill a 16-row tile; one-row classes with a
# nearly empty last tile; several chunks per (group, head) with more units per wave than one
SHAPES = [(2, 37, 5, 8, 6), (1, 19, 16, 2, 7), (3, 16, 2, 4, 16), (2, 3, 9, 2, 1), (1, 120, 5, 2, 7)]


@functools.lru_cache(maxsize=None)
def _case(G, C, P, H, max_q):
    """Inputs, the reference (computed once per shape) and the flagged kernels' outputs."""
    dev = torch.device("cuda")
    R, tiles, row_first, off, qlen, g = prefix_case(G, C, P, H, max_q, seed=G * 100 + C + P)
    W = H * 64
    qkv = torch.randn(G * R, 3 * W, generator=g).to(dev)
    dout = torch.randn(G * R, W, generator=g).to(dev)
    tiles, row_first = tiles.to(dev), row_first.to(dev)
    q32 = qkv.clone().requires_grad_(True)
    ro, rl = attn_prefix_ref(q32, G, C, P, R, off, qlen, H)
    (ro * dout).sum().backward()
    a = (G, P, R, tiles, row_first, H)
    o, lse = ops.attention_prefix(qkv, *a, lse=True, flags=SPLIT)
    d = ops.attention_prefix_bwd(qkv, o, dout, lse, *a, F32, flags=SPLIT)
    return dict(a=a, W=W, R=R, qkv=qkv, dout=dout, ro=ro.detach(), rl=rl.detach(), rgrad=q32.grad, o=o, lse=lse,
                d=d, g=g)


def _parts(W):
    return (("dq", slice(0, W)), ("dk", slice(W, 2 * W)), ("dv", slice(2 * W, 3 * W)))


@pytest.mark.parametrize("G,C,P,H,max_q", SHAPES)
def test_split_parity_vs_reference(dev, G, C, P, H, max_q):
    c = _case(G, C, P, H, max_q)
    close(c["o"], c["ro"], F32, "split prefix attn out")
    close(c["lse"], c["rl"], F32, "split prefix attn lse")
    for part, sl in _parts(c["W"]):
        close(c["d"][:, sl], c["rgrad"][:, sl], F32, f"split prefix attn {part}")


@pytest.mark.parametrize("G,C,P,H,max_q", SHAPES)
def test_split_agrees_with_fp32_valu_kernels(dev, G, C, P, H, max_q):
    c = _case(G, C, P, H, max_q)
    o, lse = ops.attention_prefix(c["qkv"], *c["a"], lse=True)
    d = ops.attention_prefix_bwd(c["qkv"], o, c["dout"], lse, *c["a"], F32)
    close(c["o"], o, F32, "out vs the fp32 kernel")
    close(c["lse"], lse, F32, "lse vs the fp32 kernel")
    for part, sl in _parts(c["W"]):
        close(c["d"][:, sl], d[:, sl], F32, f"{part} vs the fp32 kernel")


@pytest.mark.parametrize("G,C,P,H,max_q", SHAPES)
def test_split_presplit_output(dev, G, C, P, H, max_q):
    """grad dtype CLIPK_F32S: the stored dq|dk|dv (the prefix rows' reduced dK / dV included) are
    bitwise split_form of the fp32-output flagged backward's, and the qkv input-grad GEMM on them
    (CLIPK_A_SPLIT) equals the GEMM on the fp32 values."""
    c = _case(G, C, P, H, max_q)
    ds = ops.attention_prefix_bwd(c["qkv"], c["o"], c["dout"], c["lse"], *c["a"], F32, split=True, flags=SPLIT)
    assert torch.equal(ds.view(torch.int32), split_form(c["d"]).view(torch.int32))
    W = c["W"]
    w = _w16((W, 3 * W), torch.Generator().manual_seed(5), 1 / math.sqrt(3 * W)).to(dev)
    wh = ops.split_hi16(ops.split_pack(w))
    assert torch.equal(ops.gemm(ds, wh, N.EPI_NONE | N.A_SPLIT), ops.gemm(c["d"], wh, N.EPI_NONE))


def test_split_cls_group0(dev):
    """With CLIPK_PREFIX_CLS_GROUP0 the flagged calls, on a qkv whose other groups' class rows hold
    NaN, equal bitwise the plain flagged calls on the copied qkv."""
    G, C, P, H, max_q = 3, 37, 5, 8, 6
    R, tiles, row_first, off, qlen, g = prefix_case(G, C, P, H, max_q, seed=G * 100 + C + P + 7)
    W = H * 64
    qkv = torch.randn(G * R, 3 * W, generator=g).to(dev)
    for gg in range(1, G):
        qkv[gg * R + P:(gg + 1) * R] = qkv[P:R]
    hole = qkv.clone()
    for gg in range(1, G):
        hole[gg * R + P:(gg + 1) * R] = float("nan")
    a = (G, P, R, tiles.to(dev), row_first.to(dev), H)
    o, lse = ops.attention_prefix(qkv, *a, lse=True, flags=SPLIT)
    o2, lse2 = ops.attention_prefix(hole, *a, lse=True, flags=SPLIT | N.PREFIX_CLS_GROUP0)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    dout = torch.randn(G * R, W, generator=g).to(dev)
    for split in (False, True):
        d1 = ops.attention_prefix_bwd(qkv, o, dout, lse, *a, F32, split=split, flags=SPLIT)
        d2 = ops.attention_prefix_bwd(hole, o, dout, lse, *a, F32, split=split, flags=SPLIT | N.PREFIX_CLS_GROUP0)
        assert torch.equal(d1.view(torch.int32), d2.view(torch.int32))


def test_split_deterministic_and_ofwd_unread(dev):
    c = _case(1, 120, 5, 2, 7)
    d2 = ops.attention_prefix_bwd(c["qkv"], c["o"], c["dout"], c["lse"], *c["a"], F32, flags=SPLIT)
    assert torch.equal(c["d"], d2)
    nan_o = torch.full_like(c["o"], float("nan"))
    d3 = ops.attention_prefix_bwd(c["qkv"], nan_o, c["dout"], c["lse"], *c["a"], F32, flags=SPLIT)
    assert torch.equal(c["d"], d3)


def test_split_flag_refused_on_16bit(dev):
    """The flag with a 16-bit dtype is CLIPK_EINVAL (-1), forward and backward, before any launch."""
    c = _case(2, 3, 9, 2, 1)
    G, P, R, tiles, row_first, H = c["a"]
    W, lib, p = c["W"], N.load(), ops._p
    nt = tiles.numel() // 2
    nb = lib.clipk_attention_prefix_ws_bytes(G, nt, H)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    for dt, did in ((torch.float16, N.F16), (torch.bfloat16, N.BF16)):
        qkv, dout = c["qkv"].to(dt), c["dout"].to(dt)
        o = torch.zeros(G * R, W, device=dev, dtype=dt)
        dq = torch.zeros(G * R, 3 * W, device=dev, dtype=dt)
        assert lib.clipk_attention_prefix_fwd_ex(did, G, P, R, nt, p(tiles), p(row_first), H, p(qkv), 3 * W, p(o), W,
                                                 p(c["lse"]), SPLIT, ops._stream()) == -1
        assert lib.clipk_attention_prefix_bwd_ex(did, did, G, P, R, nt, p(tiles), p(row_first), H, p(qkv), 3 * W,
                                                 p(o), W, p(dout), W, p(c["lse"]), p(dq), 3 * W, p(ws), nb, SPLIT,
                                                 ops._stream()) == -1
    # fp32 q|k|v with a 16-bit grad dtype
    dq = torch.zeros(G * R, 3 * W, device=dev, dtype=torch.float16)
    assert lib.clipk_attention_prefix_bwd_ex(N.F32, N.F16, G, P, R, nt, p(tiles), p(row_first), H, p(c["qkv"]), 3 * W,
                                             p(c["o"]), W, p(c["dout"].half()), W, p(c["lse"]), p(dq), 3 * W, p(ws),
                                             nb, SPLIT, ops._stream()) == -1


def test_encoder_fp32s_text_uses_split_attention(dev, monkeypatch):
    """A small fp32s CoCoOp step (ViT-B/32, 6 classes, 2 images; packed text rows) through the
    encoder: the fp32 parity gates against the CPU oracle, and agreement with the same step on the
    exact-fp32 VALU attention kernels (CLIPK_PREFIX_SPLIT_ATTN=0) to the fp32 kernel tolerance."""
    from parity_util import run_native, rel_err
    from test_parity_gpu import _cocoop_oracle
    arch, n_cls, B = "ViT-B/32", 6, 2
    meta = {"arch": arch, "n_cls": n_cls, "batch": B, "n_ctx": 4, "ctx_init": "a photo of a", "focal": 0}
    ref = _cocoop_oracle(arch, n_cls, B)
    run = lambda: run_native(meta, {"ctx0": ref["ctx0"], "tokenized": None}, "fp32s", cocoop=True, dev=str(dev))
    monkeypatch.delenv("CLIPK_PREFIX_SPLIT_ATTN", raising=False)
    out = run()
    monkeypatch.setenv("CLIPK_PREFIX_SPLIT_ATTN", "0")
    base = run()
    assert out["packed"] and base["packed"]
    assert not np.array_equal(out["grad_ctx"], base["grad_ctx"]), "the knob selects different attention kernels"
    grads = [k for k in ref if k.startswith("grad_")]
    assert float(np.abs(out["logits"] - ref["logits"]).max()) <= 1e-3
    assert abs(out["loss"] - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))
    for k in grads:
        assert rel_err(out[k], ref[k]) <= 1e-3, k
    for k in ["logits"] + grads:
        close(torch.from_numpy(np.asarray(out[k])), torch.from_numpy(np.asarray(base[k])), F32, f"{k} vs VALU attention")
