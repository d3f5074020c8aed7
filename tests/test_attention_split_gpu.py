"""CLIPK_ATTN_SPLIT / CLIPK_ATTN_OUT_SPLIT (clipk_attention_fwd_ex): the fp32 attention forward with its
products on the 16-bit MFMA as fp16 hi / lo parts (attn_fwd_split), against the fp32 reference
tests/test_kernels_gpu.py uses for clipk_attention_fwd and against the exact-fp32 kernel, at the fp32
kernels' bar (2e-5 of max |ref|; the three-term scheme's own error is ~4e-7, so a lost lo part fails
it). Head dim 64. The shapes cover the smallest L on the kernel, a masked tail in one chunk, a second
chunk / second query block of one row (causal and not), plain text, and the ViT lengths 197 / 257 / 577."""
import functools
import math

import pytest
import torch

from fsp_amd import ops, _native as N
from test_kernels_gpu import TOL, attn_ref, close
from test_split_w16_gpu import split_form

pytestmark = pytest.mark.gpu

F32 = torch.float32
SPLIT, OSPLIT = N.ATTN_SPLIT, N.ATTN_OUT_SPLIT
SHAPES = [(2, 17, 2, 0), (2, 50, 2, 0), (1, 65, 2, 0), (1, 65, 2, 1), (2, 77, 8, 1), (1, 197, 12, 0), (1, 257, 2, 0),
          (1, 577, 2, 0)]


@functools.lru_cache(maxsize=None)
def _case(nseq, L, H, causal):
    """One seeded case, computed once: qkv, the reference, the flagged and the unflagged results."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1000 * L + 10 * H + causal)
    qkv = torch.randn(nseq * L, 3 * H * 64, generator=g).to(dev)
    ro, rl = attn_ref(qkv, nseq, L, H, causal)
    o, lse = ops.attention(qkv, nseq, L, H, causal, lse=True, flags=SPLIT)
    eo, el = ops.attention(qkv, nseq, L, H, causal, lse=True)
    return {"qkv": qkv, "ro": ro, "rl": rl, "o": o, "lse": lse, "eo": eo, "el": el}


@pytest.mark.parametrize("nseq,L,H,causal", SHAPES)
def test_parity_with_reference(dev, nseq, L, H, causal):
    c = _case(nseq, L, H, causal)
    assert torch.isfinite(c["o"]).all() and torch.isfinite(c["lse"]).all()
    for k, r in (("o", "ro"), ("lse", "rl")):
        print(f"split attn {k} vs ref {(nseq, L, H, causal)}:",
              float((c[k] - c[r]).abs().max() / c[r].abs().max()), "bar", TOL[F32])
    close(c["o"], c["ro"], F32, "split attn out")
    close(c["lse"], c["rl"], F32, "split attn lse")


@pytest.mark.parametrize("nseq,L,H,causal", SHAPES)
def test_agrees_with_exact_kernel(dev, nseq, L, H, causal):
    c = _case(nseq, L, H, causal)
    close(c["o"], c["eo"], F32, "split vs exact out")
    close(c["lse"], c["el"], F32, "split vs exact lse")
    assert not torch.equal(c["o"], c["eo"]), "the flag selects another kernel"


@pytest.mark.parametrize("nseq,L,H,causal", SHAPES)
def test_deterministic(dev, nseq, L, H, causal):
    c = _case(nseq, L, H, causal)
    o2, l2 = ops.attention(c["qkv"], nseq, L, H, causal, lse=True, flags=SPLIT)
    assert torch.equal(o2, c["o"]) and torch.equal(l2, c["lse"])


@pytest.mark.parametrize("nseq,L,H,causal", SHAPES)
def test_masked_rows_never_read(dev, nseq, L, H, causal):
    """Query rows >= L of the last block and keys >= L belong to the neighbouring sequences: with those
    rows NaN (before the first and after the last sequence) the result is bitwise unchanged."""
    c = _case(nseq, L, H, causal)
    pad = torch.full((L, 3 * H * 64), float("nan"), device=dev)
    buf = torch.cat([pad, c["qkv"], pad])
    mid = buf[L:(nseq + 1) * L]
    assert mid.is_contiguous() and mid.data_ptr() == buf.data_ptr() + L * buf.shape[1] * 4
    o, lse = ops.attention(mid, nseq, L, H, causal, lse=True, flags=SPLIT)
    assert torch.equal(o, c["o"]) and torch.equal(lse, c["lse"])
    if nseq > 1:  # ... and a NaN sequence in the same call reaches no other sequence
        q2 = c["qkv"].clone()
        q2[:L] = float("nan")
        o2, l2 = ops.attention(q2, nseq, L, H, causal, lse=True, flags=SPLIT)
        assert torch.equal(o2[L:], c["o"][L:]) and torch.equal(l2[L:], c["lse"][L:])


@pytest.mark.parametrize("nseq,L,H,causal", SHAPES)
def test_presplit_o_is_the_parts_of_fp32_o(dev, nseq, L, H, causal):
    c = _case(nseq, L, H, causal)
    W = H * 64
    os_, lse_s = ops.attention(c["qkv"], nseq, L, H, causal, lse=True, flags=SPLIT | OSPLIT)
    assert torch.equal(lse_s, c["lse"]), "lse moved"
    want, got = split_form(c["o"]).view(torch.int32), os_.view(torch.int32)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} words differ"
    lo = split_form(c["o"]).view(torch.float16).view(nseq * L, W // 8, 2, 8)[:, :, 1]
    assert int((lo != 0).sum()) > lo.numel() // 2, "the lo parts carry bits"
    g = torch.Generator().manual_seed(7)
    w = ops.split_pack((torch.randn(256, W, generator=g) / math.sqrt(W)).to(dev))
    y1 = ops.gemm(c["o"], w, N.EPI_NONE)
    y2 = ops.gemm(os_, w, N.EPI_NONE | N.A_SPLIT)
    assert torch.isfinite(y1).all() and torch.equal(y1, y2)


def test_flags_refused(dev):
    """A flag with a 16-bit dtype, OUT_SPLIT without SPLIT, an unknown bit, OUT_SPLIT with rows that do
    not hold whole 8-column groups (and at L <= 16, where the exact short kernel runs): CLIPK_EINVAL
    (-1), and the output buffers are untouched."""
    nseq, L, H = 2, 50, 2
    W = H * 64
    qkv = _case(nseq, L, H, 0)["qkv"]
    lib, p, st = N.load(), ops._p, ops._stream()
    o = torch.full((nseq * L, W + 4), 7.0, device=dev)
    lse = torch.full((nseq * L, H), 7.0, device=dev)
    fwd = lambda did, q, ldo, flags, Lx=L: lib.clipk_attention_fwd_ex(did, nseq, Lx, H, 0, p(q), 3 * W, p(o), ldo,
                                                                      p(lse), flags, st)
    for dt, did in ((torch.float16, N.F16), (torch.bfloat16, N.BF16)):
        for fl in (SPLIT, OSPLIT, SPLIT | OSPLIT):
            assert fwd(did, qkv.to(dt), W, fl) == -1
    assert fwd(N.F32, qkv, W, OSPLIT) == -1
    assert fwd(N.F32, qkv, W, 4) == -1
    assert fwd(N.F32, qkv, W, SPLIT | 8) == -1
    assert fwd(N.F32, qkv, W + 4, SPLIT | OSPLIT) == -1
    assert fwd(N.F32, qkv, W, SPLIT | OSPLIT, 16) == -1
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((lse == 7.0).all()), "a refused call launched"
    assert fwd(N.F32, qkv, W, SPLIT | OSPLIT) == 0


def test_short_rows_run_the_exact_kernel(dev):
    """L <= 16: the flagged call is the unflagged one (the exact short kernel), bitwise."""
    nseq, L, H = 3, 16, 2
    qkv = torch.randn(nseq * L, 3 * H * 64, generator=torch.Generator().manual_seed(16)).to(dev)
    a = ops.attention(qkv, nseq, L, H, 1, lse=True, flags=SPLIT)
    b = ops.attention(qkv, nseq, L, H, 1, lse=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
