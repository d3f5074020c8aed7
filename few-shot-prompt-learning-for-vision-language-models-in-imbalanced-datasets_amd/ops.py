"""Tensor-level wrappers over the C-ABI: torch tensors in, device pointers + the
current HIP stream out. torch is plumbing here (allocation, streams); every op's
arithmetic runs in libclipk.so. Inputs are validated on the host and errors map to
``ClipkError`` (RuntimeError) naming the op and status, mirroring the reference's
Python exceptions at module level.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as N

DT = {torch.float32: N.F32, torch.float16: N.F16, torch.bfloat16: N.BF16}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _need(t, name, dtype=None, cuda=True):
    if t is None:
        raise N.ClipkError(f"{name} is required")
    if cuda and not t.is_cuda:
        raise N.ClipkError(f"{name} must be a CUDA(HIP) tensor; no CPU path exists")
    if dtype is not None and t.dtype != dtype:
        raise N.ClipkError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise N.ClipkError(f"{name} must be contiguous")
    return t


def split_pack(w, out=None):
    """clipk_split_pack: fp32 weight [N, K] -> its split-fp16 packing for PREC fp32s
    (SPLIT_SCALE * w as fp16 hi + lo parts, 4 bytes per element; int32 storage [N, K]; ``out``:
    an existing packing to overwrite)."""
    _need(w, "W", torch.float32)
    n, k = w.shape
    if k % 32:
        raise N.ClipkError(f"split_pack needs K % 32 == 0, got {k}")
    if out is None:
        out = torch.empty(n, k, dtype=torch.int32, device=w.device)
    elif _need(out, "out", torch.int32).shape != w.shape:
        raise N.ClipkError("split_pack: out must have W's shape")
    # the library checks |W| < 65504 / SPLIT_SCALE itself (CLIPK_ERANGE)
    N.call("clipk_split_pack", n, k, _p(w), k, _p(out), _stream())
    return out


def split_lo_zero(packed) -> bool:
    """clipk_split_lo_zero: whether every lo part of a split_pack(...) weight is zero (the weight
    is fp16-valued, so split_hi16 compacts it for CLIPK_F32S16). Synchronises the stream."""
    _need(packed, "packed", torch.int32)
    n, k = packed.shape
    res = ctypes.c_int(-1)
    N.call("clipk_split_lo_zero", n, k, _p(packed), ctypes.byref(res), _stream())
    if res.value not in (0, 1):
        raise N.ClipkError(f"clipk_split_lo_zero: no answer ({res.value})")
    return res.value == 1


def split_hi16(packed):
    """clipk_split_hi16: the CLIPK_F32S16 B operand of an fp16-valued split_pack(...) weight -- fp16
    [N, K] = SPLIT_SCALE * W exactly (2 B per element). Raises (CLIPK_ERANGE) when W is not
    fp16-valued. Synchronises the stream."""
    _need(packed, "packed", torch.int32)
    n, k = packed.shape
    out = torch.empty(n, k, dtype=torch.float16, device=packed.device)
    N.call("clipk_split_hi16", n, k, _p(packed), _p(out), _stream())
    return out


def _split_kind(a, b):
    """The GEMM input type for (a, b): PREC fp32s when a is fp32 and b a split weight -- int32
    split_pack(...) (CLIPK_F32S) or fp16 split_hi16(...) (CLIPK_F32S16) -- else None."""
    if a.dtype != torch.float32:
        return None
    return {torch.int32: N.F32S, torch.float16: N.F32S16}.get(b.dtype)


def gemm(a, b, epi=N.EPI_NONE, out_dtype=torch.float32, bias=None, res=None, aux=None,
         want_out2=False, out=None):
    """out[M,N] = epi(a[M,K] @ b[N,K]^T); returns out (and out2 for EPI_BIAS_QGELU). With a
    fp32 and b a split weight: the fp32-class split-fp16 GEMM (b int32 split_pack(...):
    CLIPK_F32S; b fp16 split_hi16(...) of an fp16-valued weight: CLIPK_F32S16)."""
    _need(a, "A")
    split = _split_kind(a, b)
    _need(b, "B", b.dtype if split is not None else a.dtype)
    M, K = a.shape
    Nn = b.shape[0]
    if b.shape[1] != K:
        raise N.ClipkError(f"gemm K mismatch {tuple(a.shape)} x {tuple(b.shape)}^T")
    if out is None:
        out = torch.empty(M, Nn, device=a.device, dtype=out_dtype)
    out2 = torch.empty_like(out) if want_out2 else None
    if bias is not None:
        _need(bias, "bias", torch.float32)
    if res is not None:
        _need(res, "res", torch.float32 if out.dtype == torch.float32 else out.dtype)
    if aux is not None:
        _need(aux, "aux")
    args = (split if split is not None else DT[a.dtype], DT[out.dtype], epi, M, Nn, K, _p(a), K, _p(b), K, _p(bias),
            _p(res), Nn, _p(out), Nn, _p(out2), _p(aux), DT[aux.dtype] if aux is not None else 0, Nn)
    N.call("clipk_gemm", *args, _stream())
    return (out, out2) if want_out2 else out


def gemm_ln(a, b, epi, bias, stats=None, res=None, colsum=None, rnb=None, want_out2=False):
    """clipk_gemm_ln (include/clipk.h): 16-bit a[M,K] @ b[N,K]^T with the LayerNorm fold.
    Producer (EPI_BIAS_RES, colsum None): the statistics partials of the output are written to
    stats (fp32 [M, N/64, 2]). Fold (EPI_BIAS / EPI_BIAS_QGELU): a is the LayerNorm input x with
    per-row rnb = (rstd, -rstd * mean) (ln_stats_merge of its partials), b = W diag(gamma),
    bias = b + W beta, colsum = row sums of b. Output in a's dtype. PREC fp32s: a fp32 and b a
    split weight as in gemm (colsum summed over the packed value, see clip.model.ln_fold_weights)."""
    _need(a, "A")
    split = _split_kind(a, b)
    _need(b, "B", b.dtype if split is not None else a.dtype)
    M, K = a.shape
    Nn = b.shape[0]
    out = torch.empty(M, Nn, device=a.device, dtype=a.dtype)
    out2 = torch.empty_like(out) if want_out2 else None
    _need(bias, "bias", torch.float32)
    for t, nm in ((stats, "stats"), (colsum, "colsum"), (rnb, "rnb")):
        if t is not None:
            _need(t, nm, torch.float32)
    if res is not None:
        _need(res, "res", a.dtype)
    N.call("clipk_gemm_ln", split if split is not None else DT[a.dtype], epi, M, Nn, K, _p(a), K, _p(b), K, _p(bias),
           _p(res), Nn, _p(out), Nn, _p(out2), _p(stats), _p(colsum), _p(rnb), _stream())
    return (out, out2) if want_out2 else out


def gemm_ln_gamma(a, b, epi, bias, colsum, rnb, gamma, want_out2=False):
    """clipk_gemm_ln_gamma (PREC fp32s): the LayerNorm fold with gamma applied to A: a fp32 x,
    b = W itself as a split weight (int32 split_pack(W): CLIPK_F32S; fp16 split_hi16(...):
    CLIPK_F32S16), colsum = rowsums of W diag(gamma), bias = b + W beta, rnb = (rstd, -rstd *
    mean) per row."""
    _need(a, "A", torch.float32)
    split = _split_kind(a, b)
    if split is None:
        raise N.ClipkError(f"gemm_ln_gamma: B must be a split weight (int32 / fp16), got {b.dtype}")
    _need(b, "B", b.dtype)
    M, K = a.shape
    Nn = b.shape[0]
    out = torch.empty(M, Nn, device=a.device, dtype=torch.float32)
    out2 = torch.empty_like(out) if want_out2 else None
    for t, nm in ((bias, "bias"), (colsum, "colsum"), (rnb, "rnb"), (gamma, "gamma")):
        _need(t, nm, torch.float32)
    N.call("clipk_gemm_ln_gamma", split, epi, M, Nn, K, _p(a), K, _p(b), K, _p(bias),
           _p(out), Nn, _p(out2), _p(colsum), _p(rnb), _p(gamma), _stream())
    return (out, out2) if want_out2 else out


def gemm_ln_stats_split(a, b, epi, bias, stats, res, gamma):
    """clipk_gemm_ln_stats_split (PREC fp32s, split mode 2): the LayerNorm-statistics producer
    (EPI_BIAS_RES [| A_SPLIT], b a split_hi16 weight) that also writes the next fold's pre-split A,
    split(out * gamma). Returns (out fp32 [M, N], out2 [M, N] fp32 storage of fp16 parts)."""
    _need(a, "A", torch.float32)
    _need(b, "B", torch.float16)
    M, K = a.shape
    Nn = b.shape[0]
    out = torch.empty(M, Nn, device=a.device, dtype=torch.float32)
    out2 = torch.empty_like(out)
    for t, nm in ((bias, "bias"), (stats, "stats"), (res, "res"), (gamma, "gamma")):
        _need(t, nm, torch.float32)
    N.call("clipk_gemm_ln_stats_split", N.F32S16, epi, M, Nn, K, _p(a), K, _p(b), K, _p(bias), _p(res), Nn,
           _p(out), Nn, _p(stats), _p(gamma), _p(out2), _stream())
    return out, out2


def gemm_ln_merge(a, b, epi, bias, stats, colsum, want_out2=False):
    """clipk_gemm_ln_merge: ln_stats_merge(stats, K) then the fold gemm_ln(a, b, epi, bias,
    colsum=colsum, rnb=...), as one launch where the library covers the shape. Returns
    (out[, out2], mean, rstd, rnb); 16-bit a."""
    _need(a, "A")
    _need(b, "B", a.dtype)
    _need(stats, "stats", torch.float32)
    _need(colsum, "colsum", torch.float32)
    _need(bias, "bias", torch.float32)
    M, K = a.shape
    Nn = b.shape[0]
    out = torch.empty(M, Nn, device=a.device, dtype=a.dtype)
    out2 = torch.empty_like(out) if want_out2 else None
    mean = torch.empty(M, device=a.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    rnb = torch.empty(M, 2, device=a.device, dtype=torch.float32)
    N.call("clipk_gemm_ln_merge", DT[a.dtype], epi, M, Nn, K, _p(a), K, _p(b), K, _p(bias), _p(out), Nn, _p(out2),
           _p(stats), _p(colsum), _p(mean), _p(rstd), _p(rnb), _stream())
    return ((out, out2) if want_out2 else (out,)) + (mean, rstd, rnb)


def ln_stats_merge(stats, width):
    """clipk_ln_stats_merge: [M, width/64, 2] partials -> (mean, rstd, rnb): fp32 [M], [M], [M, 2]
    with rnb = (rstd, -rstd * mean)."""
    _need(stats, "stats", torch.float32)
    M = stats.shape[0]
    mean = torch.empty(M, device=stats.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    rnb = torch.empty(M, 2, device=stats.device, dtype=torch.float32)
    N.call("clipk_ln_stats_merge", M, width, _p(stats), _p(mean), _p(rstd), _p(rnb), _stream())
    return mean, rstd, rnb


def gemm_splitk(a, b, epi=N.EPI_NONE, out_dtype=torch.float32, bias=None, res=None, want_out2=False,
                splits=0):
    """Split-K form of gemm (fp32 partials in a workspace, deterministic slice-order sum);
    splits <= 0 picks the library's choice for the shape."""
    _need(a, "A")
    split = _split_kind(a, b)
    _need(b, "B", b.dtype if split is not None else a.dtype)
    ind = split if split is not None else DT[a.dtype]
    M, K = a.shape
    Nn = b.shape[0]
    if splits <= 0:
        splits = N.load().clipk_gemm_auto_splits(ind, M, Nn, K)
    out = torch.empty(M, Nn, device=a.device, dtype=out_dtype)
    out2 = torch.empty_like(out) if want_out2 else None
    ws = torch.empty(max(N.load().clipk_gemm_splitk_ws_bytes(M, Nn, splits), 1), dtype=torch.uint8,
                     device=a.device)
    N.call("clipk_gemm_splitk", ind, DT[out_dtype], epi, M, Nn, K, _p(a), K, _p(b), K, _p(bias),
           _p(res), Nn, _p(out), Nn, _p(out2), splits, _p(ws), ws.numel(), _stream())
    return (out, out2) if want_out2 else out


def layernorm(x, w, b, out_dtype=torch.float32, rows=None, stats=False):
    """LayerNorm over the last dim of x [R, W] (fp32 or 16-bit; optionally on gathered rows)."""
    _need(x, "x")
    R, W = x.shape
    n = R if rows is None else rows.numel()
    out = torch.empty(n, W, device=x.device, dtype=out_dtype)
    mean = torch.empty(n, device=x.device) if stats else None
    rstd = torch.empty(n, device=x.device) if stats else None
    if rows is not None:
        _need(rows, "rows", torch.int32)
    N.call("clipk_layernorm_fwd_x", DT[x.dtype], DT[out_dtype], n, W, _p(x), W, _p(rows), _p(w), _p(b), _p(out),
           W, _p(mean), _p(rstd), _stream())
    return (out, mean, rstd) if stats else out


def layernorm_bwd(dy, x, w, mean, rstd, dres=None, lp_dtype=None):
    """LayerNorm input-grad (+ dres) into fp32 dx and, with lp_dtype, a second copy dx_lp; lp_dtype
    "split": dx_lp in the pre-split operand form (CLIPK_A_SPLIT; fp32 storage of fp16 parts)."""
    _need(dy, "dy")
    R, W = dy.shape
    dx = torch.empty(R, W, device=dy.device, dtype=torch.float32)
    split = lp_dtype == "split"
    lp = (torch.empty(R, W, device=dy.device, dtype=torch.float32 if split else lp_dtype)
          if lp_dtype is not None else None)
    lpd = N.F32S if split else (DT[lp_dtype] if lp_dtype is not None else 0)
    _need(x, "x")
    N.call("clipk_layernorm_bwd_x", DT[x.dtype], DT[dy.dtype], R, W, _p(dy), W, _p(x), W, None, _p(w), _p(mean),
           _p(rstd), _p(dres), W, _p(dx), _p(lp), lpd, None, W, _stream())
    return (dx, lp) if lp is not None else dx


def layernorm_bwd_lp_(dy, x, w, mean, rstd, dres_lp, dx=None):
    """16-bit residual-gradient stream: dres_lp <- LN-input-grad(dy) + dres_lp, in place (the
    dtype of dres_lp); also into fp32 dx when given. Returns dres_lp."""
    _need(dy, "dy")
    _need(x, "x")
    _need(dres_lp, "dres_lp")
    R, W = dy.shape
    N.call("clipk_layernorm_bwd_x2", DT[x.dtype], DT[dy.dtype], R, W, _p(dy), W, _p(x), W, None, _p(w), _p(mean),
           _p(rstd), _p(dres_lp), DT[dres_lp.dtype], W, _p(dx), _p(dres_lp), DT[dres_lp.dtype], None, W, _stream())
    return dres_lp


def attention(qkv, nseq, L, heads, causal, lse=False, flags=0):
    """flags: N.ATTN_SPLIT (fp32, the products on the 16-bit MFMA as hi / lo parts) and, with it,
    N.ATTN_OUT_SPLIT (out in the pre-split form a GEMM reads with A_SPLIT)."""
    _need(qkv, "qkv")
    W = heads * 64
    out = torch.empty(nseq * L, W, device=qkv.device, dtype=qkv.dtype)
    l = torch.empty(nseq * L, heads, device=qkv.device) if lse else None
    N.call("clipk_attention_fwd_ex", DT[qkv.dtype], nseq, L, heads, int(causal), _p(qkv), 3 * W, _p(out),
           W, _p(l), int(flags), _stream())
    return (out, l) if lse else out


def attention_bwd(qkv, o, dout, lse, nseq, L, heads, causal, grad_dtype):
    W = heads * 64
    dqkv = torch.empty(nseq * L, 3 * W, device=qkv.device, dtype=grad_dtype)
    N.call("clipk_attention_bwd", DT[qkv.dtype], DT[grad_dtype], nseq, L, heads, int(causal), _p(qkv),
           3 * W, _p(o), W, _p(dout), W, _p(lse), _p(dqkv), 3 * W, _stream())
    return dqkv


def im2col(img, patch, Kp, out_dtype):
    _need(img, "image", torch.float32)
    B, _, R, _ = img.shape
    G = R // patch
    out = torch.empty(B * G * G, Kp, device=img.device, dtype=out_dtype)
    N.call("clipk_im2col", DT[out_dtype], B, R, patch, Kp, _p(img), _p(out), _stream())
    return out


def prompt_assemble(B, C, L, src_map, emb, ctx, ctx_sb, ctx_sc, bias, pos):
    _need(src_map, "src_map", torch.int32)
    for t, name in ((emb, "emb"), (ctx, "ctx"), (pos, "pos")):
        _need(t, name, torch.float32)
    if bias is not None:
        _need(bias, "bias", torch.float32)
    W = emb.shape[-1]
    x0 = torch.empty(B * C * L, W, device=emb.device, dtype=torch.float32)
    N.call("clipk_prompt_assemble", B, C, L, W, _p(src_map), _p(emb), _p(ctx), ctx_sb, ctx_sc, _p(bias),
           _p(pos), _p(x0), _stream())
    return x0


def prompt_assemble_rows(G, R, C, L, row_tab, src_map, emb, ctx, ctx_sg, ctx_sc, bias, pos):
    W = emb.shape[-1]
    x0 = torch.empty(G * R, W, device=emb.device, dtype=torch.float32)
    N.call("clipk_prompt_assemble_rows", G, R, C, L, W, _p(row_tab), _p(src_map), _p(emb), _p(ctx), ctx_sg,
           ctx_sc, _p(bias), _p(pos), _p(x0), _stream())
    return x0


def ctx_bias_grad_rows(G, R, W, n_ctx, slot_ptr, slot_rows, dx0, bias=True):
    """clipk_ctx_bias_grad_rows: (dctx [n_ctx, W] summed over the G groups, dbias [G, W] summed
    over the slots, or None)."""
    dctx = torch.empty(n_ctx, W, device=dx0.device, dtype=torch.float32)
    dbias = torch.empty(G, W, device=dx0.device, dtype=torch.float32) if bias else None
    N.call("clipk_ctx_bias_grad_rows", G, R, W, n_ctx, _p(slot_ptr), _p(slot_rows), _p(dx0), _p(dctx), _p(dbias),
           _stream())
    return dctx, dbias


def ctx_grad_rows(G, R, W, n_ctx, slot_ptr, slot_rows, dx0):
    d = torch.empty(G * n_ctx, W, device=dx0.device, dtype=torch.float32)
    N.call("clipk_ctx_grad_rows", G, R, W, n_ctx, _p(slot_ptr), _p(slot_rows), _p(dx0), _p(d), _stream())
    return d


def attention_prefix(qkv, G, P, R, tiles, row_first, heads, lse=False, flags=0):
    """Shared-prefix packed causal attention (clipk_attention_prefix_fwd_ex); tiles int32
    [ntiles*2] (first row, rows), row_first int32 [R]; flags N.PREFIX_CLS_GROUP0: class rows'
    q|k|v read from group 0; N.PREFIX_SPLIT (fp32 qkv only): the products on the 16-bit MFMA as
    fp16 hi / lo parts."""
    _need(qkv, "qkv")
    _need(tiles, "tiles", torch.int32)
    _need(row_first, "row_first", torch.int32)
    W = heads * 64
    out = torch.zeros(G * R, W, device=qkv.device, dtype=qkv.dtype)
    l = torch.zeros(G * R, heads, device=qkv.device) if lse else None
    N.call("clipk_attention_prefix_fwd_ex", DT[qkv.dtype], G, P, R, tiles.numel() // 2, _p(tiles), _p(row_first),
           heads, _p(qkv), 3 * W, _p(out), W, _p(l), int(flags), _stream())
    return (out, l) if lse else out


def attention_prefix_bwd(qkv, o, dout, lse, G, P, R, tiles, row_first, heads, grad_dtype, split=False, flags=0):
    """split (fp32 qkv / dout / grad_dtype): dq|dk|dv in the pre-split operand form of CLIPK_A_SPLIT
    (grad dtype CLIPK_F32S), viewed as fp32 [G*R, 3W]. flags as attention_prefix; with
    N.PREFIX_SPLIT (fp32 tensors only) `o` is not read."""
    W = heads * 64
    nt = tiles.numel() // 2
    dqkv = torch.zeros(G * R, 3 * W, device=qkv.device, dtype=grad_dtype)
    nb = N.load().clipk_attention_prefix_ws_bytes(G, nt, heads)
    ws = torch.empty(nb, dtype=torch.uint8, device=qkv.device)
    gdt = N.F32S if split else DT[grad_dtype]
    N.call("clipk_attention_prefix_bwd_ex", DT[qkv.dtype], gdt, G, P, R, nt, _p(tiles), _p(row_first),
           heads, _p(qkv), 3 * W, _p(o), W, _p(dout), W, _p(lse), _p(dqkv), 3 * W, _p(ws), nb, int(flags), _stream())
    return dqkv


def ctx_grad(B, C, L, W, n_ctx, csc, ctx_pos, dx0):
    _need(ctx_pos, "ctx_pos", torch.int32)
    _need(dx0, "dx0", torch.float32)
    outs = (B * C if csc else B) * n_ctx
    d = torch.empty(outs, W, device=dx0.device, dtype=torch.float32)
    N.call("clipk_ctx_grad", B, C, L, W, n_ctx, int(csc), _p(ctx_pos), _p(dx0), _p(d), _stream())
    return d


def cosine_logits(imf, txt, scale, per_image, C):
    _need(imf, "imf", torch.float32)
    _need(txt, "txt", torch.float32)
    B, E = imf.shape
    logits = torch.empty(B, C, device=imf.device)
    inv_t = torch.empty(txt.shape[0], device=imf.device)
    inv_i = torch.empty(B, device=imf.device)
    N.call("clipk_cosine_logits_fwd", B, C, E, int(per_image), float(scale), _p(imf), _p(txt),
           _p(logits), _p(inv_t), _p(inv_i), _stream())
    return logits, inv_t, inv_i


def cosine_logits_bwd(imf, txt, inv_t, inv_i, dlogits, scale, per_image):
    for t, name in ((imf, "imf"), (txt, "txt"), (inv_t, "inv_t"), (inv_i, "inv_i"), (dlogits, "dlogits")):
        _need(t, name, torch.float32)
    B, C = dlogits.shape
    E = imf.shape[1]
    dtxt = torch.empty_like(txt)
    N.call("clipk_cosine_logits_bwd", B, C, E, int(per_image), float(scale), _p(imf), _p(txt),
           _p(inv_t), _p(inv_i), _p(dlogits), _p(dtxt), _stream())
    return dtxt


def ce_loss(logits, labels, alpha=None, gamma=2.0, focal=False, grad=True, grad_scale=None):
    """Per-row CE / focal loss [B] and dlogits = grad_scale * d(row loss)/d logits (default
    grad_scale 1/B: the gradient of the mean)."""
    _need(logits, "logits", torch.float32)
    _need(labels, "labels", torch.int64)
    B, C = logits.shape
    if labels.shape != (B,):
        raise N.ClipkError(f"labels must be [{B}], got {tuple(labels.shape)}")
    if alpha is not None:
        _need(alpha, "alpha", torch.float32)
        if alpha.numel() < C:
            raise N.ClipkError(f"alpha must hold {C} class weights, got {alpha.numel()}")
    if focal and not gamma >= 0:
        raise N.ClipkError(f"focal needs gamma >= 0, got {gamma}")
    row = torch.empty(B, device=logits.device)
    dl = torch.empty_like(logits) if grad else None
    N.call("clipk_ce_loss", B, C, _p(logits), _p(labels), _p(alpha), float(gamma), int(focal),
           float(1.0 / B if grad_scale is None else grad_scale), _p(row), _p(dl), _stream())
    return row, dl


def meta_net(x, w1, b1, w2, b2, normalize=False):
    """(h, y); normalize: the Meta-Net on x / |x| (clipk_meta_net_fwd_norm) -> (xn, h, y)."""
    for t, name in ((x, "x"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")):
        _need(t, name, torch.float32)
    B, V = x.shape
    Hd, Wd = w1.shape[0], w2.shape[0]
    h = torch.empty(B, Hd, device=x.device)
    y = torch.empty(B, Wd, device=x.device)
    if normalize:
        xn = torch.empty(B, V, device=x.device)
        N.call("clipk_meta_net_fwd_norm", B, V, Hd, Wd, _p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(xn), _p(h),
               _p(y), _stream())
        return xn, h, y
    N.call("clipk_meta_net_fwd", B, V, Hd, Wd, _p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(h), _p(y),
           _stream())
    return h, y


def ce_loss_reduce(logits, labels, alpha=None, gamma=2.0, focal=False, grad=True, reduction="mean"):
    """clipk_ce_loss_reduce: (loss [] = mean / sum of the row losses, dlogits = d loss / d logits)
    in one launch."""
    _need(logits, "logits", torch.float32)
    _need(labels, "labels", torch.int64)
    B, C = logits.shape
    if labels.shape != (B,):
        raise N.ClipkError(f"labels must be [{B}], got {tuple(labels.shape)}")
    if alpha is not None:
        _need(alpha, "alpha", torch.float32)
        if alpha.numel() < C:
            raise N.ClipkError(f"alpha must hold {C} class weights, got {alpha.numel()}")
    if focal and not gamma >= 0:
        raise N.ClipkError(f"focal needs gamma >= 0, got {gamma}")
    red = {"mean": 1, "sum": 2}[reduction]
    row = torch.empty(B, device=logits.device)
    loss = torch.empty((), device=logits.device)
    dl = torch.empty_like(logits) if grad else None
    N.call("clipk_ce_loss_reduce", B, C, _p(logits), _p(labels), _p(alpha), float(gamma), int(focal),
           1.0 / B if reduction == "mean" else 1.0, red, _p(row), _p(loss), _p(dl), _stream())
    return loss, dl


def ce_loss_mix(logits, y_a, y_b, lam, alpha=None, gamma=2.0, focal=False, grad=True, reduction="mean"):
    """clipk_ce_loss_mix: the mixup criterion lam * L(logits, y_a) + (1 - lam) * L(logits, y_b)
    (L = CE / focal with its mean / sum) -> (loss [], dlogits = d loss / d logits) in one launch."""
    _need(logits, "logits", torch.float32)
    _need(y_a, "y_a", torch.int64)
    _need(y_b, "y_b", torch.int64)
    if logits.dim() != 2:
        raise N.ClipkError(f"logits must be [B, C], got {tuple(logits.shape)}")
    B, C = logits.shape
    if y_a.shape != (B,) or y_b.shape != (B,):
        raise N.ClipkError(f"y_a and y_b must be [{B}], got {tuple(y_a.shape)} and {tuple(y_b.shape)}")
    if alpha is not None:
        _need(alpha, "alpha", torch.float32)
        if alpha.numel() < C:
            raise N.ClipkError(f"alpha must hold {C} class weights, got {alpha.numel()}")
    if focal and not gamma >= 0:
        raise N.ClipkError(f"focal needs gamma >= 0, got {gamma}")
    red = {"mean": 1, "sum": 2}[reduction]
    row = torch.empty(2 * B, device=logits.device)
    loss = torch.empty((), device=logits.device)
    dl = torch.empty_like(logits) if grad else None
    N.call("clipk_ce_loss_mix", B, C, _p(logits), _p(y_a), _p(y_b), float(lam), _p(alpha), float(gamma), int(focal),
           1.0 / B if reduction == "mean" else 1.0, red, _p(row), _p(loss), _p(dl), _stream())
    return loss, dl


def mixup_images(x, perm, lam, labels=None):
    """mixup_data (independentVL.py:435-449): (lam * x + (1 - lam) * x[perm], labels[perm] or None)
    for fp32 x [B, ...]. perm: a host integer tensor [B] with entries in [0, B), checked here and
    uploaded on the current stream without a synchronisation. CUDA x: one clipk_mixup_images launch,
    bitwise the torch expression; CPU x: the torch expression itself (loader logic off device)."""
    _need(x, "x", torch.float32, cuda=False)
    if x.dim() < 1:
        raise N.ClipkError("x must be [B, ...]")
    B = x.shape[0]
    if perm is None or perm.is_cuda or perm.dtype not in (torch.int32, torch.int64):
        raise N.ClipkError("perm must be a host int32 / int64 tensor")
    if perm.shape != (B,):
        raise N.ClipkError(f"perm must be [{B}], got {tuple(perm.shape)}")
    if B and (int(perm.min()) < 0 or int(perm.max()) >= B):
        raise N.ClipkError(f"perm entries must lie in [0, {B})")
    if labels is not None:
        _need(labels, "labels", torch.int64, cuda=False)
        if labels.shape != (B,) or labels.device != x.device:
            raise N.ClipkError(f"labels must be [{B}] on x's device, got {tuple(labels.shape)} on {labels.device}")
    lam = float(lam)
    if not x.is_cuda:
        idx = perm.long()
        return lam * x + (1 - lam) * x[idx], (labels[idx] if labels is not None else None)
    out = torch.empty_like(x)
    y_b = torch.empty_like(labels) if labels is not None else None
    if B:
        if not x.numel():  # nothing to mix: the kernel wants n_per >= 1
            return out, (labels[perm.long().to(x.device)] if labels is not None else None)
        d_perm = perm.to(torch.int32).to(x.device, non_blocking=True)
        N.call("clipk_mixup_images", B, x.numel() // B, _p(x), _p(d_perm), _p(labels), _p(y_b), lam, 1.0 - lam,
               _p(out), _stream())
    return out, y_b


def ntxent_loss(a, b, temperature=0.07, grad=True, grad_scale=1.0):
    """clipk_ntxent_loss: NT-Xent of the two views a, b (fp32 [n, D]) -> (loss [], da, db) with
    da / db = grad_scale * d loss / d a, b (None when not grad). 1 <= n <= 512."""
    _need(a, "a", torch.float32)
    _need(b, "b", torch.float32)
    if a.dim() != 2 or b.shape != a.shape:
        raise N.ClipkError(f"a and b must be [n, D] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if b.device != a.device:
        raise N.ClipkError("a and b must be on one device")
    n, D = a.shape
    if not 1 <= n <= 512 or D < 1:
        raise N.ClipkError(f"ntxent_loss needs 1 <= n <= 512 and D >= 1, got n = {n}, D = {D}")
    if not temperature > 0:
        raise N.ClipkError(f"temperature must be positive, got {temperature}")
    ws = torch.empty(N.load().clipk_ntxent_ws_bytes(n, D), dtype=torch.uint8, device=a.device)
    loss = torch.empty((), device=a.device)
    da = torch.empty_like(a) if grad else None
    db = torch.empty_like(b) if grad else None
    N.call("clipk_ntxent_loss", n, D, _p(a), _p(b), float(temperature), float(grad_scale), _p(loss), _p(da), _p(db),
           _p(ws), _stream())
    return loss, da, db


SRC_HEAD_MAX_B = 128  # clipk_src_head's batch ceiling


def src_head(img, txt, zs_img, fixed_n, fixed_q, labels, alpha, gamma, focal, scale, w_text, w_image, w_logits,
             grad=True, grad_scale=1.0, want_logits=False):
    """clipk_src_head: the PromptSRC objective on the raw prompted image [B, E] / text [C, E] features,
    the raw frozen image features zs_img [B, E] and the frozen normalised text features fixed_n /
    fixed_q [C, E] (fixed_q: the fp16-valued copy of the zero-shot logits) -> (loss [5] = total, ce,
    kl, l1_text, l1_image; logits [B, C] or None; d_img, d_txt = grad_scale * d total / d img, txt,
    None when not grad). 1 <= B <= 128."""
    for t, name in ((img, "img"), (txt, "txt"), (zs_img, "zs_img"), (fixed_n, "fixed_n"), (fixed_q, "fixed_q")):
        _need(t, name, torch.float32)
        if t.dim() != 2:
            raise N.ClipkError(f"{name} must be 2-D, got {tuple(t.shape)}")
    _need(labels, "labels", torch.int64)
    B, E = img.shape
    C = txt.shape[0]
    if zs_img.shape != (B, E) or txt.shape != (C, E) or fixed_n.shape != (C, E) or fixed_q.shape != (C, E):
        raise N.ClipkError(f"src_head needs img, zs_img [B, E] and txt, fixed_n, fixed_q [C, E], got "
                           f"{[tuple(t.shape) for t in (img, zs_img, txt, fixed_n, fixed_q)]}")
    if labels.shape != (B,):
        raise N.ClipkError(f"labels must be [{B}], got {tuple(labels.shape)}")
    if not 1 <= B <= SRC_HEAD_MAX_B or C < 1 or E < 1:
        raise N.ClipkError(f"src_head needs 1 <= B <= {SRC_HEAD_MAX_B}, C >= 1 and E >= 1, got B = {B}, C = {C}, "
                           f"E = {E}")
    if alpha is not None:
        _need(alpha, "alpha", torch.float32)
        if alpha.numel() < C:
            raise N.ClipkError(f"alpha must hold {C} class weights, got {alpha.numel()}")
    if any(t.device != img.device for t in (txt, zs_img, fixed_n, fixed_q, labels) + ((alpha,) if alpha is not None
                                                                                      else ())):
        raise N.ClipkError("src_head: every tensor must be on one device")
    if not scale > 0:
        raise N.ClipkError(f"scale must be positive, got {scale}")
    if focal and not gamma >= 0:
        raise N.ClipkError(f"focal needs gamma >= 0, got {gamma}")
    ws = torch.empty(N.load().clipk_src_head_ws_bytes(B, C, E), dtype=torch.uint8, device=img.device)
    loss = torch.empty(5, device=img.device)
    logits = torch.empty(B, C, device=img.device) if want_logits else None
    d_img = torch.empty_like(img) if grad else None
    d_txt = torch.empty_like(txt) if grad else None
    N.call("clipk_src_head", B, C, E, _p(img), _p(txt), _p(zs_img), _p(fixed_n), _p(fixed_q), _p(labels), _p(alpha),
           float(gamma), int(bool(focal)), float(scale), float(w_text), float(w_image), float(w_logits),
           float(grad_scale), _p(loss), _p(logits), _p(d_img), _p(d_txt), _p(ws), _stream())
    return loss, logits, d_img, d_txt


PROBE_HEAD_MAX_B = 512  # clipk_probe_head's batch ceiling


def probe_head(feat, w, bias, labels, alpha, gamma, focal, normalize, scale, grad=True, want_logits=False,
               grad_scale=1.0):
    """clipk_probe_head: the linear probe's head on frozen image features feat [B, E] with the
    classifier w [C, E], bias [C] or None -> (loss [], logits [B, C] or None, d_w, d_bias =
    grad_scale * d loss / d w, bias; None when not grad, d_bias None without a bias).
    logits = scale * u w^T + bias with u = F.normalize(feat) when normalize, feat otherwise; loss =
    the mean CE / focal of clipk_ce_loss. labels None: scoring only -> (None, logits, None, None).
    1 <= B <= 512."""
    for t, name in ((feat, "feat"), (w, "w")):
        _need(t, name, torch.float32)
        if t.dim() != 2:
            raise N.ClipkError(f"{name} must be 2-D, got {tuple(t.shape)}")
    B, E = feat.shape
    C = w.shape[0]
    if w.shape != (C, E):
        raise N.ClipkError(f"probe_head needs feat [B, E] and w [C, E], got {tuple(feat.shape)} and {tuple(w.shape)}")
    if not 1 <= B <= PROBE_HEAD_MAX_B or C < 1 or E < 1:
        raise N.ClipkError(f"probe_head needs 1 <= B <= {PROBE_HEAD_MAX_B}, C >= 1 and E >= 1, got B = {B}, "
                           f"C = {C}, E = {E}")
    others = []
    if bias is not None:
        _need(bias, "bias", torch.float32)
        if bias.shape != (C,):
            raise N.ClipkError(f"bias must be [{C}], got {tuple(bias.shape)}")
        others.append(bias)
    if labels is not None:
        _need(labels, "labels", torch.int64)
        if labels.shape != (B,):
            raise N.ClipkError(f"labels must be [{B}], got {tuple(labels.shape)}")
        others.append(labels)
    if alpha is not None:
        _need(alpha, "alpha", torch.float32)
        if alpha.numel() < C:
            raise N.ClipkError(f"alpha must hold {C} class weights, got {alpha.numel()}")
        others.append(alpha)
    if w.device != feat.device or any(t.device != feat.device for t in others):
        raise N.ClipkError("probe_head: every tensor must be on one device")
    if not scale > 0:
        raise N.ClipkError(f"scale must be positive, got {scale}")
    if focal and not gamma >= 0:
        raise N.ClipkError(f"focal needs gamma >= 0, got {gamma}")
    dev = feat.device
    if labels is None:  # scoring only: one launch, no workspace
        logits = torch.empty(B, C, device=dev)
        N.call("clipk_probe_head", B, C, E, _p(feat), _p(w), _p(bias), None, None, 0.0, 0, int(bool(normalize)),
               float(scale), 1.0, None, _p(logits), None, None, None, _stream())
        return None, logits, None, None
    ws = torch.empty(N.load().clipk_probe_head_ws_bytes(B, C, E), dtype=torch.uint8, device=dev)
    loss = torch.empty((), device=dev)
    logits = torch.empty(B, C, device=dev) if want_logits else None
    d_w = torch.empty_like(w) if grad else None
    d_bias = torch.empty_like(bias) if grad and bias is not None else None
    N.call("clipk_probe_head", B, C, E, _p(feat), _p(w), _p(bias), _p(labels), _p(alpha), float(gamma),
           int(bool(focal)), int(bool(normalize)), float(scale), float(grad_scale), _p(loss), _p(logits), _p(d_w),
           _p(d_bias), _p(ws), _stream())
    return loss, logits, d_w, d_bias


def status_take(flags, host_word):
    """clipk_status_take: flags -> host_word (pinned int32), flags cleared (stream-ordered)."""
    N.call("clipk_status_take", _p(flags), _p(host_word), _stream())


def meta_net_bwd(x, h, w2, dy, V, Hd, Wd):
    for t, name in ((x, "x"), (h, "h"), (w2, "w2"), (dy, "dy")):
        _need(t, name, torch.float32)
    B = x.shape[0]
    dw1 = torch.empty(Hd, V, device=x.device)
    db1 = torch.empty(Hd, device=x.device)
    dw2 = torch.empty(Wd, Hd, device=x.device)
    db2 = torch.empty(Wd, device=x.device)
    dh = torch.empty(B, Hd, device=x.device)
    N.call("clipk_meta_net_bwd", B, V, Hd, Wd, _p(x), _p(h), _p(w2), _p(dy), _p(dw1),
           _p(db1), _p(dw2), _p(db2), _p(dh), _stream())
    return dw1, db1, dw2, db2


def sgd_step(p, g, buf, lr, momentum, weight_decay, has_buf):
    for t, name in ((p, "p"), (g, "g"), (buf, "buf")):
        _need(t, name, torch.float32)
    if g.numel() != p.numel() or buf.numel() != p.numel():
        raise N.ClipkError("sgd_step: p, g and buf must have one size")
    N.call("clipk_sgd_step", p.numel(), _p(p), _p(g), _p(buf), float(lr), float(momentum),
           float(weight_decay), int(has_buf), _stream())


def sgd_step_multi(ps, gs, bufs, lr, momentum, weight_decay, has_bufs, grad_scale=1.0, guard=None):
    """clipk_sgd_step_multi(_scaled / _if): one launch per 16 tensors (fp32, contiguous, on one
    device); grad_scale multiplies every gradient (1.0: the unscaled entry point); guard = (int32
    device flags, mask): the update is skipped on the device when flags[0] & mask."""
    import ctypes
    for i in range(0, len(ps), 16):
        P_, G_, B_ = ps[i:i + 16], gs[i:i + 16], bufs[i:i + 16]
        c = len(P_)
        VP = ctypes.c_void_p * c
        args = (c, VP(*[t.data_ptr() for t in P_]), VP(*[t.data_ptr() for t in G_]),
                VP(*[t.data_ptr() for t in B_]), (ctypes.c_long * c)(*[t.numel() for t in P_]),
                (ctypes.c_int * c)(*[int(h) for h in has_bufs[i:i + 16]]), float(lr), float(momentum),
                float(weight_decay))
        if guard is not None:
            N.call("clipk_sgd_step_multi_if", *args, float(grad_scale), _p(guard[0]), int(guard[1]), _stream())
        elif grad_scale == 1.0:
            N.call("clipk_sgd_step_multi", *args, _stream())
        else:
            N.call("clipk_sgd_step_multi_scaled", *args, float(grad_scale), _stream())


ADAM_MODES = {"adam": N.ADAM_ADAM, "adamw": N.ADAM_ADAMW, "amsgrad": N.ADAM_AMSGRAD}


def adam_step_multi(ps, gs, ms, vs, vmaxs, steps, parities, lr, beta1, beta2, eps, weight_decay, mode,
                    grad_scale=1.0, guard=None):
    """clipk_adam_step_multi: one launch per 16 tensors (fp32, contiguous, on one device). mode
    "adam" / "adamw" / "amsgrad" (vmaxs: the max_exp_avg_sq tensors, else None); steps[k]: the
    tensor's two int32 device step counters, parities[k] the one this call reads (the caller flips
    it afterwards); grad_scale multiplies every gradient; guard = (int32 device flags, mask): the
    update and the step count's advance are skipped on the device when flags[0] & mask."""
    amsgrad = mode == "amsgrad"
    lists = [ps, gs, ms, vs] + ([vmaxs] if amsgrad else [])
    if amsgrad and vmaxs is None:
        raise N.ClipkError("adam_step_multi: amsgrad needs the max_exp_avg_sq tensors")
    if any(len(l) != len(ps) for l in lists + [steps, parities]):
        raise N.ClipkError("adam_step_multi: lists of different lengths")
    for k, p in enumerate(ps):
        for l in lists:
            _need(l[k], "adam_step_multi tensor", torch.float32)
            if l[k].device != p.device or l[k].numel() != p.numel():
                raise N.ClipkError("adam_step_multi: a parameter's tensors differ in device or size")
        _need(steps[k], "step counters", torch.int32)
        if steps[k].numel() != 2 or steps[k].device != ps[0].device or p.device != ps[0].device:
            raise N.ClipkError("adam_step_multi: two int32 step counters per tensor, everything on one device")
    for i in range(0, len(ps), 16):
        c = len(ps[i:i + 16])
        VP = ctypes.c_void_p * c
        ptrs = [VP(*[t.data_ptr() for t in l[i:i + 16]]) for l in lists]
        if not amsgrad:
            ptrs.append(None)
        N.call("clipk_adam_step_multi", c, *ptrs, (ctypes.c_long * c)(*[t.numel() for t in ps[i:i + 16]]),
               VP(*[t.data_ptr() for t in steps[i:i + 16]]), (ctypes.c_int * c)(*parities[i:i + 16]),
               float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), ADAM_MODES[mode],
               float(grad_scale), _p(guard[0]) if guard is not None else None,
               int(guard[1]) if guard is not None else 0, _stream())


def cast(x, dtype):
    _need(x, "x", torch.float32)
    if dtype not in DT:
        raise N.ClipkError(f"cast: fp32 -> fp32 / fp16 / bf16 only, got {dtype}")
    y = torch.empty(x.shape, device=x.device, dtype=dtype)
    N.call("clipk_cast", DT[dtype], x.numel(), _p(x), _p(y), _stream())
    return y


def rows_inject(src, rows, dst, n_per):
    """dst[rows[p*n_per + i]] = src[p] (deep prompts: the rows a layer's learnable tokens
    replace, model.py:229-256); src fp32 [n_ctx, W], dst [*, W] any dtype, in place."""
    _need(src, "prompt rows", torch.float32)
    _need(rows, "row table", torch.int32)
    _need(dst, "destination")
    n_ctx, W = src.shape
    N.call("clipk_rows_inject", DT[dst.dtype], n_ctx, n_per, W, _p(src), _p(rows), _p(dst), dst.shape[-1], _stream())
    return dst


def rows_collect(src, rows, n_ctx, n_per, out=None, zero_src=True, src2=None):
    """out[p] = sum_i src[rows[p*n_per + i]] (fixed order); those rows of src (and src2) zeroed."""
    _need(src, "gradient rows")
    _need(rows, "row table", torch.int32)
    W = src.shape[-1]
    acc = out is not None
    if out is None:
        out = torch.empty(n_ctx, W, device=src.device, dtype=torch.float32)
    N.call("clipk_rows_collect", DT[src.dtype], n_ctx, n_per, W, _p(src), W, _p(src2),
           DT[src2.dtype] if src2 is not None else 0, W if src2 is not None else 0, _p(rows), _p(out), int(acc),
           int(zero_src), _stream())
    return out


LORA_PROJ_BITS = {"q": 1, "k": 2, "v": 4}  # proj_mask bits of clipk_lora_*
LORA_MAX_RANK = 16


def lora_merge(w0, A, B, proj_mask, layer_mask, scale, out, outT=None):
    """clipk_lora_merge: out[l] = W0[l] + scale * B[l] A[l] on the masked projections / layers
    (else W0[l]) and outT[l] its transpose, in one launch. w0: list of fp32 [3W, W]; A fp32
    [layers, 3, r, W]; B fp32 [layers, 3, W, r]; out / outT: lists of [3W, W] / [W, 3W] tensors
    (one dtype each: fp32, fp16 or bf16), written in place."""
    layers = len(w0)
    _need(A, "A", torch.float32)
    _need(B, "B", torch.float32)
    r, W = A.shape[-2], A.shape[-1]
    if tuple(A.shape) != (layers, 3, r, W) or tuple(B.shape) != (layers, 3, W, r):
        raise N.ClipkError(f"lora_merge: A {tuple(A.shape)} / B {tuple(B.shape)} do not match {layers} layers")
    if len(out) != layers or (outT is not None and len(outT) != layers):
        raise N.ClipkError("lora_merge: one output per layer")
    for t in w0:
        _need(t, "W0", torch.float32)
        if tuple(t.shape) != (3 * W, W):
            raise N.ClipkError(f"lora_merge: W0 must be [{3 * W}, {W}], got {tuple(t.shape)}")
    for t in out:
        _need(t, "out", out[0].dtype)
        if tuple(t.shape) != (3 * W, W):
            raise N.ClipkError(f"lora_merge: out must be [{3 * W}, {W}], got {tuple(t.shape)}")
    for t in outT or []:
        _need(t, "outT", outT[0].dtype)
        if tuple(t.shape) != (W, 3 * W):
            raise N.ClipkError(f"lora_merge: outT must be [{W}, {3 * W}], got {tuple(t.shape)}")
    VP = ctypes.c_void_p * layers
    N.call("clipk_lora_merge", W, layers, r, int(proj_mask), int(layer_mask), float(scale), DT[out[0].dtype],
           DT[outT[0].dtype] if outT else N.F32, VP(*[t.data_ptr() for t in w0]), _p(A), _p(B),
           VP(*[t.data_ptr() for t in out]), VP(*[t.data_ptr() for t in outT]) if outT else None, _stream())
    return out, outT


def lora_wgrad(x, mean, rstd, gamma, beta, dqkv, A, B, proj_mask, scale, dA=None, dB=None):
    """clipk_lora_wgrad: one layer's adapter gradients (dA [3, r, W], dB [3, W, r], fp32) from the
    layer input x [rows, W], its LayerNorm statistics and weights, and dqkv [rows, 3W]."""
    _need(x, "x")
    _need(dqkv, "dqkv")
    for t, nm in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta"), (A, "A"), (B, "B")):
        _need(t, nm, torch.float32)
    rows, W = x.shape
    r = A.shape[-2]
    if tuple(A.shape) != (3, r, W) or tuple(B.shape) != (3, W, r) or tuple(dqkv.shape) != (rows, 3 * W):
        raise N.ClipkError(f"lora_wgrad: shapes x {tuple(x.shape)}, dqkv {tuple(dqkv.shape)}, A {tuple(A.shape)}, "
                           f"B {tuple(B.shape)} do not match")
    if mean.numel() != rows or rstd.numel() != rows or gamma.numel() != W or beta.numel() != W:
        raise N.ClipkError("lora_wgrad: LayerNorm statistics / weights do not match x")
    dA = torch.empty_like(A) if dA is None else _need(dA, "dA", torch.float32)
    dB = torch.empty_like(B) if dB is None else _need(dB, "dB", torch.float32)
    wsb = N.load().clipk_lora_wgrad_ws_bytes(rows, W, r)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=x.device)
    N.call("clipk_lora_wgrad", DT[x.dtype], DT[dqkv.dtype], rows, W, r, int(proj_mask), float(scale), _p(x),
           _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dqkv), _p(A), _p(B), _p(dA), _p(dB), _p(ws), ws.numel(),
           _stream())
    return dA, dB


def encoder_set_lora(handle, rank, proj_mask=0, layer_mask=0, scale=0.0, A=None, B=None, dA=None, dB=None):
    """clipk_encoder_set_lora on an encoder handle (rank 0 clears)."""
    N.call("clipk_encoder_set_lora", handle, int(rank), int(proj_mask), int(layer_mask), float(scale), _p(A), _p(B),
           _p(dA), _p(dB))


# ---------------------------------------------------------------- ModifiedResNet kernels
def conv2d_nhwc(x, w, scale=None, shift=None, res=None, relu=False, ksize=1, out_f32=False, out=None):
    """clipk_conv2d_nhwc: x [B,H,W,Cin], w [Cout, ksize^2 Cin] (k = tap * Cin + c), both x's dtype
    -> out [B,H,W,Cout] = relu?(acc * scale + shift (+ res)) rounded once (out_f32: stored as fp32).
    Stride 1, pad ksize // 2. The library checks the shape constraints (CLIPK_EINVAL)."""
    _need(x, "x")
    _need(w, "w", x.dtype)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    if w.shape[1] != ksize * ksize * Cin:
        raise N.ClipkError(f"conv2d_nhwc: w must be [Cout, {ksize * ksize * Cin}], got {tuple(w.shape)}")
    for t, name in ((scale, "scale"), (shift, "shift")):
        if t is not None and _need(t, name, torch.float32).numel() != Cout:
            raise N.ClipkError(f"conv2d_nhwc: {name} must have Cout elements")
    odt = torch.float32 if out_f32 else x.dtype
    if out is None:
        out = torch.empty(B, H, W, Cout, dtype=odt, device=x.device)
    elif _need(out, "out", odt).numel() != B * H * W * Cout:
        raise N.ClipkError("conv2d_nhwc: out must hold B*H*W*Cout elements")
    if res is not None and _need(res, "res", x.dtype).numel() != B * H * W * Cout:
        raise N.ClipkError("conv2d_nhwc: res must have out's shape")
    flags = (N.CONV_RES if res is not None else 0) | (N.CONV_RELU if relu else 0) | (N.CONV_OUT_F32 if out_f32 else 0)
    N.call("clipk_conv2d_nhwc", DT[x.dtype], flags, B, H, W, Cin, Cout, ksize, _p(x), _p(w), _p(scale), _p(shift),
           _p(res), _p(out), _stream())
    return out


def im2col_3x3s2(img, out_dtype):
    """clipk_im2col_3x3s2: img fp32 [B,3,R,R] -> [B (R/2)^2, 32] rows of the stem's 3x3 / stride-2
    taps, k = (ky * 3 + kx) * 3 + c, zero padded from 27."""
    _need(img, "img", torch.float32)
    B, _, R, _ = img.shape
    out = torch.empty(B * (R // 2) ** 2, 32, dtype=out_dtype, device=img.device)
    N.call("clipk_im2col_3x3s2", DT[out_dtype], B, R, _p(img), _p(out), _stream())
    return out


def avgpool2_nhwc(x, out=None):
    """clipk_avgpool2_nhwc: AvgPool2d(2) of x [B,H,W,C] (fp32 sum, one rounding)."""
    _need(x, "x")
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty(B, H // 2, W // 2, C, dtype=x.dtype, device=x.device)
    else:
        _need(out, "out", x.dtype)
    N.call("clipk_avgpool2_nhwc", DT[x.dtype], B, H, W, C, _p(x), _p(out), _stream())
    return out


def attnpool(x, pos, q_w, q_b, kv_w, kv_b, c_w, c_b, heads):
    """clipk_attnpool: x [B, HW, C] -> fp32 [B, E] (AttentionPool2d: the mean token is the only
    query). kv_w [2C, C] is k_proj.weight over v_proj.weight; weights in x's dtype, pos / biases fp32."""
    _need(x, "x")
    B, HW, C = x.shape
    E = c_w.shape[0]
    for t, name in ((q_w, "q_w"), (kv_w, "kv_w"), (c_w, "c_w")):
        _need(t, name, x.dtype)
    for t, name in ((pos, "pos"), (q_b, "q_b"), (kv_b, "kv_b"), (c_b, "c_b")):
        _need(t, name, torch.float32)
    if pos.shape != (HW + 1, C) or q_w.shape != (C, C) or kv_w.shape != (2 * C, C) or c_w.shape != (E, C):
        raise N.ClipkError("attnpool: pos [HW+1, C], q_w [C, C], kv_w [2C, C], c_w [E, C] expected")
    feat = torch.empty(B, E, dtype=torch.float32, device=x.device)
    wsb = N.load().clipk_attnpool_ws_bytes(DT[x.dtype], B, HW, C)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=x.device)
    N.call("clipk_attnpool", DT[x.dtype], B, HW, C, heads, E, _p(x), _p(pos), _p(q_w), _p(q_b), _p(kv_w), _p(kv_b),
           _p(c_w), _p(c_b), _p(feat), _p(ws), ws.numel(), _stream())
    return feat
