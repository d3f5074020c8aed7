"""ViT attention forward A/B (HIP events, isolated launches): the step's shapes -- B/16 at 8
images (L 197, 12 heads), L/14@336 at 8 images (L 577, 16 heads), B/16 eval at 100 images --
for the kernel the library picks (attn_fwd_mfma_t). Prints us per launch and the fraction of the HBM roofline for the
algorithmic bytes (read q|k|v, write o, 16-bit).

    AB_MODE=fp32s python tools/vit_attn_ab.py

PREC fp32s: the flagged call (CLIPK_ATTN_SPLIT, attn_fwd_split) against the unflagged one (attn_fwd_f32)
on fp32 q|k|v, and the flagged call storing the pre-split o (CLIPK_ATTN_OUT_SPLIT). Each launch reads the
next of a ring of q|k|v buffers larger than the last-level cache (rotated buffers) and writes a
preallocated o through the C ABI. AB_REPEATS (3) interleaved repeats; a repeat times AB_BATCHES (7)
batches of AB_ITERS (20) launches per variant and prints the median batch mean with the batches' range."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsp_amd import ops, _native as N  # noqa: E402
from tools.kbench import timeit  # noqa: E402


def main():
    dev = torch.device("cuda")
    tag = os.environ.get("AB_TAG", "fwd")
    for nseq, L, H in ((8, 197, 12), (8, 577, 16), (100, 197, 12), (8, 50, 12)):
        g = torch.Generator(device="cpu").manual_seed(L)
        qkv = torch.randn(nseq * L, 3 * H * 64, generator=g).to(dev, torch.float16)
        t = timeit(lambda: ops.attention(qkv, nseq, L, H, 0), iters=20)
        byt = nseq * L * 4 * H * 64 * 2
        fl = 4.0 * nseq * H * L * L * 64
        print(f"{tag} nseq {nseq:4d} L {L:4d} H {H:3d}: {t * 1e3:7.1f} us  {byt / t / 1e6:7.1f} GB/s  "
              f"{fl / t / 1e9:6.1f} TF/s")


def main_fp32s():
    dev = torch.device("cuda")
    lib, p, st = N.load(), ops._p, ops._stream()
    repeats = int(os.environ.get("AB_REPEATS", 3))
    batches, iters = int(os.environ.get("AB_BATCHES", 7)), int(os.environ.get("AB_ITERS", 20))
    ring_bytes = int(os.environ.get("AB_RING_MB", 600)) << 20
    variants = (("f32", 0), ("split", N.ATTN_SPLIT), ("split+osplit", N.ATTN_SPLIT | N.ATTN_OUT_SPLIT))
    for nseq, L, H in ((8, 197, 12), (100, 197, 12), (8, 577, 16), (100, 50, 12)):
        W = H * 64
        one = nseq * L * 3 * W * 4
        nbuf = max(3, min(32, -(-ring_bytes // one)))
        g = torch.Generator(device="cpu").manual_seed(L)
        ring = [torch.randn(nseq * L, 3 * W, generator=g).to(dev) for _ in range(nbuf)]
        o = torch.empty(nseq * L, W, device=dev)
        state = {"i": 0}

        def batch(flags):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                q = ring[state["i"] % nbuf]
                state["i"] += 1
                N.check(lib.clipk_attention_fwd_ex(N.F32, nseq, L, H, 0, p(q), 3 * W, p(o), W, None, flags, st),
                        "clipk_attention_fwd_ex")
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) / iters * 1e3

        for _, fl in variants:
            batch(fl)
        for r in range(repeats):
            row = []
            for name, fl in variants:
                t = [batch(fl) for _ in range(batches)]
                row.append(f"{name} {statistics.median(t):7.1f} us [{min(t):.1f} .. {max(t):.1f}]")
            print(f"fp32s nseq {nseq:4d} L {L:4d} H {H:3d} ring {nbuf:2d} repeat {r}: " + "  ".join(row), flush=True)


if __name__ == "__main__":
    main_fp32s() if os.environ.get("AB_MODE") == "fp32s" else main()
