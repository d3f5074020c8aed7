"""The pre-split fp32s fold GEMMs of the headline step (split mode 2, M = 47,160 packed text rows,
K = 512) timed alone at the tile height CLIPK_GEMM_T256 selects: the c_fc fold (N = 2048,
EPI_BIAS_QGELU | QGELU_DERIV, A and out pre-split) and the qkv fold (N = 1536, EPI_BIAS, A
pre-split). HIP events, A rotated over > 600 MB so it streams from HBM as in the step. The knob is
read once per process: run once per setting, interleaved, and take the per-tile cost ratio
c(256) / c(192) = (us(256) / tiles per CU at 256) / (us(192) / tiles per CU at 192) for
kT256Cost in csrc/gemm.hip.

    CLIPK_GEMM_T256=0|2 python tools/t256_gemm_bench.py [tag]  -> one line per class"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsp_amd import ops, _native as N  # noqa: E402
from fsp_amd.clip import model as M_  # noqa: E402

M = int(os.environ.get("SGB_M", 47160))
K = 512
FC = N.EPI_BIAS_QGELU | N.QGELU_DERIV | N.A_SPLIT | N.OUT_SPLIT
CLASSES = [("fc_fwd", 2048, FC), ("qkv_fwd", 1536, N.EPI_BIAS | N.A_SPLIT)]


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "T256=" + os.environ.get("CLIPK_GEMM_T256", "unset")
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(0)
    lib = N.load()
    for name, Nn, epi in CLASSES:
        nrot = max(2, int(6e8 // (M * K * 4)) + 1)
        # pre-split A: any fp16 (hi, lo) pairs are valid operands; draw them as the parts of randn
        As = []
        for _ in range(nrot):
            x = torch.randn(M, K, device=dev)
            hi = x.half()
            lo = (x - hi.float()).half()
            As.append(torch.stack([hi.view(M, K // 8, 8), lo.view(M, K // 8, 8)], 2).reshape(M, 2 * K)
                      .view(torch.float32).contiguous())
        w = (torch.randn(Nn, K, generator=g) / math.sqrt(K)).half().float()
        gamma = 1.0 + 0.2 * torch.randn(K, generator=g)
        wh, s, c = M_.ln_fold_weights(w, torch.randn(Nn, generator=g), gamma, 0.1 * torch.randn(K, generator=g),
                                      torch.float32, dev, split=True, gamma_on_a=True)
        rnb = torch.stack([1.0 + 0.1 * torch.rand(M), 0.1 * torch.randn(M)], 1).contiguous().to(dev)
        gam = gamma.to(dev)
        out = torch.empty(M, Nn, device=dev)
        out2 = torch.empty(M, Nn, device=dev) if epi & N.QGELU_DERIV else None
        st = ops._stream()

        def run(i):
            N.call("clipk_gemm_ln_gamma", N.F32S16, epi, M, Nn, K, ops._p(As[i % nrot]), K, ops._p(wh), K, ops._p(c),
                   ops._p(out), Nn, ops._p(out2), ops._p(s), ops._p(rnb), ops._p(gam), st)
        import time
        t0 = time.time()
        while time.time() - t0 < 0.5:  # clocks settled before the first timed repeat
            for i in range(50):
                run(i)
            torch.cuda.synchronize()
        ts = []
        for _ in range(7):
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record()
            for i in range(20):
                run(i)
            e.record()
            torch.cuda.synchronize()
            ts.append(b.elapsed_time(e) / 20 * 1000)
        rows = lib.clipk_gemm_split_tile_rows(N.F32S16, epi, 4, M, Nn)
        tiles = -(-M // rows) * (Nn // 256)
        per_cu = -(-tiles // min(-(-tiles // 8) * 8, 256))
        tf = 2.0 * M * Nn * K / (min(ts) * 1e-6) / 1e12
        med = sorted(ts)[len(ts) // 2]
        print(f"{tag:10s} {name:8s} M {M} N {Nn} K {K} rows {rows} tiles/CU {per_cu}: best {min(ts):7.1f} median {med:7.1f} us "
              f"(repeats {' '.join(f'{t:.1f}' for t in ts)})  {tf:6.1f} TF/s  us/tile {min(ts) / per_cu:6.2f}", flush=True)
        del As


if __name__ == "__main__":
    main()
