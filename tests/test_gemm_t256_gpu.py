"""256x256 ping-pong tiles of the pre-split fp32s GEMMs (split mode 2, CLIPK_GEMM_T256).

A GEMM element accumulates the same K steps in the same order whatever the tile height, so the
256-row instantiations (the c_fc fold with and without CLIPK_QGELU_DERIV, the qkv fold; dgelu has
none: it stays on 192 rows) must give the 192-row tiles' outputs bit for bit. The same GEMMs run
in two child processes, CLIPK_GEMM_T256=2 (always 256 rows where built) and =0 (never: the
192-row launches only); the knob is read once per process. M 5,895 and 6,401 are ragged against
both heights at row counts where the tile policy already picks the ping-pong tiles for N = 1536 and
2048 (31 / 34 row tiles of 192, 24 / 26 of 256); 6,401 = 256 * 25 + 1 leaves a last 256-row tile of
one row. A's magnitudes spread over 13 binades, so both parts of the split carry bits."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

MS, NS, K = (5895, 6401), (1536, 2048), 512

_PROBE = r"""
import os, sys, math, torch
sys.path.insert(0, os.environ["FSP_ROOT"])
from fsp_amd import ops, _native as N
from fsp_amd.clip import model as M_
dev = torch.device("cuda", 0)
K = 512
lib = N.load()


def split_form(x):
    M, K = x.shape
    hi = x.half()
    lo = (x - hi.float()).half()
    return torch.stack([hi.view(M, K // 8, 8), lo.view(M, K // 8, 8)], 2).reshape(M, 2 * K).view(torch.float32)


out = {}
FC = N.EPI_BIAS_QGELU | N.A_SPLIT | N.OUT_SPLIT
for M in (5895, 6401):
    for Nn in (1536, 2048):
        g = torch.Generator(device="cpu").manual_seed(M + Nn)
        x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 7, (M, K), generator=g).float())
        w = (torch.randn(Nn, K, generator=g) / math.sqrt(K)).half().float()
        bias = torch.randn(Nn, generator=g)
        gamma = 1.0 + 0.2 * torch.randn(K, generator=g)
        beta = 0.1 * torch.randn(K, generator=g)
        wh, s, c = M_.ln_fold_weights(w, bias, gamma, beta, torch.float32, dev, split=True, gamma_on_a=True)
        mean = x.mean(1)
        rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-5)
        rnb = torch.stack([rstd, -rstd * mean], 1).contiguous().to(dev)
        gam = gamma.to(dev)
        xs = split_form((x.to(dev) * gam)).contiguous()
        fd, fdd = ops.gemm_ln_gamma(xs, wh, FC | N.QGELU_DERIV, c, s, rnb, gam, want_out2=True)
        fp, fph = ops.gemm_ln_gamma(xs, wh, FC, c, s, rnb, gam, want_out2=True)
        q = ops.gemm_ln_gamma(xs, wh, N.EPI_BIAS | N.A_SPLIT, c, s, rnb, gam)
        rows = [lib.clipk_gemm_split_tile_rows(N.F32S16, e, 4, M, Nn) for e in (FC | N.QGELU_DERIV, FC, N.EPI_BIAS | N.A_SPLIT)]
        # the 192-row answer on the fp32 A (the fold splits x * gamma itself): no 256-row form
        rows.append(lib.clipk_gemm_split_tile_rows(N.F32S16, N.EPI_BIAS, 4, M, Nn))
        out[(M, Nn)] = {"fc_deriv.out": fd.view(torch.int32).cpu(), "fc_deriv.out2": fdd.cpu(),
                        "fc.out": fp.view(torch.int32).cpu(), "fc.out2": fph.cpu(), "qkv.out": q.cpu(),
                        "rows": torch.tensor(rows)}
torch.save(out, sys.argv[1])
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path_factory.mktemp("t256")
    res = {}
    for knob in ("2", "0"):
        f = str(d / f"t256_{knob}.pt")
        env = dict(os.environ, FSP_ROOT=root, CLIPK_GEMM_T256=knob)
        p = subprocess.run([sys.executable, "-c", _PROBE, f], env=env, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        res[knob] = torch.load(f, weights_only=True)
    return res


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("Nn", NS)
def test_gemm_t256_bitwise_t192(runs, M, Nn):
    a, b = runs["2"][(M, Nn)], runs["0"][(M, Nn)]
    assert a["rows"].tolist() == [256, 256, 256, 192], "CLIPK_GEMM_T256=2: 256 rows where built"
    assert b["rows"].tolist() == [192, 192, 192, 192], "CLIPK_GEMM_T256=0: never 256 rows"
    for k in ("fc_deriv.out", "fc_deriv.out2", "fc.out", "fc.out2", "qkv.out"):
        assert a[k].shape == b[k].shape == (M, Nn)
        assert torch.equal(a[k], b[k]), f"M {M} N {Nn} {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} differ"
    # the runs computed something: finite, and not all one value
    assert torch.isfinite(a["qkv.out"]).all() and a["qkv.out"].std() > 0
