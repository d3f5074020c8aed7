"""The fp32s text encoder with its new defaults -- o handed to out_proj pre-split (CLIPK_PRESPLIT_O)
and the 256-row split tiles by their rule (CLIPK_GEMM_T256) -- against both switched off, which is
the previous launch sequence: a packed split-mode-2 forward + backward (G = 2 groups, C = 3 classes
of 1 / 6 / 11 rows behind a 5-row prefix, the 2-layer synthetic encoder on fp16-valued weights).
Both changes are exact, so txt, the loss and dx0 on the prefix rows are compared bit for bit. Each
setting runs in a child process (CLIPK_GEMM_T256 is read once per process). The default run also
shows the hand-off is live and guarded: a backward that would read the saved o as fp32 values (the
VALU attention backward, CLIPK_PREFIX_SPLIT_ATTN=1) is refused with CLIPK_EINVAL."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

_PROBE = r"""
import os, sys, torch
sys.path.insert(0, os.environ["FSP_ROOT"])
from fsp_amd import _native as N
from fsp_amd.clip import synth, model as M
from fsp_amd.trainers.prompt_base import TextShape, attention_tiles
dev = torch.device("cuda", 0)
arch = "tiny"
a = synth.ARCHS[arch]
core = M.TextEncoderCore(synth.make_state_dict(arch, seed=0, fp16_values=True), a, "fp32s", dev)
assert core.split_mode == 2, core.split_mode
G, C, P = 2, 3, 5
qlen = torch.tensor([1, 6, 11])
off = P + torch.cat([torch.zeros(1, dtype=torch.long), qlen.cumsum(0)[:-1]])
R = int(P + qlen.sum())
tiles, row_first = attention_tiles(off.numpy(), qlen.numpy(), R)
eot = torch.tensor([g * R + int(off[c] + qlen[c]) - 1 for g in range(G) for c in range(C)], dtype=torch.int32).to(dev)
shape = TextShape(eot, G=G, C=C, P=P, R=R, tiles=torch.from_numpy(tiles.reshape(-1).copy()).to(dev),
                  row_first=torch.from_numpy(row_first).to(dev), prefix_input=True)
g = torch.Generator().manual_seed(3)
W = a.transformer_width
x0 = 0.3 * torch.randn(G * R, W, generator=g)
for gg in range(1, G):  # prefix-input mode: the class rows are the same in every group
    x0[gg * R + P:(gg + 1) * R] = x0[P:R]
x0 = x0.to(dev)
dtxt = torch.randn(G * C, a.embed_dim, generator=g).to(dev)
txt, saved = core.forward(x0, shape, save=True)
dx0 = core.backward(dtxt, shape, saved)
torch.cuda.synchronize()
prefix = torch.cat([dx0[gg * R:gg * R + P] for gg in range(G)]).cpu()
loss = (txt.double().cpu() * dtxt.double().cpu()).sum()
# a backward on the fp32 VALU attention kernels reads o: refused when the forward saved it pre-split
txt2, saved2 = core.forward(x0, shape, save=True)
os.environ["CLIPK_PREFIX_SPLIT_ATTN"] = "1"
try:
    core.backward(dtxt, shape, saved2)
    refused = ""
except N.ClipkError as e:
    refused = str(e)
torch.cuda.synchronize()
torch.save({"txt": txt.cpu(), "dx0_prefix": prefix, "loss": loss, "refused": refused}, sys.argv[1])
"""


def test_text_fp32s_new_defaults_bitwise(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for name, knobs in (("new", {}), ("old", {"CLIPK_GEMM_T256": "0", "CLIPK_PRESPLIT_O": "0"})):
        f = str(tmp_path / f"{name}.pt")
        env = {k: v for k, v in os.environ.items()
               if k not in ("CLIPK_GEMM_T256", "CLIPK_PRESPLIT_O", "CLIPK_PREFIX_SPLIT_ATTN", "CLIPK_PRESPLIT")}
        env.update(knobs, FSP_ROOT=root)
        p = subprocess.run([sys.executable, "-c", _PROBE, f], env=env, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        res[name] = torch.load(f, weights_only=True)
    new, old = res["new"], res["old"]
    assert torch.isfinite(new["txt"]).all() and torch.isfinite(new["dx0_prefix"]).all()
    assert float(new["dx0_prefix"].abs().max()) > 0
    assert torch.equal(new["txt"], old["txt"]), "txt"
    assert float(new["loss"]) == float(old["loss"]), "loss"
    assert torch.equal(new["dx0_prefix"], old["dx0_prefix"]), "dx0 on the prefix rows"
    assert "invalid argument" in new["refused"], f"pre-split o read as fp32 was not refused: {new['refused']!r}"
    assert old["refused"] == "", "an fp32 o serves the VALU backward"
