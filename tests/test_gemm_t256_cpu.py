"""The tile-height rule of the pre-split fp32s GEMMs (clipk_gemm_split_tile_rows, no GPU): 256 rows
where (tiles on the busiest CU) x (measured cost of a 256-row tile over a 192-row one) is smaller
than the 192-row count, for the classes built at 256 rows; every other class answers 192. The
query runs in a child process with CLIPK_GEMM_T256 unset (the knob is read once per process)."""
import json
import os
import subprocess
import sys

from fsp_amd import _native as N

CUS = 256  # MI355X; also the library's answer where no device is visible
SHAPES = [(47160, 2048), (47160, 512), (589500, 512), (589500, 2048), (5895, 2048), (47160, 1536), (589500, 1536)]
FC = N.EPI_BIAS_QGELU | N.A_SPLIT | N.OUT_SPLIT
BUILT = {"fc_deriv": (N.F32S16, FC | N.QGELU_DERIV, 4), "fc": (N.F32S16, FC, 4),
         "qkv": (N.F32S16, N.EPI_BIAS | N.A_SPLIT, 4)}
NOT_BUILT = {"dgelu": (N.F32S16, N.EPI_DQGELU | N.QGELU_DERIV | N.A_SPLIT | N.OUT_SPLIT, 0),
             "fc_dx": (N.F32S16, N.EPI_NONE | N.A_SPLIT, 0),
             "c_proj producer": (N.F32S16, N.EPI_BIAS_RES | N.A_SPLIT, 1),
             "qkv fold, A split in the loop": (N.F32S16, N.EPI_BIAS, 4),
             "c_fc fold, fp32-valued weights": (N.F32S, FC | N.QGELU_DERIV, 4),
             "W'-fold": (N.F32S16, N.EPI_BIAS_QGELU | N.OUT_SPLIT, 2)}

_PROBE = r"""
import json, os, sys
sys.path.insert(0, os.environ["FSP_ROOT"])
from fsp_amd import _native as N
lib = N.load()
q = json.loads(sys.argv[1])
print(json.dumps({k: {"cost": lib.clipk_gemm_t256_cost(*c),
                      "rows": [lib.clipk_gemm_split_tile_rows(c[0], c[1], c[2], M, n) for M, n in q["shapes"]]}
                  for k, c in q["classes"].items()}))
"""


def _busiest(M, Nn, bm):
    tiles = -(-M // bm) * (Nn // 256)
    grid = min(-(-tiles // 8) * 8, CUS // 8 * 8)  # the persistent ping-pong grid
    return -(-tiles // grid)


def _query(knob=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "CLIPK_GEMM_T256"}
    env["FSP_ROOT"] = root
    if knob is not None:
        env["CLIPK_GEMM_T256"] = knob
    arg = json.dumps({"shapes": SHAPES, "classes": {**BUILT, **NOT_BUILT}})
    p = subprocess.run([sys.executable, "-c", _PROBE, arg], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_t256_rule_arithmetic():
    r = _query()
    for name in BUILT:
        c = r[name]["cost"]
        assert c >= 1.0, f"{name}: a 256-row tile holds 4/3 the work of a 192-row one, cost {c}"
        for (M, Nn), rows in zip(SHAPES, r[name]["rows"]):
            want = 256 if _busiest(M, Nn, 256) * c < _busiest(M, Nn, 192) else 192
            assert rows == want, f"{name} at ({M}, {Nn}): {rows}, the rule gives {want} (cost {c})"
    # one tile per CU at either height: nothing to gain from fewer, dearer tiles
    assert r["fc_deriv"]["rows"][SHAPES.index((5895, 2048))] == 192
    assert r["fc"]["cost"] == r["fc_deriv"]["cost"]


def test_t256_classes_not_built_answer_192():
    for knob in (None, "2"):
        r = _query(knob)
        for name in NOT_BUILT:
            assert r[name]["cost"] == 0.0, name
            assert r[name]["rows"] == [192] * len(SHAPES), f"{name} (knob {knob}): {r[name]['rows']}"


def test_t256_knob_off_and_forced():
    off, on = _query("0"), _query("2")
    for name in BUILT:
        assert off[name]["rows"] == [192] * len(SHAPES)
        assert on[name]["rows"] == [256] * len(SHAPES)
