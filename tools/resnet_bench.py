#!/usr/bin/env python3
"""ModifiedResNet timing on one MI355X (bench.py stays the headline; this is the RN50 tower's own).

forward   clipk_resnet_forward for a synthetic RN50 at each batch size and PREC and, beside it,
          alternated in one process, the same network composed from torch's own F.conv2d /
          F.batch_norm / F.avg_pool2d (channels_last, the same dtype) with the attention pool in
          torch: the outside yardstick. If torch's convolution cannot run on the box the record
          says so and only the roofline stands.
classes   every convolution of the tower timed alone (ops.conv2d_nhwc on random data of its shape,
          epilogue flags as in the tower) and summed per class -- 3x3 at each of the four map
          sizes, 1x1 reduce, 1x1 expand, downsample, stem -- with the algorithmic FLOPs
          (2 M K Cout) and bytes (x, w, out and the residual once each) against the peaks of the
          micro-architecture guide: 16-bit MFMA 2.5 PFLOP/s, f32 MFMA 157.3 TFLOP/s, HBM 8 TB/s.
          "share" is the larger of FLOPs / peak and bytes / peak over the measured time.
step      (--train-step) one CoOp train step, B = 32 images against C = 1000 class prompts, with
          RN50 and with ViT-B/16, for context.

    python tools/resnet_bench.py --batches 8 100 --precs fp16 fp32 --out profiles/resnet/rn50.json
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS = {torch.float16: 2.5e15, torch.bfloat16: 2.5e15, torch.float32: 157.3e12}
PEAK_HBM = 8.0e12


def timed(fns, iters, reps):
    """{name: ms per call (median, min, max)}: device events around `iters` calls, the variants
    alternated over `reps` repetitions, each warmed first."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / iters)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in out.items()}


def conv_list(arch, B):
    """Every convolution of one forward: (class, M, H, W, Cin, Cout, ksize, residual, relu)."""
    w, s = arch.vision_width, arch.image_resolution // 2
    out = [("stem", B * s * s, s, s, 32, w // 2, 1, False, True),
           ("stem", B * s * s, s, s, w // 2, w // 2, 3, False, True),
           ("stem", B * s * s, s, s, w // 2, w, 3, False, True)]
    s //= 2
    inpl = w
    for l, n in enumerate(arch.vision_layers):
        planes = w << l
        for i in range(n):
            out.append(("1x1 reduce", B * s * s, s, s, inpl, planes, 1, False, True))
            out.append((f"3x3 @{s}", B * s * s, s, s, planes, planes, 3, False, True))
            if l > 0 and i == 0:
                s //= 2
            if i == 0:
                out.append(("downsample", B * s * s, s, s, inpl, planes * 4, 1, False, False))
            out.append(("1x1 expand", B * s * s, s, s, planes, planes * 4, 1, True, True))
            inpl = planes * 4
    return out


def conv_work(c, esize):
    _, M, _, _, Cin, Cout, k, res, _ = c
    K = k * k * Cin
    return 2.0 * M * K * Cout, esize * (M * Cin + Cout * K + M * Cout * (2 if res else 1))


def class_times(arch, B, dtype, dev, iters, reps):
    from fsp_amd import ops
    shapes = {}
    for c in conv_list(arch, B):
        shapes[c] = shapes.get(c, 0) + 1
    esize = torch.empty((), dtype=dtype).element_size()
    rows = {}
    for c, count in shapes.items():
        cls, M, H, W, Cin, Cout, k, res, relu = c
        x = torch.randn(M // (H * W), H, W, Cin, device=dev).to(dtype)
        wt = (torch.randn(Cout, k * k * Cin, device=dev) * (k * k * Cin) ** -0.5).to(dtype)
        sc, sh = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
        r = torch.randn(M // (H * W), H, W, Cout, device=dev).to(dtype) if res else None
        out = torch.empty(M // (H * W), H, W, Cout, device=dev, dtype=dtype)
        t = timed({"conv": lambda: ops.conv2d_nhwc(x, wt, sc, sh, r, relu=relu, ksize=k, out=out)}, iters, reps)
        ms = t["conv"]["median_ms"]
        fl, by = conv_work(c, esize)
        row = rows.setdefault(cls, {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0})
        row["ms"] += ms * count
        row["flops"] += fl * count
        row["bytes"] += by * count
        row["launches"] += count
    for row in rows.values():
        sec = row["ms"] * 1e-3
        row["tflops"] = row["flops"] / sec / 1e12
        row["gbytes_per_s"] = row["bytes"] / sec / 1e9
        floor = max(row["flops"] / PEAK_FLOPS[dtype], row["bytes"] / PEAK_HBM)
        row["bound"] = "mfma" if row["flops"] / PEAK_FLOPS[dtype] >= row["bytes"] / PEAK_HBM else "hbm"
        row["share_of_roofline"] = floor / sec
    return rows


class TorchResNet:
    """The same network from torch's own operators (channels_last, one dtype)."""

    def __init__(self, sd, arch, dtype, dev):
        self.arch, self.dtype = arch, dtype
        self.p = {k: torch.as_tensor(v).to(dev, dtype) for k, v in sd.items()
                  if k.startswith("visual.") and not k.endswith("num_batches_tracked")}
        for k, v in self.p.items():
            if v.dim() == 4:
                self.p[k] = v.contiguous(memory_format=torch.channels_last)

    def bn(self, key, x):
        p = self.p
        return F.batch_norm(x, p[key + ".running_mean"], p[key + ".running_var"], p[key + ".weight"],
                            p[key + ".bias"], False, 0.0, 1e-5)

    def __call__(self, image):
        p = self.p
        x = image.to(self.dtype).contiguous(memory_format=torch.channels_last)
        for k, stride in ((1, 2), (2, 1), (3, 1)):
            x = F.relu(self.bn(f"visual.bn{k}", F.conv2d(x, p[f"visual.conv{k}.weight"], stride=stride, padding=1)))
        x = F.avg_pool2d(x, 2)
        for l, n in enumerate(self.arch.vision_layers, 1):
            for i in range(n):
                q = f"visual.layer{l}.{i}."
                stride = 2 if (l > 1 and i == 0) else 1
                o = F.relu(self.bn(q + "bn1", F.conv2d(x, p[q + "conv1.weight"])))
                o = F.relu(self.bn(q + "bn2", F.conv2d(o, p[q + "conv2.weight"], padding=1)))
                if stride > 1:
                    o = F.avg_pool2d(o, 2)
                o = self.bn(q + "bn3", F.conv2d(o, p[q + "conv3.weight"]))
                if i == 0:
                    x = F.avg_pool2d(x, 2) if stride > 1 else x
                    x = self.bn(q + "downsample.1", F.conv2d(x, p[q + "downsample.0.weight"]))
                x = F.relu(o + x)
        B, C = x.shape[:2]
        t = x.reshape(B, C, -1).permute(0, 2, 1)
        t = torch.cat([t.mean(1, keepdim=True), t], 1) + p["visual.attnpool.positional_embedding"]
        a = "visual.attnpool."
        heads = C // 64
        q = F.linear(t[:, :1], p[a + "q_proj.weight"], p[a + "q_proj.bias"]).reshape(B, 1, heads, 64).transpose(1, 2)
        k = F.linear(t, p[a + "k_proj.weight"], p[a + "k_proj.bias"]).reshape(B, -1, heads, 64).transpose(1, 2)
        v = F.linear(t, p[a + "v_proj.weight"], p[a + "v_proj.bias"]).reshape(B, -1, heads, 64).transpose(1, 2)
        o = torch.softmax((q * 0.125) @ k.transpose(-1, -2), -1, dtype=torch.float32).to(self.dtype) @ v
        return F.linear(o.transpose(1, 2).reshape(B, C), p[a + "c_proj.weight"], p[a + "c_proj.bias"]).float()


def forward_times(sd, arch, prec, B, dev, iters, reps):
    from fsp_amd.clip import synth
    from fsp_amd.clip.model import PREC_DTYPES, ResNetEncoder
    dtype = PREC_DTYPES[prec][0]
    enc = ResNetEncoder(sd, arch, prec, dev)
    img = torch.from_numpy(synth.make_images(B, arch.image_resolution, seed=1)).to(dev)
    fns = {"native": lambda: enc(img)}
    rec = {}
    try:
        tm = TorchResNet(sd, arch, dtype, dev)
        with torch.no_grad():
            ref = tm(img)
        torch.cuda.synchronize()
        got = enc(img)
        cos = 1.0 - float(F.cosine_similarity(got.double(), ref.double(), dim=-1).min())
        rec["one_minus_cos_native_vs_torch"] = cos
        fns["torch"] = lambda: tm(img)
    except Exception as e:  # torch's convolution cannot run here: the roofline stands alone
        rec["torch_error"] = f"{type(e).__name__}: {e}"[:300]
    with torch.no_grad():
        rec.update(timed(fns, iters, reps))
    flops = sum(conv_work(c, 1)[0] for c in conv_list(arch, B))
    rec["conv_tflops_native"] = flops / (rec["native"]["median_ms"] * 1e-3) / 1e12
    return rec


def train_step(backbone, prec, dev, B, C, iters, reps):
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.clip import synth
    from fsp_amd.data.synthetic import SyntheticDataManager
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    cfg = get_cfg_default()
    res = synth.ARCHS[backbone].image_resolution
    cfg.INPUT.SIZE = (res, res)
    cfg.MODEL.BACKBONE.NAME = backbone
    cfg.MODEL.SYNTH_FP16 = True
    cfg.OUTPUT_DIR = tempfile.mkdtemp(prefix="resnet_bench_")
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = B
    cfg.TRAINER.NAME = "CoOp"
    cfg.TRAINER.COOP.PREC = prec
    dm = SyntheticDataManager(C, res, B, n_batches=2, device=dev)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = TRAINER_REGISTRY.get("CoOp")(cfg, dm=dm)
    tr.num_batches, tr.batch_idx = 1 << 30, 0
    batches = dm.train_loader_x
    state = {"i": 0}

    def step():
        tr.forward_backward(batches[state["i"] & 1])
        state["i"] += 1

    return timed({"step": step}, iters, reps)["step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="RN50")
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 100])
    ap.add_argument("--precs", nargs="+", default=["fp16", "fp32"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--train-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet_bench needs the GPU: a CPU run measures nothing")
    from fsp_amd.clip import synth
    from fsp_amd.clip.model import PREC_DTYPES
    dev = torch.device("cuda:0")
    arch = synth.ARCHS[a.arch]
    sd = synth.make_state_dict(a.arch, seed=0, fp16_values=True)
    rec = {"arch": a.arch, "device": torch.cuda.get_device_name(0), "iters": a.iters, "reps": a.reps,
           "peaks": {"mfma16_flops": 2.5e15, "mfma_f32_flops": 157.3e12, "hbm_bytes_per_s": PEAK_HBM},
           "forward": {}, "classes": {}}

    def save():  # after every record: a run cut short keeps what it measured
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1, sort_keys=True)

    for prec in a.precs:
        for B in a.batches:
            key = f"{prec} B={B}"
            rec["forward"][key] = forward_times(sd, arch, prec, B, dev, a.iters, a.reps)
            rec["classes"][key] = class_times(arch, B, PREC_DTYPES[prec][0], dev, a.iters, a.reps)
            f = rec["forward"][key]
            print(key, "native", f"{f['native']['median_ms']:.3f} ms",
                  "torch", f"{f['torch']['median_ms']:.3f} ms" if "torch" in f else f.get("torch_error"), flush=True)
            for cls, row in sorted(rec["classes"][key].items()):
                print(f"  {cls:12s} {row['ms']:8.3f} ms  {row['tflops']:8.2f} TFLOP/s  {row['gbytes_per_s']:8.1f} GB/s  "
                      f"{row['bound']} share {row['share_of_roofline']:.3f}  ({row['launches']} launches)", flush=True)
            save()
    if a.train_step:
        rec["train_step"] = {}
        for prec in ("fp16", "fp32s"):
            for backbone in (a.arch, "ViT-B/16"):
                key = f"CoOp {backbone} {prec} B=32 C=1000"
                rec["train_step"][key] = train_step(backbone, prec, dev, 32, 1000, 3, 3)
                print(key, f"{rec['train_step'][key]['median_ms']:.2f} ms", flush=True)
                save()
    save()
    print(json.dumps({"ok": True, "out": a.out}))


if __name__ == "__main__":
    main()
