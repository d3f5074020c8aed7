"""Linear-probe head: the native clipk_probe_head (NATIVE.FUSED_PROBE) against the torch composition
with autograd, and the LinearProbeCLIP step with and without the feature cache, on one GPU.

    python tools/lab/probe_head_timing.py head  [--reps 7] [--calls 200] [--out FILE.json]
        head forward + backward at (B, C, E) = (32, 1000, 512), (128, 1000, 512), (512, 1000, 512),
        (32, 1000, 768), CE and focal: the flag-off composition (F.normalize, scale * F.linear + bias,
        CrossEntropyFn, autograd) against ProbeHeadFn, us per call. Device events around `calls`
        calls ending in a synchronise, `reps` alternated repetitions, median / min / max; first the
        agreement of the two variants' loss, d_w and d_bias.
    python tools/lab/probe_head_timing.py step  [--reps 5] [--steps 10] [--prec fp16] [--out FILE.json]
        one LinearProbeCLIP train step, ViT-B/16, C = 1000, B = 32, synthetic weights: uncached with
        FUSED_PROBE off and on (image encoder + head + optimizer) and cached off and on (a batch of
        the FeatureBank: head + optimizer alone), ms per step, alternated.
    python tools/lab/probe_head_timing.py calls VARIANT B C E FOCAL CALLS
        CALLS head calls of one variant (torch | fused) and nothing else: the target of a kernel
        trace, e.g.
            rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/lab/probe_head_timing.py calls fused 32 1000 512 0 10
    python tools/lab/probe_head_timing.py count TRACE_A.csv CALLS_A TRACE_B.csv CALLS_B
        launches per call from two such traces of different CALLS (set-up launches cancel).
"""
import argparse
import contextlib
import csv
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HEAD_SHAPES = [(32, 1000, 512), (128, 1000, 512), (512, 1000, 512), (32, 1000, 768)]
SCALE = 100.0


def head_inputs(B, C, E, dev):
    """The recipe of tests/probe_util.py."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(1000003 * B + 1009 * C + E)

    def r(*shape):
        return torch.randn(*shape, dtype=torch.float64, generator=g)

    feat = (2 * r(B, E)).float()
    w = (F.normalize(r(C, E), dim=-1) * (1 + 0.1 * r(C, 1))).float()
    bias = (0.5 * r(C)).float()
    y = torch.randint(0, C, (B,), generator=g)
    alpha = (0.25 + 4 * torch.rand(C, dtype=torch.float64, generator=g)).float()
    return {"feat": feat.to(dev), "w": w.to(dev).requires_grad_(), "bias": bias.to(dev).requires_grad_(),
            "y": y.to(dev), "alpha": alpha.to(dev)}


def head_call(variant, x, focal):
    """One forward + backward of the head on the leaves w, bias (gradients overwritten)."""
    import torch.nn.functional as F
    from fsp_amd.trainers._fns import CrossEntropyFn, ProbeHeadFn
    w, bias = x["w"], x["bias"]
    w.grad = bias.grad = None
    alpha, gamma = (x["alpha"], 2.0) if focal else (None, 0.0)
    if variant == "fused":
        loss = ProbeHeadFn.apply(x["feat"], w, bias, x["y"], alpha, gamma, focal, True, SCALE)
    else:  # LinearProbeModel.logits / loss, flag off
        logits = SCALE * F.linear(F.normalize(x["feat"], dim=-1), w) + bias
        loss = CrossEntropyFn.apply(logits, x["y"], alpha, gamma, focal)
    loss.backward()
    return loss


def timed(fn, count):
    """ms of `count` calls of fn between two device events, synchronised."""
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(count):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def run_head(args, dev):
    out = {}
    for B, C, E in HEAD_SHAPES:
        for focal in (False, True):
            x = head_inputs(B, C, E, dev)
            got = {}
            for v in ("torch", "fused"):
                loss = head_call(v, x, focal)
                got[v] = (loss.detach().clone(), x["w"].grad.clone(), x["bias"].grad.clone())
            agree = {"loss_rel": rel_err(got["fused"][0], got["torch"][0]),
                     "d_w_rel": rel_err(got["fused"][1], got["torch"][1]),
                     "d_bias_rel": rel_err(got["fused"][2], got["torch"][2])}
            key = f"{B}x{C}x{E}_{'focal' if focal else 'ce'}"
            assert max(agree.values()) <= 1e-4, (key, agree)
            per = {"torch": [], "fused": []}
            for v in per:
                timed(lambda: head_call(v, x, focal), 20)  # warm-up
            for _ in range(args.reps):
                for v in per:
                    per[v].append(1000.0 * timed(lambda: head_call(v, x, focal), args.calls) / args.calls)
            out[key] = {v: spread(t) for v, t in per.items()}
            out[key]["fused_vs_torch"] = agree
            t, f = out[key]["torch"], out[key]["fused"]
            print(f"head fwd+bwd {key} us/call: torch {t['median']:.1f} [{t['min']:.1f}, {t['max']:.1f}]  "
                  f"fused {f['median']:.1f} [{f['min']:.1f}, {f['max']:.1f}]  ratio {t['median'] / f['median']:.2f}x  "
                  f"agreement {agree}", flush=True)
    return out


def probe_trainer(prec, fused, dev, arch_name, classes, batch):
    from fsp_amd.clip import synth
    from fsp_amd.data.synthetic import SyntheticDataManager
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.trainers.linear_probe import LinearProbeCLIP
    arch = synth.ARCHS[arch_name]
    cfg = get_cfg_default()
    cfg.TRAINER.NAME = "LinearProbeCLIP"
    cfg.MODEL.BACKBONE.NAME = arch_name
    cfg.INPUT.SIZE = (arch.image_resolution, arch.image_resolution)
    cfg.TRAINER.LINEAR_PROBE.PREC = prec
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = batch
    cfg.OPTIM.MAX_EPOCH = 10
    cfg.TEST.NO_TEST = True
    cfg.MODEL.SYNTH_FP16 = True
    cfg.NATIVE.FUSED_PROBE = fused
    dm = SyntheticDataManager(classes, arch.image_resolution, batch, n_batches=2, device=dev)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = LinearProbeCLIP(cfg, dm=dm)
    tr.num_batches = 10 ** 9  # keep update_lr out of the timed loop
    tr.set_model_mode("train")
    return tr, dm


def run_step(args, dev):
    import torch
    variants = {}
    for name, fused, cached in (("uncached_off", False, False), ("uncached_on", True, False),
                                ("cached_off", False, True), ("cached_on", True, True)):
        torch.manual_seed(0)
        tr, dm = probe_trainer(args.prec, fused, dev, args.arch, args.classes, args.batch)
        batches = dm.train_loader_x
        if cached:  # what the trainer's run_epoch hands over from the bank after the first epoch
            batches = [{"feat": tr.model.image_features(b["img"]), "label": b["label"]} for b in batches]
        variants[name] = (tr, batches)
    first = {k: float(tr.forward_backward(b[0])["loss"]) for k, (tr, b) in variants.items()}
    print(f"first-step losses: {first}", flush=True)
    assert max(first.values()) - min(first.values()) <= 1e-3 * abs(first["uncached_off"]), first
    per = {k: [] for k in variants}

    def steps(k, count):
        tr, batches = variants[k]
        it = [0]

        def one():
            tr.forward_backward(batches[it[0] % 2])
            it[0] += 1
        return timed(one, count)

    for k in per:
        steps(k, 3)  # warm-up
    for _ in range(args.reps):
        for k in per:
            per[k].append(steps(k, args.steps) / args.steps)
    res = {k: spread(v) for k, v in per.items()}
    print(f"LinearProbeCLIP step {args.arch} C {args.classes} B {args.batch} {args.prec} ms/step: "
          + "  ".join(f"{k} {r['median']:.3f} [{r['min']:.3f}, {r['max']:.3f}]" for k, r in res.items()), flush=True)
    return {"first_step_loss": first, "ms_per_step": res}


def kernel_rows(path):
    with open(path, newline="") as f:
        return sum(1 for _ in csv.DictReader(f))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["head", "step", "calls", "count"])
    ap.add_argument("rest", nargs="*")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--prec", default="fp16")
    ap.add_argument("--arch", default="ViT-B/16")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.mode == "count":
        ta, ca, tb, cb = args.rest
        ka, kb = kernel_rows(ta), kernel_rows(tb)
        print(json.dumps({"kernels": [ka, kb], "calls": [int(ca), int(cb)],
                          "launches_per_call": (kb - ka) / (int(cb) - int(ca))}))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("probe_head_timing.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.mode == "calls":
        variant, B, C, E, focal, calls = args.rest[0], *(int(v) for v in args.rest[1:6])
        x = head_inputs(B, C, E, dev)
        for _ in range(calls):
            head_call(variant, x, bool(focal))
        torch.cuda.synchronize()
        return
    if args.reps is None:
        args.reps = 7 if args.mode == "head" else 5
    res = {"mode": args.mode, "device": torch.cuda.get_device_name(0),
           "result": run_head(args, dev) if args.mode == "head" else run_step(args, dev)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
