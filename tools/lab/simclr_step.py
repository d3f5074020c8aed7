"""SimCLR training: the native NT-Xent loss and the shared text encode (NATIVE.FUSED_SIMCLR)
against the torch composition and the reference's two forward_once calls.

    python tools/lab/simclr_step.py loss  [--reps 7] [--calls 200] [--out FILE.json]
        Loss forward + backward at (n, D) = (32, 1000) and (8, 512): LogitsNTXentLoss(fused=False)
        against NTXentFn, us per call. Device events around `calls` calls ending in a synchronise,
        every shape warmed up, the two variants alternated in one process, `reps` repetitions;
        median, min and max are reported.
    python tools/lab/simclr_step.py step  [--reps 5] [--steps 10] [--prec fp32s] [--out FILE.json]
        CoOp SimCLR train step at config 2's shapes (ViT-B/16, C = 1000, B = 32, n_ctx 16):
        FUSED_SIMCLR off against on, ms per step, alternated; first the agreement of the two
        variants' loss and ctx.grad on the same batch and ctx (max rel err).
    python tools/lab/simclr_step.py calls VARIANT N D CALLS
        Exactly CALLS loss forward + backward calls of VARIANT (torch | fused), nothing timed: the
        body of a kernel-trace run. Launches per call = the difference of the kernel counts of two
        runs over the difference of their CALLS (set-up and first-call kernels cancel):
            rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/lab/simclr_step.py calls fused 32 1000 10
    python tools/lab/simclr_step.py count TRACE_A.csv CALLS_A TRACE_B.csv CALLS_B
        That difference from two kernel-trace CSVs.
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

LOSS_SHAPES = [(32, 1000), (8, 512)]


def loss_inputs(n, D, dev):
    import torch
    g = torch.Generator().manual_seed(1000 * n + D)
    a = 4 * torch.randn(n, D, dtype=torch.float64, generator=g)
    b = 0.2 * a + 4 * torch.randn(n, D, dtype=torch.float64, generator=g)
    return a.float().to(dev).requires_grad_(), b.float().to(dev).requires_grad_()


def loss_call(variant, a, b):
    """One forward + backward of the loss on leaves a, b (gradients overwritten, not summed)."""
    from fsp_amd.trainers.losses import LogitsNTXentLoss
    a.grad = b.grad = None
    LogitsNTXentLoss(fused=variant == "fused")(a, b).backward()


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


def run_loss(args, dev):
    out = {}
    for n, D in LOSS_SHAPES:
        a, b = loss_inputs(n, D, dev)
        per = {"torch": [], "fused": []}
        for v in per:
            timed(lambda: loss_call(v, a, b), 20)  # warm-up
        for _ in range(args.reps):
            for v in per:
                per[v].append(1000.0 * timed(lambda: loss_call(v, a, b), args.calls) / args.calls)
        out[f"{n}x{D}"] = {v: spread(x) for v, x in per.items()}
        t, f = out[f"{n}x{D}"]["torch"], out[f"{n}x{D}"]["fused"]
        print(f"loss fwd+bwd ({n}, {D}) us/call: torch {t['median']:.1f} [{t['min']:.1f}, {t['max']:.1f}]  "
              f"fused {f['median']:.1f} [{f['min']:.1f}, {f['max']:.1f}]  ratio {t['median'] / f['median']:.2f}x",
              flush=True)
    return out


def coop_trainer(prec, fused, dev, arch_name="ViT-B/16", classes=1000, batch=32):
    from fsp_amd.clip import synth
    from fsp_amd.data.synthetic import SyntheticDataManager
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.trainers.coop import CoOp
    arch = synth.ARCHS[arch_name]
    cfg = get_cfg_default()
    cfg.TRAINER.NAME = "CoOp"
    cfg.MODEL.BACKBONE.NAME = arch_name
    cfg.INPUT.SIZE = (arch.image_resolution, arch.image_resolution)
    c = cfg.TRAINER.COOP
    c.N_CTX, c.CTX_INIT, c.CSC, c.CLASS_TOKEN_POSITION, c.PREC, c.LOSS_TYPE = 16, "", False, "end", prec, "simclr"
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = batch
    cfg.OPTIM.MAX_EPOCH = 10
    cfg.TEST.NO_TEST = True
    cfg.MODEL.SYNTH_FP16 = True
    cfg.NATIVE.FUSED_SIMCLR = fused
    dm = SyntheticDataManager(classes, arch.image_resolution, batch, n_batches=2, device=dev, two_views=True)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = CoOp(cfg, dm=dm)
    tr.num_batches = 10 ** 9  # keep update_lr out of the timed loop
    return tr, dm


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def loss_grad_errors(trainer_dm, dev):
    """How well conditioned the step's own loss is: d loss / d logits of the torch composition and
    of the kernel at the step's two-view logits, against the oracle in fp64 on the CPU (max abs
    err over max |grad64|). Where both are far above fp32 eps the loss sits in its saturated
    regime and the variants' ctx.grad agreement is bounded by that, not by the kernel."""
    import torch
    from fsp_amd import ops
    from fsp_amd.trainers.losses import LogitsNTXentLoss
    from oracle import clip_oracle as O
    tr, dm = trainer_dm
    b = dm.train_loader_x[0]
    with torch.no_grad():
        l1, l2 = tr.model.forward_two_views(b["img1"], b["img2"])
    a64, b64 = l1.double().cpu().requires_grad_(), l2.double().cpu().requires_grad_()
    O.ntxent_logits_loss(a64, b64).backward()
    g64 = torch.cat([a64.grad, b64.grad])
    at, bt = l1.clone().requires_grad_(), l2.clone().requires_grad_()
    LogitsNTXentLoss(fused=False)(at, bt).backward()
    _, da, db = ops.ntxent_loss(l1.contiguous(), l2.contiguous())
    gmax = float(g64.abs().max())
    out = {"grad64_max": gmax,
           "torch": float((torch.cat([at.grad, bt.grad]).double().cpu() - g64).abs().max()) / gmax,
           "kernel": float((torch.cat([da, db]).double().cpu() - g64).abs().max()) / gmax}
    print(f"d loss / d logits at the step's logits vs fp64: max |grad64| {gmax:.3e}, rel err torch "
          f"{out['torch']:.2e}, kernel {out['kernel']:.2e}", flush=True)
    return out


def run_step(args, dev):
    import torch
    kw = dict(arch_name=args.arch, classes=args.classes, batch=args.batch)
    torch.manual_seed(0)  # the random ctx init
    trainers ={"off": coop_trainer(args.prec, False, dev, **kw), "on": coop_trainer(args.prec, True, dev, **kw)}
    ctx_off = trainers["off"][0].model.prompt_learner.ctx
    with torch.no_grad():
        trainers["on"][0].model.prompt_learner.ctx.copy_(ctx_off)
    # agreement on one batch, before any step
    got = {}
    for v, (tr, dm) in trainers.items():
        b = dm.train_loader_x[0]
        tr.model.train()
        ctx = tr.model.prompt_learner.ctx
        ctx.grad = None
        loss = tr.model(b["img1"], None, b["img2"])
        loss.backward()
        got[v] = (loss.detach().clone(), ctx.grad.detach().clone())
        ctx.grad = None
    agree = {"loss_off": float(got["off"][0]), "loss_on": float(got["on"][0]),
             "loss_rel": rel_err(got["on"][0], got["off"][0]), "ctx_grad_rel": rel_err(got["on"][1], got["off"][1])}
    print(f"agreement on vs off ({args.prec}): loss {agree['loss_off']:.6f} / {agree['loss_on']:.6f} rel "
          f"{agree['loss_rel']:.2e}, ctx.grad max rel err {agree['ctx_grad_rel']:.2e}", flush=True)
    agree["loss_grad_vs_fp64"] = loss_grad_errors(trainers["on"], dev)
    # which half of the key moves ctx.grad: one model, the two halves switched separately
    tr, dm = trainers["off"]
    b = dm.train_loader_x[0]
    ctx = tr.model.prompt_learner.ctx
    parts = {}
    for name, shared, fused in [("off", False, False), ("loss_only", False, True), ("text_only", True, False),
                                ("on", True, True)]:
        tr.model.fused_simclr, tr.model.criterion_simclr.fused = shared, fused
        ctx.grad = None
        tr.model(b["img1"], None, b["img2"]).backward()
        parts[name] = ctx.grad.detach().clone()
    tr.model.fused_simclr = tr.model.criterion_simclr.fused = False
    ctx.grad = None
    agree["ctx_grad_rel_by_part"] = {k: rel_err(v, parts["off"]) for k, v in parts.items() if k != "off"}
    print("ctx.grad max rel err vs off, one model: " +
          ", ".join(f"{k} {v:.2e}" for k, v in agree["ctx_grad_rel_by_part"].items()), flush=True)
    per = {"off": [], "on": []}

    def steps(v, count):
        tr, dm = trainers[v]
        it = [0]

        def one():
            tr.forward_backward(dm.train_loader_x[it[0] % 2])
            it[0] += 1
        return timed(one, count)

    for v in per:
        steps(v, 3)  # warm-up
    for _ in range(args.reps):
        for v in per:
            per[v].append(steps(v, args.steps) / args.steps)
    res = {v: spread(x) for v, x in per.items()}
    print(f"CoOp SimCLR step {args.arch} C {args.classes} B {args.batch} {args.prec} ms/step: "
          f"off {res['off']['median']:.3f} [{res['off']['min']:.3f}, {res['off']['max']:.3f}]  "
          f"on {res['on']['median']:.3f} [{res['on']['min']:.3f}, {res['on']['max']:.3f}]  "
          f"ratio {res['off']['median'] / res['on']['median']:.3f}x", flush=True)
    return {"agreement": agree, "ms_per_step": res}


def kernel_rows(path):
    with open(path, newline="") as f:
        return sum(1 for _ in csv.DictReader(f))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["loss", "step", "calls", "count"])
    ap.add_argument("rest", nargs="*")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--prec", default="fp32s")
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
        raise SystemExit("simclr_step.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.mode == "calls":
        variant, n, D, calls = args.rest[0], int(args.rest[1]), int(args.rest[2]), int(args.rest[3])
        a, b = loss_inputs(n, D, dev)
        for _ in range(calls):
            loss_call(variant, a, b)
        torch.cuda.synchronize()
        return
    if args.reps is None:
        args.reps = 7 if args.mode == "loss" else 5
    res = {"mode": args.mode, "device": torch.cuda.get_device_name(0),
           "result": run_loss(args, dev) if args.mode == "loss" else run_step(args, dev)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
