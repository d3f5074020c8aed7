"""PromptSRC head: the native clipk_src_head (NATIVE.FUSED_SRC) against the torch composition with
autograd that PromptSRCCustomCLIP.forward / PromptSRC.forward_backward run with the flag off.

    python tools/lab/src_head_timing.py head  [--reps 7] [--calls 200] [--out FILE.json]
        Head forward + backward at (B, C, E) = (4, 100, 512), (4, 1000, 512), (32, 1000, 512), CE and
        focal: the composition against SRCHeadFn, us per call. Device events around `calls` calls
        ending in a synchronise, every case warmed up, the two variants alternated in one process,
        `reps` repetitions; median, min and max are reported.
    python tools/lab/src_head_timing.py step  [--reps 5] [--steps 10] [--prec fp32s] [--out FILE.json]
        One PromptSRC train step (ViT-B/16, C = 1000, B = 4, synthetic fp16-valued weights):
        FUSED_SRC off against on, ms per step, alternated; first the agreement of the two variants'
        loss and of every trainable tensor's gradient on the same batch and parameters (max rel err).
    python tools/lab/src_head_timing.py calls VARIANT B C E FOCAL CALLS
        Exactly CALLS head forward + backward calls of VARIANT (torch | fused), nothing timed: the
        body of a kernel-trace run. Launches per call = the difference of the kernel counts of two
        runs over the difference of their CALLS (set-up and first-call kernels cancel):
            rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/lab/src_head_timing.py calls fused 4 1000 512 0 10
    python tools/lab/src_head_timing.py count TRACE_A.csv CALLS_A TRACE_B.csv CALLS_B
        That difference from two kernel-trace CSVs.
"""
import argparse
import contextlib
import csv
import io
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HEAD_SHAPES = [(4, 100, 512), (4, 1000, 512), (32, 1000, 512)]
SCALE, W_TEXT, W_IMAGE, W_LOGITS = 100.0, 25.0, 10.0, 1.0


def head_inputs(B, C, E, dev):
    """The recipe of tests/srchead_util.py: prompted features near the frozen ones."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(1000003 * B + 1009 * C + E)

    def r(*shape):
        return torch.randn(*shape, dtype=torch.float64, generator=g)

    fixed_n = F.normalize(r(C, E), dim=-1).float()
    txt = (3 * (fixed_n.double() + 0.5 * r(C, E) / math.sqrt(E))).float()
    zs = (2 * r(B, E)).float()
    img = (2.5 * (F.normalize(zs.double(), dim=-1) + 0.5 * r(B, E) / math.sqrt(E))).float()
    y = torch.randint(0, C, (B,), generator=g)
    alpha = (0.25 + 4 * torch.rand(C, dtype=torch.float64, generator=g)).float()
    return {"img": img.to(dev).requires_grad_(), "txt": txt.to(dev).requires_grad_(), "zs": zs.to(dev),
            "fixed_n": fixed_n.to(dev), "fixed_q": fixed_n.half().float().to(dev), "y": y.to(dev),
            "alpha": alpha.to(dev)}


def head_call(variant, x, focal):
    """One forward + backward of the head on the leaves img, txt (gradients overwritten)."""
    import torch
    import torch.nn.functional as F
    from fsp_amd.trainers._fns import CrossEntropyFn, SRCHeadFn
    img, txt = x["img"], x["txt"]
    img.grad = txt.grad = None
    alpha, gamma = (x["alpha"], 2.0) if focal else (None, 0.0)
    if variant == "fused":
        loss = SRCHeadFn.apply(img, txt, x["zs"], x["fixed_n"], x["fixed_q"], x["y"], alpha, gamma, focal, SCALE,
                               W_TEXT, W_IMAGE, W_LOGITS)
    else:  # _DeepCLIP.features, PromptSRCCustomCLIP.forward and PromptSRC.forward_backward, flag off
        u = F.normalize(img, dim=-1)
        t = F.normalize(txt, dim=-1)
        logits = SCALE * u @ t.t()
        fixed = F.normalize(x["fixed_n"], dim=-1)
        with torch.no_grad():
            z = F.normalize(x["zs"], dim=-1)
            zs_logits = SCALE * z @ fixed.half().float().t()
        loss_ce = CrossEntropyFn.apply(logits, x["y"], alpha, gamma, focal)
        l_text = F.l1_loss(t, fixed, reduction="mean") * W_TEXT
        l_img = F.l1_loss(u, z, reduction="mean") * W_IMAGE
        l_logits = F.kl_div(F.log_softmax(logits, dim=1), F.log_softmax(zs_logits, dim=1), reduction="sum",
                            log_target=True) / logits.numel() * W_LOGITS
        loss = loss_ce + (l_logits + l_text + l_img)
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
                got[v] = (loss.detach().clone(), x["img"].grad.clone(), x["txt"].grad.clone())
            per = {"torch": [], "fused": []}
            for v in per:
                timed(lambda: head_call(v, x, focal), 20)  # warm-up
            for _ in range(args.reps):
                for v in per:
                    per[v].append(1000.0 * timed(lambda: head_call(v, x, focal), args.calls) / args.calls)
            key = f"{B}x{C}x{E}_{'focal' if focal else 'ce'}"
            out[key] = {v: spread(t) for v, t in per.items()}
            out[key]["fused_vs_torch"] = {"loss_rel": rel_err(got["fused"][0], got["torch"][0]),
                                          "d_img_rel": rel_err(got["fused"][1], got["torch"][1]),
                                          "d_txt_rel": rel_err(got["fused"][2], got["torch"][2])}
            t, f = out[key]["torch"], out[key]["fused"]
            print(f"head fwd+bwd {key} us/call: torch {t['median']:.1f} [{t['min']:.1f}, {t['max']:.1f}]  "
                  f"fused {f['median']:.1f} [{f['min']:.1f}, {f['max']:.1f}]  ratio {t['median'] / f['median']:.2f}x  "
                  f"agreement {out[key]['fused_vs_torch']}", flush=True)
    return out


def promptsrc_trainer(prec, fused, dev, arch_name="ViT-B/16", classes=1000, batch=4, loss_type="ce"):
    from fsp_amd.clip import synth
    from fsp_amd.data.synthetic import SyntheticDataManager
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.trainers.deep import PromptSRC
    arch = synth.ARCHS[arch_name]
    cfg = get_cfg_default()
    cfg.TRAINER.NAME = "PromptSRC"
    cfg.MODEL.BACKBONE.NAME = arch_name
    cfg.INPUT.SIZE = (arch.image_resolution, arch.image_resolution)
    cfg.TRAINER.PROMPTSRC.PREC = prec
    cfg.TRAINER.PROMPTSRC.LOSS_TYPE = loss_type
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = batch
    cfg.OPTIM.MAX_EPOCH = 10
    cfg.TEST.NO_TEST = True
    cfg.MODEL.SYNTH_FP16 = True
    cfg.NATIVE.FUSED_SRC = fused
    dm = SyntheticDataManager(classes, arch.image_resolution, batch, n_batches=2, device=dev)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = PromptSRC(cfg, dm=dm)
    tr.num_batches = 10 ** 9  # keep update_lr and the GPA accumulate out of the timed loop
    return tr, dm


def run_step(args, dev):
    import torch
    kw = dict(arch_name=args.arch, classes=args.classes, batch=args.batch)
    trainers = {}
    for v, fused in (("off", False), ("on", True)):
        torch.manual_seed(0)  # the random prompt init
        trainers[v] = promptsrc_trainer(args.prec, fused, dev, **kw)
    p_off = dict(trainers["off"][0].model.named_parameters())
    with torch.no_grad():
        for k, p in trainers["on"][0].model.named_parameters():
            p.copy_(p_off[k])
    # agreement on one batch, before any step
    got = {}
    s = trainers["off"][0].sec
    for v, (tr, dm) in trainers.items():
        import torch.nn.functional as F
        b = dm.train_loader_x[0]
        tr.model.train()
        params = {k: p for k, p in tr.model.named_parameters() if p.requires_grad}
        for p in params.values():
            p.grad = None
        if v == "on":
            loss = tr.model.fused_loss(b["img"], b["label"], s.TEXT_LOSS_WEIGHT, s.IMAGE_LOSS_WEIGHT,
                                       s.get("LOGITS_LOSS_WEIGHT", 1.0))
            assert loss is not None, "the fused path did not take the step's inputs"
        else:
            loss_ce, txt, fixed, zs, img, zs_logits, logits = tr.model(b["img"], b["label"])
            loss = loss_ce + (F.kl_div(F.log_softmax(logits, dim=1), F.log_softmax(zs_logits, dim=1),
                                       reduction="sum", log_target=True) / logits.numel()
                              * s.get("LOGITS_LOSS_WEIGHT", 1.0)
                              + F.l1_loss(txt, fixed, reduction="mean") * s.TEXT_LOSS_WEIGHT
                              + F.l1_loss(img, zs, reduction="mean") * s.IMAGE_LOSS_WEIGHT)
        loss.backward()
        got[v] = (loss.detach().clone(), {k: p.grad.detach().clone() for k, p in params.items()})
        for p in params.values():
            p.grad = None
    agree = {"loss_off": float(got["off"][0]), "loss_on": float(got["on"][0]),
             "loss_rel": rel_err(got["on"][0], got["off"][0]),
             "grad_rel": {k: rel_err(g, got["off"][1][k]) for k, g in got["on"][1].items()}}
    print(f"agreement on vs off ({args.prec}): loss {agree['loss_off']:.6f} / {agree['loss_on']:.6f} rel "
          f"{agree['loss_rel']:.2e}; max rel err of the trainable gradients: "
          f"{max(agree['grad_rel'].values()):.2e} ({len(agree['grad_rel'])} tensors)", flush=True)
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
    slower_by = res["on"]["median"] - res["off"]["median"]
    res["on_minus_off_ms"] = slower_by
    res["off_spread_ms"] = res["off"]["max"] - res["off"]["min"]
    res["on_within_off_spread"] = bool(slower_by <= res["off_spread_ms"])
    print(f"PromptSRC step {args.arch} C {args.classes} B {args.batch} {args.prec} ms/step: "
          f"off {res['off']['median']:.3f} [{res['off']['min']:.3f}, {res['off']['max']:.3f}]  "
          f"on {res['on']['median']:.3f} [{res['on']['min']:.3f}, {res['on']['max']:.3f}]  "
          f"on - off {slower_by:+.3f} ms (off's spread {res['off_spread_ms']:.3f} ms)", flush=True)
    return {"agreement": agree, "ms_per_step": res}


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
    ap.add_argument("--prec", default="fp32s")
    ap.add_argument("--arch", default="ViT-B/16")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=4)
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
        raise SystemExit("src_head_timing.py measures on the GPU; none is visible")
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
