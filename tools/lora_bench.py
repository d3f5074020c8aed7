#!/usr/bin/env python3
"""LoRA timing on one MI355X (bench.py stays the headline; this is the LoRA trainer's own).

One LoRA train step (trainers/lora.py: merge, both encoders forward + backward with the adapter
gradients, cosine head + CE, FusedAdam / adamw) on a synthetic ViT-B/16 CLIP, RANK 2, ENCODER both,
B images against C class prompts, and beside it, alternated in one process:

  hook_off   the same step with the LoRA work taken out (no merge, no clipk_lora_wgrad: the
             encoders' forward + input-gradient backward on the merged tables alone) -- the cost
             baseline;
  torch      the oracle composition (oracle/clip_oracle.py on p' = W0 + s B A, autograd) in fp32
             torch on the device -- what PyTorch would do.

Parts, device events around each: the merge of both encoders (and, PREC fp32s, its split-pack
launches, timed separately), and the clipk_lora_wgrad launches of a step summed per encoder
(clipk_prof_sites: events around each call on the launch stream, with its algorithmic bytes: X and
dq|dk|dv read twice).

    python tools/lora_bench.py --prec fp16 --classes 100 1000 --out profiles/lora/timing_fp16.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def build(prec, C, B, rank, dev):
    from fsp_amd.clip import synth
    from fsp_amd.clip.model import build_model
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.engine.optim import build_optimizer
    from fsp_amd.trainers import lora as L
    arch = synth.ARCHS["ViT-B/16"]
    sd = synth.make_state_dict("ViT-B/16", seed=0, fp16_values=True)
    cfg = get_cfg_default()
    cfg.TRAINER.LORA.PREC, cfg.TRAINER.LORA.RANK = prec, rank
    cfg.OPTIM.NAME, cfg.OPTIM.LR = "adamw", 2e-4
    sec = cfg.TRAINER.LORA
    clip = build_model(sd, prec=prec, device=dev, text_grad=True, vision_grad=True,
                       text_lora=L.lora_spec(sec, arch.transformer_layers),
                       vision_lora=L.lora_spec(sec, arch.vision_layers))
    ad = L.LoraAdapters(arch, rank).to(dev)
    with torch.no_grad():  # past the initial B = 0: both gradients carry work-like values
        for side in (ad.text, ad.visual):
            side.lora_B.normal_(0.0, 0.01)
    model = L.LoraCLIP(cfg, synth.synthetic_classnames(C), clip, ad).train()
    opt = build_optimizer(ad, cfg.OPTIM)
    img = torch.from_numpy(synth.make_images(B, arch.image_resolution, seed=1)).to(dev)
    lbl = torch.from_numpy(synth.make_labels(B, C, seed=2)).to(dev)
    return arch, sd, model, ad, opt, img, lbl


def torch_step(sd, ad, model, img, lbl, rank, dev):
    """The oracle composition in fp32 torch on the device: a closure running one forward + backward."""
    from oracle import clip_oracle as O
    from lora_util import lora_params
    p = {k: v.to(dev) for k, v in O.as_torch_sd(sd).items()}
    leaves = {s: (getattr(ad, s).lora_A.detach().clone().requires_grad_(True),
                  getattr(ad, s).lora_B.detach().clone().requires_grad_(True)) for s in ("text", "visual")}
    masks = {"text": (1 << 12) - 1, "visual": (1 << 12) - 1}
    Lr = model.L
    tok = torch.zeros(model.n_cls, 77, dtype=torch.int64, device=dev)
    tok[torch.arange(model.n_cls, device=dev), model.eot] = 1  # argmax -> the EOT positions
    prompts = (model.x0 - p["positional_embedding"][:Lr]).contiguous()
    scale = float(model.logit_scale_value)

    def step():
        for a, b in leaves.values():
            a.grad = b.grad = None
        with torch.device(dev):  # (the oracle's masks and index ranges: created where its inputs live)
            q = lora_params(p, leaves, 1.0 / rank, 7, masks)
            txt = O.encode_text(q, prompts, tok)
            imf = O.encode_image(q, img)
            F.cross_entropy(scale * O.normalize(imf) @ O.normalize(txt).t(), lbl).backward()

    return step


def run(prec, C, B, rank, iters, reps, dev):
    from fsp_amd import _native as N, ops
    arch, sd, model, ad, opt, img, lbl = build(prec, C, B, rank, dev)
    tabs = {"text": model.clip.text.lora, "visual": model.clip.visual.lora}

    def step():
        loss = model(img, lbl)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    real = {k: (t.merge, t.grads) for k, t in tabs.items()}

    def step_off():
        for t in tabs.values():  # no merge, no adapter-gradient hook
            t.merge = lambda A, Bm: None
            t.grads = lambda h, A, Bm: (torch.zeros_like(A), torch.zeros_like(Bm))
        try:
            return step()
        finally:
            for k, t in tabs.items():
                t.merge, t.grads = real[k]

    res = {"prec": prec, "C": C, "B": B, "rank": rank, "text_rows": model.n_cls * model.L,
           "vit_rows": B * model.clip.visual.n_tokens, "loss": float(step().detach())}
    fns = {"lora_step": step, "hook_off_step": step_off,
           "torch_fp32_step": torch_step(sd, ad, model, img, lbl, rank, dev)}
    res["step"] = timed(fns, iters, reps)

    # parts: the merge of both encoders (its split-pack launches apart), hipEvents around each
    def merge_only():
        for k, t in tabs.items():
            a = getattr(ad, k)
            sp = t.spec
            ops.lora_merge(t.w0, a.lora_A.detach(), a.lora_B.detach(), sp.proj_mask, sp.layer_mask, sp.scale,
                           t.stage if t.split else t.out, t.stageT if t.split else t.outT)

    parts = {"merge_both": merge_only}
    if prec == "fp32s":
        def pack_only():
            for t in tabs.values():
                for src, dst in zip(t.stage + t.stageT, t.out + t.outT):
                    ops.split_pack(src, out=dst)
        parts["split_pack_both"] = pack_only
        res["split_pack_launches_per_step"] = sum(len(t.stage) + len(t.stageT) for t in tabs.values())
    res["parts"] = timed(parts, 20, reps)
    esz = {"fp32": 4, "fp32s": 4}.get(prec, 2)
    mbytes = sum(t.layers * 3 * t.W * t.W * (4 + 2 * esz) for t in tabs.values())
    res["parts"]["merge_both"]["bytes"] = mbytes
    res["parts"]["merge_both"]["GBps"] = mbytes / res["parts"]["merge_both"]["median_ms"] / 1e6
    # the wgrad launches of a step, summed per encoder (events around each call)
    lib = N.load()
    step()
    torch.cuda.synchronize()
    lib.clipk_prof_sites_enable(1)
    nstep = 5
    for _ in range(nstep):
        step()
    torch.cuda.synchronize()
    sites = N.prof_sites_read(128)
    lib.clipk_prof_sites_enable(0)
    res["wgrad"] = {k: {"ms_per_step": v[0] / nstep, "calls_per_step": v[1] / nstep, "bytes_per_step": v[3] / nstep,
                        "GBps": v[3] / v[0] / 1e6} for k, v in sites.items() if k.endswith("lora_wgrad")}
    st = res["step"]
    res["lora_share_of_step"] = (st["lora_step"]["median_ms"] - st["hook_off_step"]["median_ms"]) / \
        st["lora_step"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", default="fp16")
    ap.add_argument("--classes", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rank", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lora_bench.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    results = []
    for C in a.classes:
        r = run(a.prec, C, a.batch, a.rank, a.iters, a.reps, dev)
        print(json.dumps(r), flush=True)
        results.append(r)
        if a.out:  # (after every case: a later one running out of time keeps the earlier ones)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
