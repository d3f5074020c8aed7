"""Times the two mixup kernels against what they replace, on the GPU (DESIGN section 5 "Mixup").

  python tools/lab/mixup_timing.py [--out FILE.json]

* clipk_mixup_images (ops.mixup_images, perm upload included) against torch's
  lam * x + (1 - lam) * x[perm] at B = 32, 3 x 224 x 224 fp32;
* the mixed criterion forward + backward at [32, 1000], CE and focal: MixedCrossEntropyFn
  (clipk_ce_loss_mix) against the two-call branch (two CrossEntropyFn combined through autograd) and
  against the torch expression (F.cross_entropy / the focal form, twice).

Each variant runs `--iters` calls per block between two synchronises (host clock), the variants
alternate block by block for `--rounds` rounds, and the median block is reported as us per call.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def timed(variants, iters, rounds):
    for fn in variants.values():  # warm-up: code objects, allocator
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    blocks = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            blocks[k].append((time.perf_counter() - t0) / iters * 1e6)
    return {k: {"us_median": statistics.median(v), "us_min": min(v), "us_max": max(v)} for k, v in blocks.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mixup_timing.py needs the GPU: nothing is measured without one")
    from fsp_amd import ops
    from fsp_amd.trainers._fns import CrossEntropyFn, MixedCrossEntropyFn, backward_unit
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds}

    B = 32
    x = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    labels = torch.randint(0, 1000, (B,), generator=g).to(dev)
    perm = torch.randperm(B, generator=g)
    lam = 0.37
    out, y_b = ops.mixup_images(x, perm, lam, labels)
    assert torch.equal(out, lam * x + (1 - lam) * x[perm.to(dev)]) and torch.equal(y_b, labels[perm.to(dev)])

    def torch_mix():
        idx = perm.to(dev, non_blocking=True)
        return lam * x + (1 - lam) * x[idx], labels[idx]

    r = timed({"clipk_mixup_images": lambda: ops.mixup_images(x, perm, lam, labels), "torch": torch_mix},
              args.iters, args.rounds)
    nbytes = 3 * x.numel() * 4  # two reads and one write per element
    for v in r.values():
        v["GBps_at_median"] = nbytes / v["us_median"] * 1e-3
    res["mixup_images_B32_224"] = dict(r, bytes=nbytes)

    C = 1000
    logits = (10 * torch.randn(B, C, generator=g)).to(dev).requires_grad_(True)
    y_a = torch.randint(0, C, (B,), generator=g).to(dev)
    y_p = y_a[perm.to(dev)]
    alpha = (torch.rand(C, generator=g) + 0.5).to(dev)

    def run(loss_fn):
        logits.grad = None
        backward_unit(loss_fn())

    def torch_L(y, focal):
        if not focal:
            return F.cross_entropy(logits, y)
        ce = F.cross_entropy(logits, y, reduction="none")
        return (alpha[y] * (1 - torch.exp(-ce)) ** 2 * ce).mean()

    for focal in (False, True):
        a = alpha if focal else None
        variants = {
            "clipk_ce_loss_mix": lambda: run(lambda: MixedCrossEntropyFn.apply(logits, y_a, y_p, lam, a, 2.0, focal)),
            "two_call_branch": lambda: run(lambda: lam * CrossEntropyFn.apply(logits, y_a, a, 2.0, focal)
                                           + (1 - lam) * CrossEntropyFn.apply(logits, y_p, a, 2.0, focal)),
            "torch": lambda: run(lambda: lam * torch_L(y_a, focal) + (1 - lam) * torch_L(y_p, focal)),
        }
        grads = {}
        for k, fn in variants.items():
            fn()
            grads[k] = logits.grad.clone()
        scale = float(grads["torch"].abs().max())
        r = timed(variants, args.iters, args.rounds)
        for k in r:
            r[k]["dlogits_vs_torch_rel"] = float((grads[k] - grads["torch"]).abs().max()) / scale
        res["mixed_%s_fwd_bwd_32x1000" % ("focal" if focal else "ce")] = r

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
