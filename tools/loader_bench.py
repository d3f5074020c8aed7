"""Times the training loader's per-image host path with NATIVE.DEVICE_TABLES and NATIVE.IMAGE_BANK
off and on (DESIGN section 5 "Image bank").

  python tools/loader_bench.py [--out profiles/image_bank/loader_bench.json] [--parts a,b,c]
                               [--variants off,tables,bank,both]

(a) the GpuTransform call on 32 decoded 500 x 375 images -> 32 views and 2 x 32 views of 224 (the
    shapes of DESIGN section 5 "Colour views"); with the bank the 32 images are banked beforehand,
    as from the second epoch on;
(b) two epochs of a DataManager over 512 JPEG files written by Pillow from seeded arrays into a
    temporary directory, read by the real read_image in 8 worker processes: images/s of epoch 1
    (decode, and with the bank the fill) and of epoch 2 (with the bank: no decode, no upload);
(c) the CoOp step (ViT-B/16, C = 1000, B = 32, n_ctx 16, CE; fp16 and fp32s) fed by the one-view
    call of (a).

The method is tools/lab/color_timing.py's: the host clock around blocks that end in a synchronise,
every variant warmed up, the variants alternated block by block in one process for `--rounds`
rounds, median [min, max] per variant. "off" is the loader as it is without the flags; a variant
is faster only where it beats "off" by more than that spread. `--parts a --variants off` runs on a
tree from before the flags too (nothing newer is imported), for the same-shape comparison with the
parent commit in a process of its own.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLAGS = {"off": (False, False), "tables": (True, False), "bank": (False, True), "both": (True, True)}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(variants, iters, rounds, warm=3, unit=1e6):
    for fn in variants.values():  # warm-up: code objects, allocator, pinned blocks
        for _ in range(warm):
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
            blocks[k].append((time.perf_counter() - t0) / iters * unit)
    return {k: spread(v) for k, v in blocks.items()}


def base_cfg(variant):
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (224, 224)
    tables, bank = FLAGS[variant]
    if tables:
        cfg.NATIVE.DEVICE_TABLES = True
    if bank:
        cfg.NATIVE.IMAGE_BANK = True
    return cfg


def transform_call(variant, images, dev, views):
    """-> a function of no arguments: one GpuTransform call on the 32 images."""
    from fsp_amd.data.preprocess import GpuTransform
    g = torch.Generator()
    g.manual_seed(0)
    tf = GpuTransform(base_cfg(variant), is_train=True, device=dev, generator=g)
    src = images
    if FLAGS[variant][1]:
        from fsp_amd.data.image_bank import ImageBank
        bank = ImageBank(len(images), dev)
        src = [bank.fetch(k, im) for k, im in enumerate(images)]
        tf.bank = bank  # keeps the chunks alive
    return (lambda: tf(src)) if views == 1 else (lambda: tf(src, views=2))


def part_a(args, dev, images, variants):
    out = {}
    for views in (1, 2):
        calls = {v: transform_call(v, images, dev, views) for v in variants}
        first = {v: fn() for v, fn in calls.items()}  # equal seeds: the variants must agree bit for bit
        ref = first[variants[0]]
        for v, x in first.items():
            same = torch.equal(x, ref) if views == 1 else all(torch.equal(p, q) for p, q in zip(x, ref))
            assert same, f"variant {v} differs from {variants[0]}"
        out[f"views{views}_us_B32"] = timed(calls, args.iters, args.rounds)
    return out


def write_jpegs(root, n, seed=0):
    """n JPEG files of 500 x 375 from seeded arrays (smooth content plus noise, so that the files
    decode at a photo's cost, not a flat field's)."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:375, 0:500]
    noise = rs.normal(0, 12, (375, 500, 3))
    paths = []
    for k in range(n):
        a, b, c = rs.uniform(0.01, 0.05, 3)
        base = np.stack([127 + 100 * np.sin(a * xx + k), 127 + 100 * np.cos(b * yy - k),
                         127 + 100 * np.sin(c * (xx + yy))], axis=2)
        img = np.clip(base + np.roll(noise, 7 * k, axis=1), 0, 255).astype(np.uint8)
        path = os.path.join(root, f"{k:04d}.jpg")
        Image.fromarray(img).save(path, quality=90)
        paths.append(path)
    return paths


def part_b(args, dev, variants):
    from fsp_amd.clip import synth
    from fsp_amd.data.fewshot import Datum
    from fsp_amd.data.manager import DataManager
    names = synth.synthetic_classnames(4)
    out = {v: {"epoch1_img_per_s": [], "epoch2_img_per_s": []} for v in variants}
    with tempfile.TemporaryDirectory() as root:
        paths = write_jpegs(root, args.files)

        class DS:
            train_x = [Datum(impath=p, label=k % 4, classname=names[k % 4]) for k, p in enumerate(paths)]
            test = train_x[:4]
            classnames = names
            lab2cname = dict(enumerate(names))
            num_classes = 4

        def two_epochs(v):
            cfg = base_cfg(v)
            cfg.DATALOADER.NUM_WORKERS = args.workers
            cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 32
            torch.manual_seed(0)
            dm = DataManager(cfg, DS, dev)
            rates = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                for b in dm.train_loader_x:
                    n += b["img"].shape[0]
                torch.cuda.synchronize()
                rates.append(n / (time.perf_counter() - t0))
            return rates

        for v in variants:  # warm-up: the file cache, code objects
            print(f"two epochs, warm-up, {v}: %.0f / %.0f img/s" % tuple(two_epochs(v)), flush=True)
        t_start = time.perf_counter()
        for r in range(args.rounds_b):
            if args.max_seconds_b and r and time.perf_counter() - t_start > args.max_seconds_b * r / (r + 1):
                print(f"two epochs: stopping after {r} rounds (--max-seconds-b)", flush=True)
                break
            for v in variants:
                e1, e2 = two_epochs(v)
                out[v]["epoch1_img_per_s"].append(e1)
                out[v]["epoch2_img_per_s"].append(e2)
                print(f"two epochs, round {r}, {v}: {e1:.0f} / {e2:.0f} img/s", flush=True)
    res = {v: {k: spread(x) for k, x in r.items()} for v, r in out.items()}
    res["rounds"] = len(out[variants[0]]["epoch1_img_per_s"])
    return res


def coop_trainer(prec, dev, classes=1000, batch=32):
    from fsp_amd.clip import synth
    from fsp_amd.data.synthetic import SyntheticDataManager
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.trainers.coop import CoOp
    arch = synth.ARCHS["ViT-B/16"]
    cfg = get_cfg_default()
    cfg.TRAINER.NAME = "CoOp"
    cfg.MODEL.BACKBONE.NAME = "ViT-B/16"
    cfg.INPUT.SIZE = (arch.image_resolution, arch.image_resolution)
    c = cfg.TRAINER.COOP
    c.N_CTX, c.CTX_INIT, c.CSC, c.CLASS_TOKEN_POSITION, c.PREC, c.LOSS_TYPE = 16, "", False, "end", prec, "ce"
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = batch
    cfg.OPTIM.MAX_EPOCH = 10
    cfg.TEST.NO_TEST = True
    cfg.MODEL.SYNTH_FP16 = True
    dm = SyntheticDataManager(classes, arch.image_resolution, batch, n_batches=2, device=dev)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = CoOp(cfg, dm=dm)
    tr.num_batches = 10 ** 9  # keep update_lr out of the timed loop
    return tr


def part_c(args, dev, images, variants):
    out = {}
    labels = torch.from_numpy(np.random.RandomState(1).randint(0, 1000, size=32).astype(np.int64)).to(dev)
    for prec in args.precs.split(","):
        torch.manual_seed(0)
        tr = coop_trainer(prec, dev)
        calls = {v: transform_call(v, images, dev, 1) for v in variants}

        def step(fn):
            tr.forward_backward({"img": fn(), "label": labels})

        steps = {v: (lambda fn=fn: step(fn)) for v, fn in calls.items()}
        steps["no_transform"] = (lambda x=calls[variants[0]](): tr.forward_backward({"img": x, "label": labels}))
        out[f"coop_step_ms_{prec}"] = dict(timed(steps, args.steps, args.rounds, warm=2, unit=1e3),
                                           shapes="ViT-B/16 C 1000 B 32 n_ctx 16 CE, one-view transform call included")
        del tr
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--variants", default="off,tables,bank,both")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rounds-b", type=int, default=7)
    ap.add_argument("--max-seconds-b", type=float, default=0.0,
                    help="part (b) starts no further round once the next one would pass this many seconds")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--precs", default="fp16,fp32s")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench.py needs the GPU: nothing is measured without one")
    variants = args.variants.split(",")
    if any(v not in FLAGS for v in variants):
        raise SystemExit(f"variants are {sorted(FLAGS)}")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    images = [rs.randint(0, 256, size=(375, 500, 3), dtype=np.uint8) for _ in range(32)]
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "variants": variants}
    parts = args.parts.split(",")
    if "a" in parts:
        res["transform_call"] = part_a(args, dev, images, variants)
        print(json.dumps({"transform_call": res["transform_call"]}), flush=True)
    if "c" in parts:
        res["coop_step"] = part_c(args, dev, images, variants)
        print(json.dumps({"coop_step": res["coop_step"]}), flush=True)
    if "b" in parts:  # last: it forks DataLoader workers
        res["two_epochs"] = dict(part_b(args, dev, variants), files=args.files, workers=args.workers)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
