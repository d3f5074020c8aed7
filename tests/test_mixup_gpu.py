"""GPU: IVLP mixup training from the loader to the optimizer step with NATIVE.MIXUP.

* clipk_mixup_images bitwise against torch's lam * x + (1 - lam) * x[perm] on the device, on both
  access paths; out-of-range perm entries, aliasing and the other argument errors at the C ABI;
* clipk_ce_loss_mix against an fp64 restatement of the formula, its error held to twice that of the
  two-call branch it replaces (two CrossEntropyFn calls combined with lam through autograd), which
  is measured against the same fp64 values in the same test;
* the registry-built IVLP trainer on SyntheticDataManager(mixup_alpha=1.0): key on against key off
  at the project's gate for fp32 re-orderings (loss / parameters rel <= 1e-4, gradients rel <= 1e-3),
  and which loss call each issues;
* the loaders: GpuLoader(mixup_alpha=...) on the real transform, DataManager with the key on / off.
"""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fsp_amd import _native as N
from fsp_amd import ops
from parity_util import rel_err

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
LAMS = (0.0, 1.0, 0.3, 1.0 / 3.0)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ clipk_mixup_images
def _perm(B, fixed_point, g):
    perm = torch.randperm(B, generator=g)
    if fixed_point and not any(int(perm[i]) == i for i in range(B)):
        j = int((perm == 0).nonzero()[0])
        perm[j], perm[0] = perm[0].clone(), 0  # still a permutation, with perm[0] == 0
    return perm


@pytest.mark.parametrize("B,shape,fixed_point", [
    (1, (192,), False),
    (3, (75,), False),           # a tail, rows start misaligned: the one-float path
    (5, (192,), True),           # a fixed point in perm
    (4, (3, 224, 224), False),   # grid coverage: many blocks per row, a partly filled last one
    (2, (2051,), False),         # the one-float path over more than one block
])
def test_mixup_images_bitwise(dev, B, shape, fixed_point):
    g = torch.Generator().manual_seed(B * 1000 + shape[-1])
    x = torch.randn(B, *shape, generator=g).to(dev)
    labels = torch.randint(0, 10, (B,), generator=g).to(dev)
    perm = _perm(B, fixed_point, g)
    if fixed_point:
        assert any(int(perm[i]) == i for i in range(B))
    idx = perm.to(dev)
    for lam in LAMS:
        out, y_b = ops.mixup_images(x, perm, lam, labels)
        ref = lam * x + (1 - lam) * x[idx]
        assert out.shape == x.shape and out.dtype == torch.float32
        assert torch.equal(out, ref), (lam, float((out - ref).abs().max()))
        assert torch.equal(y_b, labels[idx])
        out2, none = ops.mixup_images(x, perm.int(), lam)  # without labels, int32 perm
        assert none is None and torch.equal(out2, ref)
    assert torch.equal(ops.mixup_images(x, perm, 1.0)[0], x)


def test_mixup_images_misaligned_base_takes_the_scalar_path(dev):
    """n_per % 4 == 0 but x (or out) 4 bytes past a 16-byte boundary."""
    g = torch.Generator().manual_seed(7)
    B, n = 3, 1032
    base = torch.randn(B * n + 1, generator=g).to(dev)
    x = base[1:].view(B, n)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    perm = torch.tensor([2, 0, 1])
    out, _ = ops.mixup_images(x, perm, 0.3)
    assert torch.equal(out, 0.3 * x + (1 - 0.3) * x[perm.to(dev)])
    # ... and an aligned x into a misaligned out, through the C ABI
    xa = x.clone()
    assert xa.data_ptr() % 16 == 0
    obase = torch.zeros(B * n + 1, device=dev)
    o = obase[1:].view(B, n)
    N.call("clipk_mixup_images", B, n, _p(xa), _p(perm.int().to(dev)), None, None, 0.3, 1.0 - 0.3, _p(o), _stream())
    assert torch.equal(o, out) and float(obase[0]) == 0.0


def test_mixup_images_out_of_range_perm_rows_mix_with_themselves(dev):
    g = torch.Generator().manual_seed(11)
    B, n = 5, 192
    x = torch.randn(B, n, generator=g).to(dev)
    labels = torch.arange(B).to(dev) + 100
    perm = torch.tensor([3, -1, 4, B, 0], dtype=torch.int32).to(dev)
    idx = torch.tensor([3, 1, 4, 3, 0]).to(dev)  # rows 1 and 3 take p = b
    out = torch.empty_like(x)
    y_b = torch.empty_like(labels)
    lam = 0.3
    N.call("clipk_mixup_images", B, n, _p(x), _p(perm), _p(labels), _p(y_b), lam, 1.0 - lam, _p(out), _stream())
    torch.cuda.synchronize()  # the run is clean
    assert torch.equal(out, lam * x + (1 - lam) * x[idx])
    assert torch.equal(y_b, labels[idx])


def test_mixup_images_argument_errors(dev):
    lib = N.load()
    B, n = 4, 64
    x = torch.randn(B, n).to(dev)
    keep = x.clone()
    out = torch.full_like(x, 7.0)
    perm = torch.tensor([1, 0, 3, 2], dtype=torch.int32).to(dev)
    labels = torch.arange(B).to(dev)
    y_b = torch.full_like(labels, -5)

    def rc(B_, n_, x_, perm_, labels_, y_b_, out_):
        return lib.clipk_mixup_images(B_, n_, _p(x_), _p(perm_), _p(labels_), _p(y_b_), 0.5, 0.5, _p(out_), _stream())

    assert rc(B, n, x, perm, labels, y_b, x) == -1                       # out is x
    assert rc(B - 1, n, x, perm, labels, y_b, x[1:]) == -1               # out overlaps x
    assert rc(B, n, None, perm, labels, y_b, out) == -1
    assert rc(B, n, x, None, labels, y_b, out) == -1
    assert rc(B, n, x, perm, labels, y_b, None) == -1
    assert rc(B, n, x, perm, labels, None, out) == -1                    # only one of labels / y_b
    assert rc(B, n, x, perm, None, y_b, out) == -1
    assert rc(-1, n, x, perm, labels, y_b, out) == -2
    assert rc(B, 0, x, perm, labels, y_b, out) == -2
    assert rc(0, n, None, None, None, None, None) == 0                   # B == 0: nothing to do
    torch.cuda.synchronize()
    # nothing was launched
    assert torch.equal(x, keep) and bool((out == 7.0).all()) and bool((y_b == -5).all())
    with pytest.raises(N.ClipkError):
        ops.mixup_images(x, torch.tensor([0, 1, 2, 4]), 0.5)
    empty, y0 = ops.mixup_images(x[:0], torch.zeros(0, dtype=torch.int64), 0.5, labels[:0])
    assert empty.shape == (0, n) and y0.shape == (0,)


# ------------------------------------------------------------------ clipk_ce_loss_mix
def _fp64_reference(logits, y_a, y_b, lam, alpha, focal, reduction):
    """The formula in float64 on the CPU from the same fp32 logits -> (loss, d loss / d logits)."""
    z = logits.detach().double().cpu().requires_grad_(True)
    a64 = alpha.double().cpu() if alpha is not None else None

    def L(y):
        y = y.cpu()
        ce = F.cross_entropy(z, y, reduction="none")
        if focal:
            p = torch.exp(-ce)
            w = a64[y] if a64 is not None else 1.0
            ce = w * (1.0 - p) ** 2 * ce
        return ce.mean() if reduction == "mean" else ce.sum()

    loss = lam * L(y_a) + (1.0 - lam) * L(y_b)
    loss.backward()
    return loss.detach(), z.grad


def _yardstick(logits, y_a, y_b, lam, alpha, focal, reduction):
    """The two-call branch of IVLP.forward_backward: two CrossEntropyFn calls combined by autograd."""
    from fsp_amd.trainers._fns import CrossEntropyFn
    z = logits.detach().clone().requires_grad_(True)
    loss = lam * CrossEntropyFn.apply(z, y_a, alpha, 2.0, focal, reduction) \
        + (1 - lam) * CrossEntropyFn.apply(z, y_b, alpha, 2.0, focal, reduction)
    loss.backward()
    return loss.detach(), z.grad


def _err(got, ref):
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


VARIANTS = [(False, False), (True, False), (True, True)]  # (focal, with alpha)


@pytest.mark.parametrize("C", [2, 63, 64, 65, 130, 1000])
@pytest.mark.parametrize("B", [1, 3, 5, 9])
def test_ce_loss_mix_against_fp64(dev, B, C):
    """The kernel's eight waves see a ragged count (B = 1, 3, 5) and a second round (9); C around
    the wave width and up to the benchmark's 1,000. Measured on an MI355X over all of these cases
    (540 variants): loss error 2.8e-7 at most for the kernel and the two-call branch alike,
    dlogits 1.68e-6 for both at the worst variant and at most 1.42x the branch's in any; (1, 2)
    apart at 2.5e-4 for both (DESIGN section 3 "Mixup kernels")."""
    _check_against_fp64(dev, B, C)


@pytest.mark.parametrize("C", [1024, 1025, 1500])
def test_ce_loss_mix_against_fp64_long_rows(dev, C):
    """Rows of more than 1,024 classes leave the registers: the last cached size and the looping form."""
    _check_against_fp64(dev, 5, C)


def _check_against_fp64(dev, B, C):
    g = torch.Generator().manual_seed(100 * B + C)
    logits = (10 * torch.randn(B, C, generator=g)).to(dev)
    y_a = torch.randint(0, C, (B,), generator=g).to(dev)
    y_rand = torch.randint(0, C, (B,), generator=g).to(dev)
    alpha = (torch.rand(C, generator=g) + 0.5).to(dev)
    # one row with y_a == y_b (B == 1: the only row, so that size also runs without one)
    targets = []
    fixed = y_rand.clone()
    fixed[0] = y_a[0]
    targets.append(fixed)
    if B == 1:
        other = y_rand.clone()
        other[0] = (y_a[0] + 1) % C
        targets.append(other)
    worst = {"loss": (0.0, 0.0), "dlogits": (0.0, 0.0)}
    for y_b in targets:
        for focal, with_alpha in VARIANTS:
            a = alpha if with_alpha else None
            for reduction in ("mean", "sum"):
                for lam in (0.0, 1.0, 0.37):
                    ref_l, ref_d = _fp64_reference(logits, y_a, y_b, lam, a, focal, reduction)
                    yl, yd = _yardstick(logits, y_a, y_b, lam, a, focal, reduction)
                    loss, dl = ops.ce_loss_mix(logits, y_a, y_b, lam, a, 2.0, focal, reduction=reduction)
                    e_new = (_err(loss, ref_l), _err(dl, ref_d))
                    e_old = (_err(yl, ref_l), _err(yd, ref_d))
                    tag = (B, C, focal, with_alpha, reduction, lam)
                    print("ce_loss_mix", tag, "loss err new %.3g two-call %.3g" % (e_new[0], e_old[0]),
                          "dlogits err new %.3g two-call %.3g" % (e_new[1], e_old[1]))
                    for k, name in enumerate(("loss", "dlogits")):
                        if e_new[k] > worst[name][0]:
                            worst[name] = (e_new[k], e_old[k])
                        assert e_new[k] <= max(2.0 * e_old[k], 4.0 * EPS), (name, tag, e_new[k], e_old[k])
                    # forward only: the same loss
                    loss0, none = ops.ce_loss_mix(logits, y_a, y_b, lam, a, 2.0, focal, grad=False, reduction=reduction)
                    assert none is None and torch.equal(loss0, loss)
                    # reproducible bit for bit
                    loss2, dl2 = ops.ce_loss_mix(logits, y_a, y_b, lam, a, 2.0, focal, reduction=reduction)
                    assert torch.equal(loss2, loss) and torch.equal(dl2, dl)
                    if lam == 1.0:  # ... is clipk_ce_loss_reduce on y_a
                        l1, d1 = ops.ce_loss_reduce(logits, y_a, a, 2.0, focal, reduction=reduction)
                        bound_l, bound_d = (max(2.0 * e, 4.0 * EPS) for e in e_old)
                        assert _err(loss, l1) <= bound_l and _err(dl, d1) <= bound_d, tag
    print("ce_loss_mix worst", (B, C), worst)


def test_ce_loss_mix_row_losses_and_bad_labels(dev):
    """row_loss [2B] = the y_a losses then the y_b losses (clipk_ce_loss's); a label outside [0, C)
    is not dereferenced and makes that row's loss NaN."""
    g = torch.Generator().manual_seed(9)
    B, C = 6, 37
    logits = (10 * torch.randn(B, C, generator=g)).to(dev)
    y_a = torch.randint(0, C, (B,), generator=g).to(dev)
    y_b = torch.randint(0, C, (B,), generator=g).to(dev)
    alpha = (torch.rand(C, generator=g) + 0.5).to(dev)

    def run(ya, yb, focal):
        row = torch.zeros(2 * B, device=dev)
        loss = torch.zeros((), device=dev)
        dl = torch.zeros_like(logits)
        N.call("clipk_ce_loss_mix", B, C, _p(logits), _p(ya), _p(yb), 0.37, _p(alpha), 2.0, int(focal), 1.0 / B, 1,
               _p(row), _p(loss), _p(dl), _stream())
        return row, loss, dl

    for focal in (False, True):
        row, loss, dl = run(y_a, y_b, focal)
        ra, _ = ops.ce_loss(logits, y_a, alpha, 2.0, focal)
        rb, _ = ops.ce_loss(logits, y_b, alpha, 2.0, focal)
        assert torch.equal(row[:B], ra) and torch.equal(row[B:], rb)
        bad_a, bad_b = y_a.clone(), y_b.clone()
        bad_a[1], bad_b[0], bad_b[4] = C, -1, 1 << 40
        row2, loss2, dl2 = run(bad_a, bad_b, focal)
        torch.cuda.synchronize()  # the run is clean
        nan = torch.isnan(row2)
        assert nan.nonzero().flatten().tolist() == [1, B + 0, B + 4]
        assert torch.equal(row2[~nan], row[~nan])
        assert bool(torch.isnan(loss2))
        rows_ok = [2, 3, 5]
        assert torch.equal(dl2[rows_ok], dl[rows_ok]) and bool(torch.isnan(dl2[[0, 1, 4]]).all())


def test_ce_loss_mix_argument_errors(dev):
    lib = N.load()
    B, C = 3, 5
    logits = torch.randn(B, C).to(dev)
    y = torch.zeros(B, dtype=torch.int64, device=dev)
    row = torch.full((2 * B,), 7.0, device=dev)
    loss = torch.full((), 7.0, device=dev)
    dl = torch.full_like(logits, 7.0)

    def rc(B_, C_, logits_, ya_, yb_, red, row_, loss_):
        return lib.clipk_ce_loss_mix(B_, C_, _p(logits_), _p(ya_), _p(yb_), 0.5, None, 2.0, 0, 1.0, red, _p(row_),
                                     _p(loss_), _p(dl), _stream())

    assert rc(B, C, None, y, y, 1, row, loss) == -1
    assert rc(B, C, logits, None, y, 1, row, loss) == -1
    assert rc(B, C, logits, y, None, 1, row, loss) == -1
    assert rc(B, C, logits, y, y, 1, None, loss) == -1
    assert rc(B, C, logits, y, y, 1, row, None) == -1
    assert rc(B, C, logits, y, y, 0, row, loss) == -1
    assert rc(B, C, logits, y, y, 3, row, loss) == -1
    assert rc(0, C, logits, y, y, 1, row, loss) == -2
    assert rc(-1, C, logits, y, y, 1, row, loss) == -2
    assert rc(B, 0, logits, y, y, 2, row, loss) == -2
    torch.cuda.synchronize()
    assert bool((row == 7.0).all()) and float(loss) == 7.0 and bool((dl == 7.0).all())  # nothing was launched
    assert rc(B, C, logits, y, y, 1, row, loss) == 0
    with pytest.raises(N.ClipkError):
        ops.ce_loss_mix(logits, y, y[:2], 0.5)
    with pytest.raises(N.ClipkError):
        ops.ce_loss_mix(logits, y, y.int(), 0.5)


def test_mixed_cross_entropy_fn_backward(dev):
    """The gradient comes from the forward call; backward_unit's cached 1.0 is passed through, any
    other upstream gradient multiplies it."""
    from fsp_amd.trainers._fns import MixedCrossEntropyFn, backward_unit
    g = torch.Generator().manual_seed(2)
    logits = (4 * torch.randn(5, 11, generator=g)).to(dev)
    y_a = torch.randint(0, 11, (5,), generator=g).to(dev)
    y_b = torch.randint(0, 11, (5,), generator=g).to(dev)
    _, want = ops.ce_loss_mix(logits, y_a, y_b, 0.37)
    z = logits.clone().requires_grad_(True)
    backward_unit(MixedCrossEntropyFn.apply(z, y_a, y_b, 0.37, None, 2.0, False))
    assert torch.equal(z.grad, want)
    z2 = logits.clone().requires_grad_(True)
    (3.0 * MixedCrossEntropyFn.apply(z2, y_a, y_b, 0.37, None, 2.0, False)).backward()
    assert torch.equal(z2.grad, want * 3.0)
    with torch.no_grad():
        loss = MixedCrossEntropyFn.apply(logits, y_a, y_b, 0.37, None, 2.0, False)
    assert torch.equal(loss, ops.ce_loss_mix(logits, y_a, y_b, 0.37, grad=False)[0])


# ------------------------------------------------------------------ the trainer
SHOTS = [4, 1, 2, 1, 3, 1]


def _ivlp_trainer(outdir, native, focal, dm):
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.engine.config import get_cfg_default
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.OUTPUT_DIR = str(outdir)
    cfg.OPTIM.MAX_EPOCH = 2
    cfg.TEST.NO_TEST = True
    cfg.TRAINER.NAME = "IVLP"
    s = cfg.TRAINER.IVLP
    s.PREC = "fp32"
    s.PROMPT_DEPTH_TEXT = s.PROMPT_DEPTH_VISION = 2
    s.USE_FOCAL_LOSS = focal
    if focal:
        cfg.DATASET.PER_CLASS_SHOTS = list(SHOTS)
    cfg.NATIVE.MIXUP = native
    torch.manual_seed(11)  # the prompts' random init, the same for both trainers
    with contextlib.redirect_stdout(io.StringIO()):
        return TRAINER_REGISTRY.get("IVLP")(cfg, dm=dm)


@pytest.mark.parametrize("focal", [False, True])
def test_ivlp_trainer_native_mixup_matches_the_two_call_branch(dev, tmp_path, monkeypatch, focal):
    from fsp_amd.data.synthetic import SyntheticDataManager
    dm = SyntheticDataManager(len(SHOTS), 32, 4, n_batches=2, device=dev, mixup_alpha=1.0,
                              per_class_shots=SHOTS if focal else None)
    assert all({"img", "y_a", "y_b", "lam"} <= set(b) and 0.0 < b["lam"] < 1.0 for b in dm.train_loader_x)
    names = []
    orig = N.call
    monkeypatch.setattr(N, "call", lambda name, *a: names.append(name) or orig(name, *a))
    runs = {}
    for native in (False, True):
        tr = _ivlp_trainer(tmp_path / f"out{int(native)}", native, focal, dm)
        assert tr.model.focal == focal and (tr.model.alpha is not None) == focal
        params = {k: p for k, p in tr.model.named_parameters() if p.requires_grad}
        start = {k: p.detach().cpu().numpy().copy() for k, p in params.items()}
        losses, grads, loss_calls = [], [], []
        fb = tr.forward_backward

        def step(b, fb=fb, losses=losses, grads=grads, loss_calls=loss_calls, params=params):
            n0 = len(names)
            losses.append(float(fb(b)["loss"]))
            loss_calls.append((names[n0:].count("clipk_ce_loss_mix"), names[n0:].count("clipk_ce_loss_reduce")))
            grads.append({k: p.grad.detach().cpu().numpy().copy() for k, p in params.items()})
            return {"loss": losses[-1]}

        tr.forward_backward = step
        with contextlib.redirect_stdout(io.StringIO()):
            for tr.epoch in range(tr.max_epoch):
                tr.run_epoch()
                tr.after_epoch()
        # a mixed step is one clipk_ce_loss_mix and no clipk_ce_loss_reduce; the reverse with the key off
        assert loss_calls == [(1, 0) if native else (0, 2)] * 4, loss_calls
        runs[native] = (np.asarray(losses), grads, start, {k: p.detach().cpu().numpy() for k, p in params.items()})
    (l0, g0, s0, p0), (l1, g1, s1, p1) = runs[False], runs[True]
    assert s0 and all(np.array_equal(s0[k], s1[k]) for k in s0)  # the same initial prompts
    report = {"loss": rel_err(l1, l0), "params": max(rel_err(p1[k], p0[k]) for k in p0),
              "grads": max(rel_err(a[k], b[k]) for a, b in zip(g1, g0) for k in b)}
    print("ivlp mixup trainer focal", focal, "loss off", l0, "on", l1, report)
    for losses in (l0, l1):
        assert len(losses) == 4 and np.isfinite(losses).all() and len(set(losses.tolist())) > 1
    assert any(not np.array_equal(p0[k], s0[k]) for k in p0)  # the prompts move
    assert report["loss"] <= 1e-4
    assert report["params"] <= 1e-4
    assert report["grads"] <= 1e-3


# ------------------------------------------------------------------ the loaders
def _images():
    rs = np.random.RandomState(21)
    return [rs.randint(0, 256, size=(int(rs.randint(60, 301)), int(rs.randint(60, 301)), 3), dtype=np.uint8)
            for _ in range(6)]


def _transform(seed, dev):
    from fsp_amd.data.preprocess import GpuTransform
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (64, 64)
    g = torch.Generator()
    g.manual_seed(seed)
    return GpuTransform(cfg, is_train=True, device=dev, generator=g)


def test_gpu_loader_mixes_after_the_transform(dev):
    from fsp_amd.data.manager import GpuLoader, draw_mix
    images = _images()
    host = [{"img": images[:3], "label": torch.tensor([0, 1, 2]), "n_global": 3, "n_local": 3},
            {"img": images[3:], "label": torch.tensor([3, 4, 0]), "n_global": 3, "n_local": 3}]
    batches = list(GpuLoader(host, _transform(5, dev), dev, mixup_alpha=1.0))
    ref_t = _transform(5, dev)
    for b, h in zip(batches, host):
        x = ref_t(h["img"])  # the batch's crop draws, then lam, then the permutation
        lam, perm = draw_mix(1.0, 3, ref_t.generator)
        assert type(b["lam"]) is float and b["lam"] == lam and 0.0 < lam < 1.0
        assert b["img"].device.type == "cuda" and b["img"].shape == (3, 3, 64, 64)
        assert torch.equal(b["img"], lam * x + (1 - lam) * x[perm.to(dev)])
        assert torch.equal(b["label"].cpu(), h["label"]) and b["y_a"] is b["label"]
        assert torch.equal(b["y_b"].cpu(), h["label"][perm])
    plain = list(GpuLoader(host, _transform(5, dev), dev))
    assert all(not {"y_a", "y_b", "lam"} & set(b) for b in plain)


def _data_manager(native, dev):
    from fsp_amd.data.fewshot import Datum
    from fsp_amd.data.manager import DataManager
    from fsp_amd.engine.config import get_cfg_default
    images = _images()
    cfg = get_cfg_default()  # USE_MIXUP True, MIXUP_ALPHA 1.0 as the reference's defaults
    cfg.INPUT.SIZE = (64, 64)
    cfg.TRAINER.NAME = "IVLP"
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 3
    cfg.DATALOADER.TRAIN_X.SAMPLER = "SequentialSampler"
    cfg.NATIVE.MIXUP = native

    class DS:
        train_x = [Datum(impath=str(i), label=i % 4, classname=f"c{i % 4}") for i in range(6)]
        test = train_x
        classnames = [f"c{i}" for i in range(4)]
        lab2cname = {i: f"c{i}" for i in range(4)}
        num_classes = 4

    return DataManager(cfg, DS, dev, reader=lambda path: images[int(path)], num_workers=0)


def test_data_manager_mixes_only_with_the_key(dev):
    from fsp_amd.data.synthetic import SyntheticDataManager
    torch.manual_seed(3)  # augment_generator seeds from torch's seed: both managers draw the same crops
    off = list(_data_manager(False, dev).train_loader_x)
    on = list(_data_manager(True, dev).train_loader_x)
    assert len(off) == len(on) == 2
    for a, b in zip(off, on):
        assert "y_a" not in a and "y_b" not in a and "lam" not in a  # default config: nothing mixes
        assert {"img", "label", "y_a", "y_b", "lam"} <= set(b)
        assert torch.equal(a["label"], b["label"]) and torch.equal(b["y_a"], b["label"])
        lam = b["lam"]
        assert type(lam) is float and 0.0 < lam < 1.0
        # the first batch's crops precede every mix draw: its mix is of exactly the key-off images
        if a is off[0]:
            perms = [torch.tensor(q) for q in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))]
            assert any(torch.equal(b["img"], lam * a["img"] + (1 - lam) * a["img"][q.to(dev)])
                       and torch.equal(b["y_b"], a["label"][q.to(dev)]) for q in perms)
    for b in _data_manager(True, dev).test_loader:
        assert "y_a" not in b  # evaluation does not change
    assert all("y_a" not in b for b in SyntheticDataManager(4, 32, 2, n_batches=1, device=dev).train_loader_x)
