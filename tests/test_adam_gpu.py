"""The fused Adam / AdamW / AMSGrad step (clipk_adam_step_multi, ops.adam_step_multi,
engine.optim.FusedAdam) on the GPU against the installed torch.optim.

The reference is torch.optim.Adam / AdamW in float64 on the CPU. The tolerance is measured, not
fixed: the kernel's largest absolute deviation from the float64 run may be at most ``SLACK`` = 4
times the deviation of the same torch optimizer run in float32 on the CPU on the same inputs (FMA
contraction and another operation order are within that; a wrong bias correction, decay or step
count is orders of magnitude outside it). The same rule holds for the optimizer state.
"""
import contextlib
import ctypes
import io
import os
import sys

import pytest
import torch

from parity_util import load_fixture

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

SLACK = 4.0
LR, BETAS, EPS, WD = 2e-3, (0.9, 0.999), 1e-8, 5e-4
STEPS = 12
GRID_CAP = 2048  # csrc/optim.hip kAdamGridCap: blocks per tensor; one grid pass = GRID_CAP * 256 accesses
BIG = GRID_CAP * 256 * 4 + 5  # 16-byte accesses: more than one pass, and a one-by-one tail
BIG_VIEW = GRID_CAP * 256 + 3  # the misaligned view goes one element per access: more than one pass
SIZES = [1, 3, 255, 256, 257, 1027, 2048, BIG, 5, 64, 511, 512, 513, 1024, 4099, 100]  # + the view = 17
ZEROS_AT = 5  # this tensor's gradient has exact zeros
MODES = {"adam": (torch.optim.Adam, {}), "amsgrad": (torch.optim.Adam, {"amsgrad": True}),
         "adamw": (torch.optim.AdamW, {})}
STATE = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _grads(sizes, steps, seed):
    """Per step and tensor: random signs, magnitudes spread log-uniformly over 1e-6..1."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        gs = []
        for k, n in enumerate(sizes):
            mag = torch.pow(10.0, -6.0 * torch.rand(n, generator=gen))
            g = mag * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
            if k == ZEROS_AT:
                g[::3] = 0.0
            gs.append(g.float())
        out.append(gs)
    return out


def _params(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [0.1 * torch.randn(n, generator=gen) for n in sizes]


def _torch_run(mode, p0, grads, dtype):
    cls, kw = MODES[mode]
    ps = [p.to(dtype).clone().requires_grad_(True) for p in p0]
    opt = cls(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, **kw)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.to(dtype)
        opt.step()
    state = {k: [opt.state[p][k].detach() for p in ps] for k in STATE if k in opt.state[ps[0]]}
    return [p.detach() for p in ps], state


class _Dev:
    """A param group on the device for ops.adam_step_multi: the last tensor of ``p0`` becomes a
    [1:] view of a flat buffer (4 bytes past a 16-byte boundary)."""

    def __init__(self, mode, p0, dev, view_last=True):
        self.mode = mode
        self.p = [p.to(dev) for p in p0]
        if view_last:
            flat = torch.zeros(p0[-1].numel() + 1, device=dev)
            self.p[-1] = flat[1:]
            self.p[-1].copy_(p0[-1])
            assert self.p[-1].data_ptr() % 16 == 4 and self.p[-1].is_contiguous()
        self.m = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.p]
        self.v = [torch.zeros_like(m) for m in self.m]
        self.vmax = [torch.zeros_like(m) for m in self.m] if mode == "amsgrad" else None
        self.steps = [torch.zeros(2, dtype=torch.int32, device=dev) for _ in self.p]
        self.parity = [0] * len(self.p)
        self.dev = dev

    def step(self, gs, **kw):
        from fsp_amd import ops
        ops.adam_step_multi(self.p, [g.to(self.dev) for g in gs], self.m, self.v, self.vmax, self.steps,
                            self.parity, LR, BETAS[0], BETAS[1], EPS, WD, self.mode, **kw)
        self.parity = [q ^ 1 for q in self.parity]

    def counts(self):
        return [int(s[q]) for s, q in zip(self.steps, self.parity)]

    def snapshot(self):
        t = {"p": self.p, "exp_avg": self.m, "exp_avg_sq": self.v}
        if self.vmax is not None:
            t["max_exp_avg_sq"] = self.vmax
        return {k: [x.detach().cpu().clone() for x in v] for k, v in t.items()}, self.counts()


def _maxdev(xs, refs):
    return max(float((x.double().cpu() - r).abs().max()) for x, r in zip(xs, refs))


def _assert_bitwise(a, b):
    assert a[1] == b[1], (a[1], b[1])
    for k in a[0]:
        for i, (x, y) in enumerate(zip(a[0][k], b[0][k])):
            assert torch.equal(x, y), (k, i)


@pytest.fixture(scope="module")
def inputs():
    sizes = SIZES + [BIG_VIEW]
    assert len(sizes) == 17  # two launches
    return _params(sizes, 11), _grads(sizes, STEPS, 12)


@pytest.mark.parametrize("mode", ["adam", "adamw", "amsgrad"])
def test_kernel_matches_torch(dev, inputs, mode):
    p0, grads = inputs
    ref_p, ref_s = _torch_run(mode, p0, grads, torch.float64)
    t32_p, t32_s = _torch_run(mode, p0, grads, torch.float32)
    d = _Dev(mode, p0, dev)
    for gs in grads:
        d.step(gs)
    torch.cuda.synchronize()
    got, counts = d.snapshot()
    assert counts == [STEPS] * 17
    assert set(got) == {"p"} | set(ref_s)
    for name, refs, t32 in [("p", ref_p, t32_p)] + [(k, ref_s[k], t32_s[k]) for k in ref_s]:
        margin = _maxdev(t32, refs)
        mine = _maxdev(got[name], refs)
        print(f"adam kernel [{mode}] {name}: |kernel - f64| {mine:.3e}, |torch f32 - f64| {margin:.3e}, "
              f"ratio {mine / margin:.2f}")
        assert margin > 0 and mine <= SLACK * margin, (name, mine, margin)
    # per tensor as well, the parameters: a fault in one small tensor must not hide under the
    # margin of the largest
    for k, (x, r, t) in enumerate(zip(got["p"], ref_p, t32_p)):
        margin = max(float((t.double() - r).abs().max()), float(r.abs().max()) * 2.0 ** -24)  # (>= half an ulp)
        assert float((x.double() - r).abs().max()) <= SLACK * margin, (k, x.numel())


SMALL = [1, 3, 255, 257, 1027, 2048, 4099]


@pytest.mark.parametrize("mode", ["adam", "adamw", "amsgrad"])
def test_grad_scale_is_bitwise(dev, mode):
    """A power-of-two grad_scale is bitwise the update on pre-scaled gradients -- 0.125 * g against
    the unscaled kernel on the exactly scaled g / 8 -- and, the other way round, the unscaled entry
    on g against the scaled kernel at 0.125 on 8 g; grad_scale = 1.0 is the unscaled entry."""
    p0, grads = _params(SMALL, 21), _grads(SMALL, 3, 22)
    runs = {}
    for name, mul, kw in (("plain", 1.0, {}), ("one", 1.0, {"grad_scale": 1.0}),
                          ("scaled_on_8g", 8.0, {"grad_scale": 0.125}),
                          ("scaled", 1.0, {"grad_scale": 0.125}), ("prescaled", 0.125, {})):
        d = _Dev(mode, p0, dev)
        for gs in grads:
            d.step([g * mul for g in gs], **kw)
        runs[name] = d.snapshot()
    _assert_bitwise(runs["one"], runs["plain"])
    _assert_bitwise(runs["scaled_on_8g"], runs["plain"])
    _assert_bitwise(runs["scaled"], runs["prescaled"])
    assert not torch.equal(runs["scaled"][0]["p"][-1], runs["plain"][0]["p"][-1])


@pytest.mark.parametrize("mode", ["adam", "adamw", "amsgrad"])
def test_guard_skips_update_and_count(dev, mode):
    """flags = 2 with mask 2 on what would be step 3: p, m, v, vmax and the count bitwise
    unchanged; the next unguarded step is what step 3 would have been (the count did not
    advance). A flag bit outside the mask does not skip."""
    sizes = SMALL + list(range(10, 20))  # 17 tensors: the skip holds in both launches
    p0, grads = _params(sizes, 31), _grads(sizes, 3, 32)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    want = _Dev(mode, p0, dev)
    flags.fill_(1)
    for gs in grads:
        want.step(gs, guard=(flags, 2))
    assert want.counts() == [3] * 17
    d = _Dev(mode, p0, dev)
    flags.zero_()
    for gs in grads[:2]:
        d.step(gs, guard=(flags, 2))
    before = d.snapshot()
    assert before[1] == [2] * 17
    flags.fill_(2)
    d.step(grads[2], guard=(flags, 2))
    _assert_bitwise(d.snapshot(), before)
    flags.zero_()
    d.step(grads[2], guard=(flags, 2))
    _assert_bitwise(d.snapshot(), want.snapshot())


def _fused(mode, p0, dev):
    from fsp_amd.engine.optim import FusedAdam
    ps = [torch.nn.Parameter(p.to(dev)) for p in p0]
    return ps, FusedAdam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, amsgrad=mode == "amsgrad",
                         decoupled=mode == "adamw")


def _fused_step(ps, opt, gs, **kw):
    for p, g in zip(ps, gs):
        p.grad = g.to(p.device)
    opt.step(**kw)


def _fused_snapshot(ps, opt):
    sd = opt.state_dict()["state"]
    out = {"p": [p.detach().cpu().clone() for p in ps]}
    for k in STATE:
        if sd and k in sd[0]:
            out[k] = [sd[i][k].detach().cpu().clone() for i in range(len(ps))]
    return out, [float(sd[i]["step"]) for i in range(len(ps))] if sd else []


@pytest.mark.parametrize("mode", ["adam", "adamw", "amsgrad"])
def test_fused_adam_step_guard_and_state(dev, mode):
    """FusedAdam.step(guard=...): a skipped first step creates state that is fresh state, whether
    the caller pops the parameters in ``created_last`` (as CoCoOp's deferred check does) or not; a
    skipped third step leaves parameters, state and the exported ``step`` alone. The class drives
    the kernel exactly as the ops-level run (17 parameters, two launches)."""
    sizes = SMALL + list(range(10, 20))
    p0, grads = _params(sizes, 31), _grads(sizes, 3, 32)
    raw = _Dev(mode, p0, dev, view_last=False)
    for gs in grads:
        raw.step(gs)
    want = raw.snapshot()
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    for pop in (True, False):
        ps, opt = _fused(mode, p0, dev)
        gen0 = [getattr(p, "_clipk_gen", 0) for p in ps]
        flags.fill_(2)
        _fused_step(ps, opt, grads[0], guard=(flags, 2))
        assert [id(p) for p in opt.created_last] == [id(p) for p in ps]
        snap = _fused_snapshot(ps, opt)
        assert snap[1] == [0.0] * 17 and all(torch.equal(x, y) for x, y in zip(snap[0]["p"], p0))
        assert all(not bool(x.any()) for k in snap[0] if k != "p" for x in snap[0][k])
        if pop:
            for p in opt.created_last:
                opt.state.pop(p, None)
        flags.zero_()
        _fused_step(ps, opt, grads[0], guard=(flags, 2))
        assert len(opt.created_last) == (17 if pop else 0)
        _fused_step(ps, opt, grads[1])
        before = _fused_snapshot(ps, opt)
        assert before[1] == [2.0] * 17
        flags.fill_(2)
        _fused_step(ps, opt, grads[2], guard=(flags, 2))
        _assert_bitwise(_fused_snapshot(ps, opt), before)
        flags.zero_()
        _fused_step(ps, opt, grads[2], guard=(flags, 2))
        got = _fused_snapshot(ps, opt)
        _assert_bitwise((got[0], [int(c) for c in got[1]]), want)
        assert [getattr(p, "_clipk_gen", 0) - g for p, g in zip(ps, gen0)] == [5] * 17  # bumped per call
        sd = opt.state_dict()["state"][0]
        assert sd["step"].dtype == torch.float32 and sd["step"].dim() == 0
        assert list(sd) == ["step", "exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if mode == "amsgrad" else [])


def test_fused_adam_grad_scale_tag_and_errors(dev):
    """``defer_grad_scale`` tags are honoured (bitwise the pre-scaled step) and consumed; the step
    refuses what FusedSGD refuses."""
    from fsp_amd.engine.optim import FusedAdam
    p0, grads = _params(SMALL, 41), _grads(SMALL, 2, 42)
    a_ps, a = _fused("adam", p0, dev)
    b_ps, b = _fused("adam", p0, dev)
    for gs in grads:
        for p, g in zip(a_ps, gs):
            p.grad = g.to(dev)
        a.defer_grad_scale([p.grad for p in a_ps], 0.25)
        a.step()
        assert not any(hasattr(p.grad, "_clipk_grad_scale") for p in a_ps)
        _fused_step(b_ps, b, [g * 0.25 for g in gs])
    _assert_bitwise(_fused_snapshot(a_ps, a), _fused_snapshot(b_ps, b))
    p = torch.nn.Parameter(torch.zeros(4, dtype=torch.float16, device=dev))
    p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError, match="fp32"):
        FusedAdam([p]).step()
    q = torch.nn.Parameter(torch.zeros(4, device=dev))
    q.grad = torch.zeros_like(q)
    opt = FusedAdam([q])
    opt.param_groups[0]["maximize"] = True
    with pytest.raises(ValueError, match="maximize"):
        opt.step()


@pytest.mark.parametrize("mode", ["adam", "adamw", "amsgrad"])
def test_state_passes_through_torch_and_back(dev, mode):
    """3 fused steps, the state dict loaded into the torch optimizer, its state dict loaded into a
    new FusedAdam, 3 more steps: bitwise the 6 steps in one go (the loaded ``step`` goes back to
    the device; a wrong count would change the bias corrections)."""
    cls, kw = MODES[mode]
    p0, grads = _params(SMALL, 51), _grads(SMALL, 6, 52)
    a_ps, a = _fused(mode, p0, dev)
    for gs in grads:
        _fused_step(a_ps, a, gs)
    b_ps, b = _fused(mode, p0, dev)
    for gs in grads[:3]:
        _fused_step(b_ps, b, gs)
    t = cls([torch.nn.Parameter(p.detach().clone()) for p in b_ps], **kw)
    t.load_state_dict(b.state_dict())
    assert [float(t.state[p]["step"]) for p in t.param_groups[0]["params"]] == [3.0] * len(SMALL)
    assert t.param_groups[0]["lr"] == LR and t.param_groups[0]["betas"] == BETAS
    c_ps, c = _fused(mode, [p.detach().cpu() for p in b_ps], dev)
    c.load_state_dict(t.state_dict())
    for gs in grads[3:]:
        _fused_step(c_ps, c, gs)
    _assert_bitwise(_fused_snapshot(c_ps, c), _fused_snapshot(a_ps, a))
    assert _fused_snapshot(a_ps, a)[1] == [6.0] * len(SMALL)


def test_bad_arguments_are_refused_before_any_launch(dev):
    from fsp_amd import _native as N
    lib = N.load()
    d = _Dev("adam", _params([8] * 17, 61), dev, view_last=False)
    g = [torch.ones(8, device=dev) for _ in range(17)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(count=1, p=d.p, beta1=0.9, beta2=0.999, eps=1e-8, mode=N.ADAM_ADAM, vmax=None, parity=0):
        VP = ctypes.c_void_p * 17
        arr = lambda ts: None if ts is None else VP(*[t.data_ptr() if t is not None else 0 for t in ts])
        return lib.clipk_adam_step_multi(count, arr(p), arr(g), arr(d.m), arr(d.v), arr(vmax),
                                         (ctypes.c_long * 17)(*[8] * 17), arr(d.steps),
                                         (ctypes.c_int * 17)(*[parity] * 17), LR, beta1, beta2, eps, WD, mode, 1.0,
                                         None, 0, stream)

    EINVAL = -1
    assert call(count=0) == EINVAL and call(count=17) == EINVAL and call(count=-1) == EINVAL
    assert call(p=None) == EINVAL and call(p=[None] + d.p[1:]) == EINVAL
    assert call(beta1=1.0) == EINVAL and call(beta2=1.0) == EINVAL and call(beta1=-0.1) == EINVAL
    assert call(eps=-1e-8) == EINVAL and call(mode=3) == EINVAL and call(mode=-1) == EINVAL
    assert call(mode=N.ADAM_AMSGRAD, vmax=None) == EINVAL and call(parity=2) == EINVAL
    torch.cuda.synchronize()
    assert d.counts() == [0] * 17 and all(not bool(m.any()) for m in d.m)
    assert call(count=16) == 0  # and the same call within the limits runs
    torch.cuda.synchronize()
    assert [int(s[1]) for s in d.steps] == [1] * 16 + [0]


# ---------------------------------------------------------------- trainers
def _setup(trainer, outdir, dev, optim, prec=None, native=None):
    """The tiny trainer of tests/test_trainer_gpu.py (_setup), with OPTIM overrides."""
    import make_golden_trainer as MT
    from fsp_amd.clip import synth
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    import fsp_amd.trainers  # noqa: F401
    cfg = MT.make_cfg(trainer, str(outdir))
    cfg.TEST.NO_TEST = True
    cfg.NATIVE.COCOOP_SHARD = "image"
    if prec is not None:
        getattr(cfg.TRAINER, trainer.upper()).PREC = prec
    for k, v in (native or {}).items():
        cfg.NATIVE[k] = v
    for k, v in optim.items():
        cfg.OPTIM[k] = v
    names = synth.synthetic_classnames(MT.N_CLS)
    train, test = MT.batches()
    mv = lambda b: {k: v.to(dev) for k, v in b.items()}

    class DM:
        class dataset:
            classnames = names
            lab2cname = {i: n for i, n in enumerate(names)}
        train_loader_x = [mv(b) for b in train]
        test_loader = [mv(b) for b in test]
        val_loader = None

    with contextlib.redirect_stdout(io.StringIO()):
        tr = TRAINER_REGISTRY.get(trainer)(cfg, dm=DM())
    meta, ref = load_fixture(f"trainer_{trainer.lower()}")
    pl = tr.model.prompt_learner
    a = synth.ARCHS["tiny"]
    with torch.no_grad():
        pl.ctx.copy_(torch.from_numpy(ref["ctx0"]).to(dev))
        if trainer == "CoCoOp":
            for k, v in synth.make_meta_net(a.embed_dim, a.transformer_width, seed=4).items():
                dict(pl.named_parameters())[k].copy_(torch.from_numpy(v).to(dev))
    return tr, cfg


def _three_steps(tr):
    """2 batches of epoch 0 (constant warmup LR), the LR update, 1 batch of epoch 1."""
    tr.max_epoch = 2
    tr.epoch = 0
    tr.run_epoch()
    tr.dm.train_loader_x = tr.dm.train_loader_x[:1]
    tr.epoch = 1
    tr.run_epoch()
    torch.cuda.synchronize()
    return {k: p.detach().cpu().clone() for k, p in tr.model.prompt_learner.named_parameters()}


OPTIM = {"LR_SCHEDULER": "multi_step", "STEPSIZE": (1,), "GAMMA": 0.5}


@pytest.mark.parametrize("name", ["adam", "adamw"])
@pytest.mark.parametrize("trainer", ["CoOp", "CoCoOp"])
def test_trainer_matches_torch_optimizer(dev, tmp_path, trainer, name):
    """OPTIM.NAME adam / adamw with LR_SCHEDULER multi_step, 3 steps across an epoch boundary,
    against the same trainer with torch.optim.Adam / AdamW over the same parameters. The margin is
    measured as above: the torch trainer's gradients and LRs, replayed through the torch optimizer
    in float64 on the CPU, are the reference, and the torch trainer's own (float32) distance from
    it the margin."""
    from fsp_amd.engine.optim import FusedAdam, build_lr_scheduler
    cls = MODES[name][0]
    fused, cfg = _setup(trainer, tmp_path / "a", dev, dict(OPTIM, NAME=name))
    assert isinstance(fused.optim, FusedAdam) and fused.optim._mode(fused.optim.param_groups[0]) == name
    got = _three_steps(fused)
    lrs_fused = fused.get_current_lr()

    theirs, _ = _setup(trainer, tmp_path / "b", dev, dict(OPTIM, NAME=name))
    pl = theirs.model.prompt_learner
    params = [p for p in pl.parameters() if p.requires_grad]
    names = [k for k, p in pl.named_parameters() if p.requires_grad]
    o = cfg.OPTIM
    kw = dict(lr=o.LR, betas=(o.ADAM_BETA1, o.ADAM_BETA2), weight_decay=o.WEIGHT_DECAY)
    theirs.optim = cls(params, **kw)
    theirs.sched = build_lr_scheduler(theirs.optim, o)
    theirs._optims["prompt_learner"], theirs._scheds["prompt_learner"] = theirs.optim, theirs.sched
    p0 = [p.detach().double().cpu().clone() for p in params]
    tape = []
    step = theirs.optim.step
    theirs.optim.step = lambda *a, **k: tape.append(([p.grad.detach().double().cpu() for p in params],
                                                     theirs.optim.param_groups[0]["lr"])) or step(*a, **k)
    want = _three_steps(theirs)
    assert len(tape) == 3 and [lr for _, lr in tape] == [1e-5, 1e-5, 0.002]
    assert theirs.get_current_lr() == lrs_fused == 0.001  # the milestone at epoch 1 of the successor's count

    ref = [p.clone().requires_grad_(True) for p in p0]
    opt64 = cls(ref, **kw)
    for gs, lr in tape:
        opt64.param_groups[0]["lr"] = lr
        for p, g in zip(ref, gs):
            p.grad = g
        opt64.step()
    for k, r in zip(names, ref):
        margin = float((want[k].double() - r.detach()).abs().max())
        mine = float((got[k].double() - r.detach()).abs().max())
        moved = float((r.detach() - p0[names.index(k)]).abs().max())
        print(f"{trainer} {name} {k}: |fused - f64| {mine:.3e}, |torch f32 - f64| {margin:.3e}, moved {moved:.3e}")
        assert moved > 1e-4  # (the steps did move the parameter: ~ LR per element at the last step)
        assert mine <= SLACK * margin, (k, mine, margin)


def _fp32s_adam_run(dev, outdir, defer, target=None, monkeypatch=None):
    from fsp_amd.clip.model import TextEncoderCore
    if target is not None:
        monkeypatch.setattr(TextEncoderCore, "SPLIT_TARGET", target)
    tr, _ = _setup("CoCoOp", outdir, dev, dict(OPTIM, NAME="adam"), prec="fp32s",
                   native={"DEFER_SPLIT_CHECK": defer})
    params = _three_steps(tr)
    assert tr.model.text_core.defer_check is defer
    sd = tr.optim.state_dict()["state"]
    state = [sd[i][k].detach().cpu().clone() for i in sorted(sd) for k in ("step", "exp_avg", "exp_avg_sq")]
    return params, state, tr.get_current_lr()


def test_cocoop_fp32s_deferred_check_with_adam(dev, tmp_path, monkeypatch):
    """PREC fp32s CoCoOp with FusedAdam takes the deferred overflow check (core.defer_check) and
    trains bitwise as with the check inside the backward; with every step forced to overflow
    (scale target 2^20) each step is skipped on the device -- state created, count not advanced --
    and re-run to the same bits as the in-backward retry."""
    from fsp_amd.trainers.cocoop import CoCoOp
    a = _fp32s_adam_run(dev, tmp_path / "a", False)
    b = _fp32s_adam_run(dev, tmp_path / "b", True)
    d0 = CoCoOp.deferred_redos
    c = _fp32s_adam_run(dev, tmp_path / "c", False, 20, monkeypatch)
    d = _fp32s_adam_run(dev, tmp_path / "d", True, 20, monkeypatch)
    assert CoCoOp.deferred_redos == d0 + 3
    for x, y in ((a, b), (c, d)):
        assert x[2] == y[2]
        for k in x[0]:
            assert torch.equal(x[0][k], y[0][k]), k
        assert all(torch.equal(s, t) for s, t in zip(x[1], y[1]))
        assert [float(s) for s in x[1][0::3]] == [3.0] * (len(x[1]) // 3)
