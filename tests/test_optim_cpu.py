"""CPU: the Adam-family optimizers and the step LR schedules, host side (no GPU compute).

* ``build_optimizer`` maps OPTIM.NAME adam / amsgrad / adamw to ``FusedAdam`` in the right mode
  and keeps raising for the rest;
* a ``FusedAdam`` state dict and a ``torch.optim.Adam`` / ``AdamW`` one load into each other
  (construction and ``load_state_dict`` need no GPU; ``step`` does);
* ``single_step`` / ``multi_step`` give the LR sequence of torch ``StepLR`` / ``MultiStepLR`` driven
  as Dassl drives them: under its Constant / LinearWarmupScheduler (re-stated below from Dassl's
  lr_scheduler.py, over the installed torch's scheduler base class), with and without
  WARMUP_RECOUNT, and resume from a state dict.

LRs are compared to rtol 1e-12: doubles, and the two sides differ at most in the order of a
handful of multiplications (a few ulp of 2.2e-16 each).
"""
import copy
import warnings

import pytest
import torch
from torch.optim.lr_scheduler import LRScheduler, MultiStepLR, StepLR

from fsp_amd.engine.config import get_cfg_default
from fsp_amd.engine.optim import FusedAdam, FusedSGD, build_lr_scheduler, build_optimizer

MODES = {"adam": (torch.optim.Adam, {}), "amsgrad": (torch.optim.Adam, {"amsgrad": True}),
         "adamw": (torch.optim.AdamW, {})}


def _module():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2, bias=False))


def test_config_defaults_carry_the_adam_and_step_keys():
    o = get_cfg_default().OPTIM
    assert (o.ADAM_BETA1, o.ADAM_BETA2, o.STEPSIZE, o.GAMMA) == (0.9, 0.999, (-1,), 0.1)
    assert (o.NAME, o.LR_SCHEDULER) == ("sgd", "cosine")


@pytest.mark.parametrize("name", ["adam", "amsgrad", "adamw"])
def test_build_optimizer_modes(name):
    cfg = get_cfg_default()
    cfg.OPTIM.NAME = name
    cfg.OPTIM.ADAM_BETA1, cfg.OPTIM.ADAM_BETA2 = 0.8, 0.99
    m = _module()
    opt = build_optimizer(m, cfg.OPTIM)
    assert isinstance(opt, FusedAdam) and hasattr(opt, "created_last") and hasattr(opt, "defer_grad_scale")
    g, = opt.param_groups
    assert opt._mode(g) == name
    assert g["lr"] == cfg.OPTIM.LR and g["weight_decay"] == cfg.OPTIM.WEIGHT_DECAY and g["betas"] == (0.8, 0.99)
    assert g["amsgrad"] == (name == "amsgrad") and g["eps"] == 1e-8
    assert [id(p) for p in g["params"]] == [id(p) for p in m.parameters()]
    # every key of the installed torch's group, so that state dicts load both ways
    cls, kw = MODES[name]
    assert set(g) == set(cls(m.parameters(), **kw).param_groups[0])


def test_build_optimizer_sgd_unchanged_and_rest_raises():
    cfg = get_cfg_default()
    assert isinstance(build_optimizer(_module(), cfg.OPTIM), FusedSGD)
    for name in ("rmsprop", "radam"):
        cfg.OPTIM.NAME = name
        with pytest.raises(NotImplementedError, match="adam"):  # the message names what exists
            build_optimizer(_module(), cfg.OPTIM)
    with pytest.raises(ValueError):
        FusedAdam(_module().parameters(), amsgrad=True, decoupled=True)


def test_fused_adam_has_no_cpu_path():
    m = _module()
    opt = FusedAdam(m.parameters())
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="GPU only"):
        opt.step()


def _torch_run(cls, kw, params, steps, seed=1):
    opt = cls(params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4, **kw)
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return opt


def _assert_state_equal(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert list(a["state"][k]) == list(b["state"][k])  # the same keys in torch's order
        for n, v in a["state"][k].items():
            w = b["state"][k][n]
            assert v.dtype == w.dtype and v.shape == w.shape and torch.equal(v, w), (k, n)


@pytest.mark.parametrize("name", ["adam", "amsgrad", "adamw"])
def test_state_dict_round_trip_with_torch(name):
    cls, kw = MODES[name]
    kwf = dict(amsgrad=name == "amsgrad", decoupled=name == "adamw")
    params = [p.detach().clone().requires_grad_(True) for p in _module().parameters()]
    ref = _torch_run(cls, kw, params, 3)
    sd = copy.deepcopy(ref.state_dict())  # (load_state_dict keeps the tensors it is given)
    assert float(sd["state"][0]["step"]) == 3.0 and sd["state"][0]["step"].dtype == torch.float32

    # torch -> FusedAdam: loads, and presents the same state again
    mine = [p.detach().clone().requires_grad_(True) for p in params]
    fused = FusedAdam(mine, lr=1.0, betas=(0.5, 0.5), weight_decay=0.0, **kwf)  # (all replaced by the load)
    fused.load_state_dict(sd)
    assert fused._mode(fused.param_groups[0]) == name
    _assert_state_equal(fused.state_dict(), sd)

    # FusedAdam -> torch: a torch optimizer loaded from it goes on exactly as the original
    theirs = [p.detach().clone().requires_grad_(True) for p in params]
    back = cls(theirs, **kw)
    back.load_state_dict(copy.deepcopy(fused.state_dict()))
    for ps, opt in ((params, ref), (theirs, back)):
        gen = torch.Generator().manual_seed(7)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    for p, q in zip(params, theirs):
        assert torch.equal(p, q)
    _assert_state_equal(back.state_dict(), ref.state_dict())

    # a FusedAdam that never stepped: empty state, and torch takes it
    fresh = FusedAdam([p.detach().clone().requires_grad_(True) for p in params], **kwf).state_dict()
    assert fresh["state"] == {}
    cls([p.detach().clone().requires_grad_(True) for p in params], **kw).load_state_dict(fresh)


# ---------------------------------------------------------------- LR schedules
class _Warmup(LRScheduler):
    """Dassl's _BaseWarmupScheduler with its Constant (cons_lr) / Linear (min_lr) get_lr."""

    def __init__(self, optimizer, successor, warmup_epoch, cons_lr=None, min_lr=None):
        self.successor, self.warmup_epoch, self.cons_lr, self.min_lr = successor, warmup_epoch, cons_lr, min_lr
        super().__init__(optimizer, -1)

    def get_lr(self):
        if self.last_epoch >= self.warmup_epoch:
            return self.successor.get_last_lr()
        if self.cons_lr is not None:
            return [self.cons_lr for _ in self.base_lrs]
        if self.last_epoch == 0:
            return [self.min_lr for _ in self.base_lrs]
        return [lr * self.last_epoch / self.warmup_epoch for lr in self.base_lrs]

    def step(self, epoch=None):
        if self.last_epoch >= self.warmup_epoch:
            self.successor.step(epoch)
            self._last_lr = self.successor.get_last_lr()
        else:
            super().step(epoch)


def _sched_cfg(sched, stepsize, warmup, recount):
    o = get_cfg_default().OPTIM
    o.LR_SCHEDULER, o.STEPSIZE, o.GAMMA, o.MAX_EPOCH, o.LR = sched, stepsize, 0.1, 10, 0.002
    o.WARMUP_EPOCH, o.WARMUP_TYPE = (2, warmup) if warmup else (-1, "linear")
    o.WARMUP_CONS_LR, o.WARMUP_MIN_LR, o.WARMUP_RECOUNT = 1e-5, 3e-5, recount
    return o


def _dassl_scheduler(opt, o):
    """Dassl's build_lr_scheduler for single_step / multi_step, on torch's own schedulers."""
    if o.LR_SCHEDULER == "single_step":
        size = o.STEPSIZE[-1] if o.STEPSIZE[-1] > 0 else o.MAX_EPOCH
        s = StepLR(opt, step_size=size, gamma=o.GAMMA)
    else:
        s = MultiStepLR(opt, milestones=list(o.STEPSIZE), gamma=o.GAMMA)
    if o.WARMUP_EPOCH > 0:
        if not o.WARMUP_RECOUNT:
            s.last_epoch = o.WARMUP_EPOCH
        if o.WARMUP_TYPE == "constant":
            s = _Warmup(opt, s, o.WARMUP_EPOCH, cons_lr=o.WARMUP_CONS_LR)
        else:
            s = _Warmup(opt, s, o.WARMUP_EPOCH, min_lr=o.WARMUP_MIN_LR)
    return s


def _sgd(lr):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)


EPOCHS = 12


@pytest.mark.parametrize("recount", [True, False])
@pytest.mark.parametrize("warmup", [None, "constant", "linear"])
@pytest.mark.parametrize("stepsize", [(-1,), (4,), (3, 7)])
@pytest.mark.parametrize("sched", ["single_step", "multi_step"])
def test_step_schedules_match_torch(sched, stepsize, warmup, recount):
    o = _sched_cfg(sched, stepsize, warmup, recount)
    with warnings.catch_warnings():  # (no optimizer.step() between the scheduler steps)
        warnings.simplefilter("ignore")
        ref_opt = _sgd(o.LR)
        ref = _dassl_scheduler(ref_opt, o)
        want, succ = [], []
        for _ in range(EPOCHS):
            want.append(ref_opt.param_groups[0]["lr"])
            succ.append((getattr(ref, "successor", ref).last_epoch, getattr(ref, "successor", ref).get_last_lr()))
            ref.step()
    opt = _sgd(o.LR)
    mine = build_lr_scheduler(opt, o)
    got = []
    for e in range(EPOCHS):
        assert mine.get_last_lr() == [opt.param_groups[0]["lr"]]
        got.append(opt.param_groups[0]["lr"])
        if e == 5:  # resume at epoch 5: a fresh scheduler loaded from the state goes on the same way
            sd = mine.state_dict()
            opt = _sgd(o.LR)
            mine = build_lr_scheduler(opt, o)
            mine.load_state_dict(sd)
            assert mine.last_epoch == 5 and opt.param_groups[0]["lr"] == got[-1]
            # ... and the state has Dassl's shape: the torch scheduler (with warmup, as the
            # wrapper's successor) at the reference's epoch and LR
            t = sd["successor"].state_dict() if warmup else sd
            assert t["last_epoch"] == succ[5][0] and t["_last_lr"] == pytest.approx(succ[5][1], rel=1e-12)
            assert ("step_size" in t) == (sched == "single_step") and ("milestones" in t) == (sched == "multi_step")
            if warmup:
                assert sd["warmup_epoch"] == 2 and sd["last_epoch"] == 2
                assert ("cons_lr" in sd) == (warmup == "constant") and ("min_lr" in sd) == (warmup == "linear")
        mine.step()
    assert got == pytest.approx(want, rel=1e-12), (got, want)
    # the cases do decay (except with STEPSIZE -1, where at most MAX_EPOCH counts): the comparison
    # is not of constants
    if stepsize != (-1,):
        assert min(got[2:]) < 0.5 * o.LR


def test_torch_scheduler_resumes_from_our_state():
    """Without warmup the state dict is the torch scheduler's own: StepLR / MultiStepLR load it
    and go on with the same LRs."""
    for sched, cls, kw in (("single_step", StepLR, {"step_size": 1}), ("multi_step", MultiStepLR, {"milestones": [1]})):
        o = _sched_cfg(sched, (3, 7), None, True)
        opt = _sgd(o.LR)
        mine = build_lr_scheduler(opt, o)
        for _ in range(5):
            mine.step()
        topt = _sgd(o.LR)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t = cls(topt, gamma=0.5, **kw)
            t.load_state_dict(mine.state_dict())
            topt.param_groups[0]["lr"] = t.get_last_lr()[0]  # (as a resumed optimizer's group carries it)
            for _ in range(5):
                mine.step()
                t.step()
                assert topt.param_groups[0]["lr"] == pytest.approx(opt.param_groups[0]["lr"], rel=1e-12)


def test_unknown_scheduler_raises():
    o = _sched_cfg("exponential", (4,), None, True)
    with pytest.raises(NotImplementedError, match="multi_step"):
        build_lr_scheduler(_sgd(o.LR), o)


# ---------------------------------------------------------------- library and checkpoint
def test_adam_kernel_is_built_and_in_the_source_digest():
    import os
    from fsp_amd import _native
    assert "csrc/optim.hip" in [r for r, _ in _native.source_files()]
    mk = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "Makefile")).read()
    assert "optim.hip" in mk.split("SRCS :=")[1].splitlines()[0]
    assert hasattr(_native.load(), "clipk_adam_step_multi") and "clipk_adam_step_multi" in _native.SIGNATURES


def test_adam_bad_arguments_return_einval_without_a_device():
    """The argument checks come before any launch or pointer use, so they hold on a machine
    without a GPU: the 'device pointers' here are never dereferenced."""
    import ctypes
    from fsp_amd import _native as N
    lib = N.load()
    VP, fake = ctypes.c_void_p * 17, [0x1000 * (i + 1) for i in range(17)]

    def call(count=1, p=fake, beta1=0.9, beta2=0.999, eps=1e-8, lr=2e-3, wd=5e-4, mode=N.ADAM_ADAM, vmax=None,
             n=8, parity=0):
        arr = lambda a: None if a is None else VP(*a)
        return lib.clipk_adam_step_multi(count, arr(p), arr(fake), arr(fake), arr(fake), arr(vmax),
                                         (ctypes.c_long * 17)(*[n] * 17), arr(fake), (ctypes.c_int * 17)(*[parity] * 17),
                                         lr, beta1, beta2, eps, wd, mode, 1.0, None, 0, None)

    for kw in (dict(count=0), dict(count=17), dict(count=-3), dict(p=None), dict(p=[0] + fake[1:]),
               dict(count=16, p=fake[:15] + [0, 1]), dict(beta1=1.0), dict(beta2=1.0), dict(beta1=-0.5),
               dict(beta2=float("nan")), dict(eps=-1e-8), dict(lr=-1.0), dict(wd=-1.0), dict(mode=3), dict(mode=-1),
               dict(mode=N.ADAM_AMSGRAD), dict(mode=N.ADAM_AMSGRAD, vmax=[0] + fake[1:]), dict(parity=2)):
        assert call(**kw) == -1, kw  # CLIPK_EINVAL
    assert call(n=-1) == -2  # CLIPK_ESHAPE


def test_step_scheduler_state_survives_a_checkpoint(tmp_path):
    """The scheduler entry of a checkpoint -- with warmup it carries the torch successor as a
    pickled object, as Dassl's does -- reads back through load_checkpoint (nothing from the file
    runs) and resumes the schedule."""
    from fsp_amd.engine.checkpoint import load_checkpoint, save_checkpoint
    for sched in ("single_step", "multi_step"):
        for warmup in (None, "constant"):
            o = _sched_cfg(sched, (3, 7), warmup, True)
            opt = _sgd(o.LR)
            mine = build_lr_scheduler(opt, o)
            for _ in range(8):
                mine.step()
            d = tmp_path / f"{sched}_{warmup}"
            save_checkpoint({"state_dict": {}, "epoch": 8, "optimizer": None, "scheduler": mine.state_dict()}, str(d))
            ck = load_checkpoint(str(d / "model.pth.tar-8"))
            opt2 = _sgd(o.LR)
            again = build_lr_scheduler(opt2, o)
            again.load_state_dict(ck["scheduler"])
            assert again.last_epoch == 8 and opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
