"""Optimizer + LR schedule for the prompt parameters.

``FusedSGD``: torch.optim.SGD semantics as Dassl builds it for CoOp/CoCoOp
(Dassl.pytorch/dassl/optim/optimizer.py:105-113: momentum 0.9, weight decay 5e-4,
dampening 0, no nesterov) with the update running in the clipk_sgd_step HIP kernel.
``WarmupCosineLR``: Dassl's ConstantWarmupScheduler(CosineAnnealingLR) per-epoch LR
(lr_scheduler.py:35-54,120-152); closed form, pinned by tests/golden/lr_schedule.npz.
``FusedAdam``: Dassl's ``adam`` / ``amsgrad`` / ``adamw`` (torch.optim.Adam / AdamW semantics) in
the clipk_adam_step_multi HIP kernel. ``WarmupStepLR`` / ``WarmupMultiStepLR``: Dassl's
``single_step`` / ``multi_step`` under the same warmup wrapper, checked against torch's StepLR /
MultiStepLR (tests/test_optim_cpu.py).
"""
from __future__ import annotations

import math
import warnings

import torch

from .. import ops


class FusedSGD(torch.optim.Optimizer):
    """Param groups carry every key of torch.optim.SGD's groups, so ``state_dict()`` loads
    into the reference's torch.optim.SGD (and a reference SGD state into this one)."""

    created_last = ()

    def __init__(self, params, lr=0.002, momentum=0.9, weight_decay=5e-4, dampening=0.0,
                 nesterov=False):
        if dampening != 0 or nesterov:
            raise ValueError("FusedSGD implements dampening=0, nesterov=False (the Dassl CoOp setup)")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay,
                                      nesterov=False, maximize=False, foreach=None, differentiable=False,
                                      fused=None))

    @staticmethod
    def defer_grad_scale(grads, s):
        """The next step updates with s * g for these gradient tensors (dist.allreduce_grads folds
        the average of a SUM all-reduce here: one launch less per step). A tag on each tensor,
        set (not multiplied) per all-reduce and consumed by step()."""
        for g in grads:
            g._clipk_grad_scale = s

    @torch.no_grad()
    def step(self, closure=None, guard=None):
        """guard = (int32 device flags, mask): the update is skipped on the device when
        flags[0] & mask (clipk_sgd_step_multi_if); ``created_last`` lists the parameters whose
        momentum buffer this call created (a skipped step's are never written)."""
        loss = closure() if closure is not None else None
        self.created_last = []
        for grp in self.param_groups:
            # the group's tensors in one launch per 16 (clipk_sgd_step_multi): at the reference's
            # batch of 1 the five per-tensor launches were kernel boundaries on the critical path
            ps, gs, bufs, has, scales = [], [], [], [], []
            for p in grp["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("FusedSGD runs on the GPU only (HIP kernel); no CPU path")
                if grp.get("dampening", 0) != 0 or grp.get("nesterov", False) or grp.get("maximize", False):
                    raise ValueError("FusedSGD implements dampening=0, nesterov=False, maximize=False")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError("FusedSGD: fp32 contiguous parameters")
                st = self.state[p]
                buf = st.get("momentum_buffer")
                h = buf is not None
                if not h:
                    buf = st["momentum_buffer"] = torch.empty_like(p)
                    self.created_last.append(p)
                elif buf.device != p.device or not buf.is_contiguous():
                    buf = st["momentum_buffer"] = buf.to(p.device).contiguous()
                ps.append(p.data)
                scales.append(getattr(p.grad, "_clipk_grad_scale", 1.0))
                if hasattr(p.grad, "_clipk_grad_scale"):
                    del p.grad._clipk_grad_scale
                gs.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
                bufs.append(buf)
                has.append(h)
                p._clipk_gen = getattr(p, "_clipk_gen", 0) + 1  # invalidates cached text features
            if ps:
                if len(set(scales)) > 1:  # (mixed tags: scaled here, then one unscaled launch)
                    gs = [g * sc if sc != 1.0 else g for g, sc in zip(gs, scales)]
                    scales = [1.0]
                ops.sgd_step_multi(ps, gs, bufs, grp["lr"], grp["momentum"], grp["weight_decay"], has,
                                   grad_scale=scales[0], guard=guard)
        return loss


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (``decoupled=True``: AdamW; ``amsgrad=True``: AMSGrad) with the update
    running in the clipk_adam_step_multi HIP kernel. Param groups carry every key of the installed
    torch's Adam / AdamW groups and ``state_dict()`` presents the per-parameter state as torch does
    (``step`` an fp32 scalar tensor, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``), so a state
    loads into torch's optimizer and a torch state into this one.

    Live state keeps the step count on the device instead -- ``step_dev``, two int32 counters, and
    ``parity``, the one the next launch reads -- because a guarded step skipped on the device must
    not advance it (clipk_adam_step_multi). ``state_dict()`` reads it back (a synchronisation, at
    save time only); a loaded ``step`` moves to the device at the parameter's next step."""

    created_last = ()
    defer_grad_scale = staticmethod(FusedSGD.defer_grad_scale)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                 decoupled=False):
        self.decoupled = bool(decoupled)
        if decoupled and amsgrad:
            raise ValueError("FusedAdam implements Adam, AdamW and AMSGrad (Adam), not AdamW with amsgrad")
        ref = (torch.optim.AdamW if decoupled else torch.optim.Adam)(
            [torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, dict(ref.defaults))

    def _mode(self, grp):
        if grp.get("decoupled_weight_decay", self.decoupled):
            if grp["amsgrad"]:
                raise ValueError("FusedAdam: AdamW with amsgrad is not implemented")
            return "adamw"
        return "amsgrad" if grp["amsgrad"] else "adam"

    @staticmethod
    def _export(st):
        """One parameter's state as torch.optim.Adam keeps it."""
        if "step_dev" in st:
            step = torch.tensor(float(st["step_dev"][st["parity"]].item()), dtype=torch.float32)
        else:  # loaded and not stepped since
            step = st["step"]
        out = {"step": step, "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
        if "max_exp_avg_sq" in st:
            out["max_exp_avg_sq"] = st["max_exp_avg_sq"]
        return out

    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = {k: self._export(st) for k, st in sd["state"].items()}
        return sd

    @torch.no_grad()
    def step(self, closure=None, guard=None):
        """guard = (int32 device flags, mask): the update is skipped on the device when
        flags[0] & mask, step count included; ``created_last`` lists the parameters whose state
        this call created (all zeros, which a skipped step leaves: fresh state)."""
        loss = closure() if closure is not None else None
        self.created_last = []
        for grp in self.param_groups:
            mode = self._mode(grp)
            names = ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if mode == "amsgrad" else ())
            ps, gs, scales, sts = [], [], [], []
            for p in grp["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("FusedAdam runs on the GPU only (HIP kernel); no CPU path")
                if grp.get("maximize", False):
                    raise ValueError("FusedAdam implements maximize=False")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError("FusedAdam: fp32 contiguous parameters")
                st = self.state[p]
                if "step_dev" not in st:
                    if not st:
                        self.created_last.append(p)
                    t = int(st.pop("step", 0))
                    st["step_dev"] = torch.full((2,), t, dtype=torch.int32, device=p.device)
                    st["parity"] = 0
                for k in names:
                    b = st.get(k)
                    if b is None:
                        st[k] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    elif b.device != p.device or b.dtype != torch.float32 or not b.is_contiguous():
                        st[k] = b.to(p.device, torch.float32).contiguous()
                ps.append(p.data)
                scales.append(getattr(p.grad, "_clipk_grad_scale", 1.0))
                if hasattr(p.grad, "_clipk_grad_scale"):
                    del p.grad._clipk_grad_scale
                gs.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
                sts.append(st)
                p._clipk_gen = getattr(p, "_clipk_gen", 0) + 1  # invalidates cached text features
            if ps:
                if len(set(scales)) > 1:  # (mixed tags: scaled here, then one unscaled launch)
                    gs = [g * sc if sc != 1.0 else g for g, sc in zip(gs, scales)]
                    scales = [1.0]
                ops.adam_step_multi(ps, gs, [s["exp_avg"] for s in sts], [s["exp_avg_sq"] for s in sts],
                                    [s["max_exp_avg_sq"] for s in sts] if mode == "amsgrad" else None,
                                    [s["step_dev"] for s in sts], [s["parity"] for s in sts], grp["lr"],
                                    grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"], mode,
                                    grad_scale=scales[0], guard=guard)
                for s in sts:
                    s["parity"] ^= 1
        return loss


def warmup_lr(epoch: int, base_lr: float, after, warmup_epoch: int = -1, warmup_type: str = "constant",
              warmup_cons_lr: float = 1e-5, warmup_min_lr: float = 1e-5, warmup_recount: bool = True) -> float:
    """Dassl's Constant / LinearWarmupScheduler over a successor: ``after(e, start)`` is the
    successor's LR at its epoch e, its count having started at ``start``."""
    if warmup_epoch > 0 and epoch < warmup_epoch:
        if warmup_type == "constant":
            return warmup_cons_lr
        if warmup_type == "linear":  # LinearWarmupScheduler
            return epoch / warmup_epoch * base_lr if epoch > 0 else warmup_min_lr
        raise ValueError(warmup_type)
    # the successor restarts its count after warmup unless WARMUP_RECOUNT is off
    # (lr_scheduler.py:128-130: then it starts at last_epoch = WARMUP_EPOCH)
    if warmup_epoch > 0 and warmup_recount:
        return after(epoch - warmup_epoch, 0)
    return after(epoch, max(warmup_epoch, 0))


def warmup_cosine_lr(epoch: int, base_lr: float, max_epoch: int, warmup_epoch: int = -1,
                     warmup_type: str = "constant", warmup_cons_lr: float = 1e-5,
                     warmup_min_lr: float = 1e-5, warmup_recount: bool = True) -> float:
    return warmup_lr(epoch, base_lr, lambda e, start: 0.5 * base_lr * (1 + math.cos(math.pi * e / max_epoch)),
                     warmup_epoch, warmup_type, warmup_cons_lr, warmup_min_lr, warmup_recount)


def step_decay_lr(e: int, start: int, base_lr: float, gamma: float, decays) -> float:
    """torch StepLR / MultiStepLR as they chain: the LR is multiplied by gamma ** decays(k) on
    entering epoch k, for every k in (start, e] (a count that starts at ``start`` never sees the
    milestones before it)."""
    lr = base_lr
    for k in range(start + 1, e + 1):
        if decays(k):
            lr = lr * gamma ** decays(k)
    return lr


class WarmupLR:
    """Epoch-stepped scheduler with the Dassl get_last_lr()/step()/state_dict() surface; a
    subclass gives the successor's closed form (``_after``) and its torch scheduler (``_torch``).

    ``state_dict()`` has the shape of the scheduler Dassl's build_lr_scheduler returns
    (lr_scheduler.py:128-152): with warmup, the __dict__ of a Constant/LinearWarmupScheduler
    including its ``successor`` -- the torch scheduler advanced to the same epoch (on a
    detached one-parameter SGD, as a resumed Dassl successor is) -- so the reference's
    ``resume_from_checkpoint`` restores it; without warmup, the torch scheduler's state dict.
    ``load_state_dict`` needs only ``last_epoch`` (the LR is a closed form of it)."""

    def __init__(self, optimizer, optim_cfg):
        self.opt = optimizer
        self.cfg = optim_cfg
        self.base_lr = optim_cfg.LR
        self.last_epoch = 0
        for g in self.opt.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self._apply()

    def _after(self, e, start):
        raise NotImplementedError

    def _torch(self, optimizer):
        raise NotImplementedError

    def _lr(self, e):
        c = self.cfg
        return warmup_lr(e, c.LR, self._after, c.WARMUP_EPOCH, c.WARMUP_TYPE, c.WARMUP_CONS_LR,
                         c.WARMUP_MIN_LR, c.get("WARMUP_RECOUNT", True))

    def _apply(self):
        for g in self.opt.param_groups:
            g["lr"] = self._lr(self.last_epoch)

    def step(self):
        self.last_epoch += 1
        self._apply()

    def get_last_lr(self):
        return [g["lr"] for g in self.opt.param_groups]

    def _successor(self, start, done, groups=1):
        """The torch scheduler on a detached SGD of ``groups`` one-parameter groups, its count
        started at ``start`` and stepped ``done`` times."""
        dummy = torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(1))]} for _ in range(groups)],
                                lr=self.cfg.LR)
        succ = self._torch(dummy)
        succ.last_epoch = start
        with warnings.catch_warnings():  # the detached optimizer never steps
            warnings.simplefilter("ignore")
            for _ in range(done):
                succ.step()
        return succ

    def _plain_state(self, epochs):
        """Without warmup: the torch scheduler's own state dict at ``epochs``."""
        return self._successor(0, epochs, len(self.opt.param_groups)).state_dict()

    def state_dict(self):
        c = self.cfg
        n = len(self.opt.param_groups)
        if not (c.WARMUP_EPOCH > 0):
            return self._plain_state(self.last_epoch)
        # the successor: stepped only after the warmup epochs (lr_scheduler.py:27-33)
        done = max(0, self.last_epoch - c.WARMUP_EPOCH)
        start = 0 if c.get("WARMUP_RECOUNT", True) else c.WARMUP_EPOCH
        succ = self._successor(start, done)
        # Dassl's warmup wrapper stops counting once the successor takes over (its step()
        # only steps the successor past warmup, lr_scheduler.py:27-33)
        outer = min(self.last_epoch, c.WARMUP_EPOCH)
        sd = {"successor": succ, "warmup_epoch": c.WARMUP_EPOCH, "base_lrs": [c.LR] * n,
              "last_epoch": outer, "_step_count": outer + 1,
              "_get_lr_called_within_step": False, "_is_initial": False,
              "_last_lr": [g["lr"] for g in self.opt.param_groups]}
        if c.WARMUP_TYPE == "constant":
            sd["cons_lr"] = c.WARMUP_CONS_LR
        else:
            sd["min_lr"] = c.WARMUP_MIN_LR
        return sd

    def load_state_dict(self, sd):
        """Epochs stepped so far, from our state or a Dassl one: past warmup, Dassl keeps the
        wrapper's last_epoch at WARMUP_EPOCH and counts on in the successor (whose count
        starts at 0, or at WARMUP_EPOCH without WARMUP_RECOUNT)."""
        c = self.cfg
        e = int(sd["last_epoch"])
        succ = sd.get("successor")
        if c.WARMUP_EPOCH > 0 and e >= c.WARMUP_EPOCH:
            s_last = getattr(succ, "last_epoch", None) if not isinstance(succ, dict) else succ.get("last_epoch")
            if s_last is not None:
                start = 0 if c.get("WARMUP_RECOUNT", True) else c.WARMUP_EPOCH
                e = c.WARMUP_EPOCH + int(s_last) - start
        self.last_epoch = e
        self._apply()


class WarmupCosineLR(WarmupLR):
    """Dassl's ``cosine``: CosineAnnealingLR(T_max = MAX_EPOCH) under the warmup wrapper."""

    def _after(self, e, start):
        return 0.5 * self.cfg.LR * (1 + math.cos(math.pi * e / self.cfg.MAX_EPOCH))

    def _torch(self, optimizer):
        return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, float(self.cfg.MAX_EPOCH))

    def _plain_state(self, epochs):
        c = self.cfg
        return {"T_max": float(c.MAX_EPOCH), "eta_min": 0.0, "base_lrs": [c.LR] * len(self.opt.param_groups),
                "last_epoch": epochs, "_step_count": epochs + 1,
                "_get_lr_called_within_step": False, "_is_initial": False,
                "_last_lr": [0.5 * c.LR * (1 + math.cos(math.pi * epochs / c.MAX_EPOCH))] * len(self.opt.param_groups)}


class WarmupStepLR(WarmupLR):
    """Dassl's ``single_step``: StepLR(step_size = STEPSIZE[-1], or MAX_EPOCH when that is <= 0,
    gamma = GAMMA) under the warmup wrapper."""

    def __init__(self, optimizer, optim_cfg):
        size = optim_cfg.STEPSIZE
        size = size[-1] if isinstance(size, (list, tuple)) else size
        self.step_size = int(size) if size > 0 else int(optim_cfg.MAX_EPOCH)
        super().__init__(optimizer, optim_cfg)

    def _after(self, e, start):
        return step_decay_lr(e, start, self.cfg.LR, self.cfg.GAMMA, lambda k: k % self.step_size == 0)

    def _torch(self, optimizer):
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=self.step_size, gamma=self.cfg.GAMMA)


class WarmupMultiStepLR(WarmupLR):
    """Dassl's ``multi_step``: MultiStepLR(milestones = STEPSIZE, gamma = GAMMA) under the warmup
    wrapper."""

    def __init__(self, optimizer, optim_cfg):
        if not isinstance(optim_cfg.STEPSIZE, (list, tuple)):
            raise TypeError(f"For multi_step lr_scheduler, STEPSIZE must be a list, got {type(optim_cfg.STEPSIZE)}")
        self.milestones = [int(m) for m in optim_cfg.STEPSIZE]
        super().__init__(optimizer, optim_cfg)

    def _after(self, e, start):
        return step_decay_lr(e, start, self.cfg.LR, self.cfg.GAMMA, self.milestones.count)

    def _torch(self, optimizer):
        return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=self.milestones, gamma=self.cfg.GAMMA)


OPTIMIZERS = ("sgd", "adam", "amsgrad", "adamw")
LR_SCHEDULERS = {"cosine": WarmupCosineLR, "single_step": WarmupStepLR, "multi_step": WarmupMultiStepLR}


def build_optimizer(module, optim_cfg):
    name = optim_cfg.NAME
    if name not in OPTIMIZERS:
        raise NotImplementedError(f"Optimizer {name} not implemented on this path (implemented: "
                                  f"{', '.join(OPTIMIZERS)})")
    params = [p for p in module.parameters() if p.requires_grad]
    if name == "sgd":
        return FusedSGD(params, lr=optim_cfg.LR, momentum=optim_cfg.MOMENTUM,
                        weight_decay=optim_cfg.WEIGHT_DECAY, dampening=optim_cfg.SGD_DAMPNING,
                        nesterov=optim_cfg.SGD_NESTEROV)
    # Dassl: Adam(amsgrad=...) / AdamW with betas = (ADAM_BETA1, ADAM_BETA2)
    return FusedAdam(params, lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY,
                     betas=(optim_cfg.ADAM_BETA1, optim_cfg.ADAM_BETA2), amsgrad=name == "amsgrad",
                     decoupled=name == "adamw")


def build_lr_scheduler(optimizer, optim_cfg):
    if optim_cfg.LR_SCHEDULER not in LR_SCHEDULERS:
        raise NotImplementedError(f"LR scheduler {optim_cfg.LR_SCHEDULER} not implemented on this path "
                                  f"(implemented: {', '.join(LR_SCHEDULERS)})")
    return LR_SCHEDULERS[optim_cfg.LR_SCHEDULER](optimizer, optim_cfg)
