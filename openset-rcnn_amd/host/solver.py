"""Mirror of the two detectron2 solver factories the reference's trainer calls (train.py:110-111): `build_optimizer(cfg, model)`
and `build_lr_scheduler(cfg, optimizer)`, so that the loop body of train.py:135-146 runs unchanged on the HIP path --

    loss_dict = model(data); losses = sum(loss_dict.values()); assert torch.isfinite(losses).all(), loss_dict
    loss_dict_reduced = {k: v.item() for k, v in comm.reduce_dict(loss_dict).items()}
    optimizer.zero_grad(); losses.backward(); optimizer.step(); scheduler.step()

`losses.backward()` runs the explicit HIP backward into the trainer's flat fp32 gradient buffer (modeling._ExplicitBackward);
`optimizer.step()` sums that buffer over the ranks (RCCL, bucketed, overlapped with the tail of the backward when several ranks
run) and applies SGD with momentum and weight decay on the fp32 masters, gated by the overflow guard: one launch over every
parameter, osr_sgd_step_multi_ex (csrc/osr_solver.hip). The [d2] options beyond one plain SGD group -- SOLVER.CLIP_GRADIENTS (per
parameter), BIAS_LR_FACTOR / WEIGHT_DECAY_BIAS (a bias group) and NESTEROV -- are arguments of that launch and entries of its
table (norm clipping adds the norm pass, osr_grad_norm_partials, in front of it); with none of them on it is torch.optim.SGD's
plain step, through the same kernel."""
from __future__ import annotations

import bisect
import math
from typing import Callable, List, Optional

from .train import SolverOptions, warmup_multistep_lr

CLIP_TYPES = ("value", "norm")


class HipSGD:
    """[d2] build_optimizer -> torch.optim.SGD over get_default_optimizer_params' groups, merged as reduce_param_groups merges them:
    group 0 holds every trainable parameter that is not a bias (BASE_LR, WEIGHT_DECAY; the PLN representatives included); every
    parameter named `bias` gets BASE_LR * BIAS_LR_FACTOR and WEIGHT_DECAY_BIAS (None: WEIGHT_DECAY), a group of its own when that
    differs from group 0. (Every norm layer on this path is a FrozenBN, so WEIGHT_DECAY_NORM has no parameter to act on.)
    `param_groups[0]["lr"]` is what train.py:147 logs; the scheduler multiplies every group's `initial_lr` by the same factor.
    `clip` ([d2] maybe_add_gradient_clipping): None or (CLIP_TYPE, CLIP_VALUE, NORM_TYPE), applied per parameter to the averaged
    gradient before the weight decay."""

    def __init__(self, model, lr: float, momentum: float, weight_decay: float, nesterov: bool = False, bias_lr_factor: float = 1.0,
                 weight_decay_bias: Optional[float] = None, clip: Optional[tuple] = None):
        self.model = model
        wd_bias = float(weight_decay) if weight_decay_bias is None else float(weight_decay_bias)
        base = dict(lr=float(lr), momentum=float(momentum), weight_decay=float(weight_decay), nesterov=bool(nesterov), initial_lr=float(lr))
        self.param_groups: List[dict] = [base]
        if float(bias_lr_factor) != 1.0 or wd_bias != float(weight_decay):
            blr = float(lr) * float(bias_lr_factor)
            self.param_groups.append(dict(base, lr=blr, initial_lr=blr, weight_decay=wd_bias))
        if clip is not None:
            ctype, cval, ntype = clip
            if ctype not in CLIP_TYPES:
                raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_TYPE {ctype!r}: not one of {CLIP_TYPES}")
            clip = (ctype, float(cval), float(ntype))
            if ctype == "norm" and not clip[2] > 0:
                raise ValueError(f"SOLVER.CLIP_GRADIENTS.NORM_TYPE {ntype}: must be > 0 (inf for the max norm)")
        self.clip = clip

    def solver_options(self) -> Optional[SolverOptions]:
        """None when the update is one plain SGD group (the launches of every committed yaml file); else the trainer's options."""
        g0 = self.param_groups[0]
        nesterov = bool(g0.get("nesterov", False))
        factor, wd_bias = 1.0, None
        if len(self.param_groups) > 1:
            gb = self.param_groups[1]
            factor = gb["initial_lr"] / g0["initial_lr"] if g0["initial_lr"] else 1.0
            wd_bias = float(gb["weight_decay"])
            if bool(gb.get("nesterov", False)) != nesterov or gb["momentum"] != g0["momentum"]:
                raise NotImplementedError("HipSGD: the bias group's momentum / nesterov must be the base group's")
        if self.clip is None and factor == 1.0 and (wd_bias is None or wd_bias == g0["weight_decay"]) and not nesterov:
            return None
        ctype, cval, ntype = self.clip if self.clip is not None else (None, 1.0, 2.0)
        return SolverOptions(factor, wd_bias, nesterov, ctype, cval, ntype)

    def zero_grad(self, set_to_none: bool = True) -> None:
        """No-op: every backward overwrites the whole gradient buffer (there is no accumulation across iterations)."""

    def step(self) -> None:
        t = self.model.trainer()
        if not getattr(t, "grads_ready", False):
            raise RuntimeError("optimizer.step() before losses.backward(): the gradient buffer holds no gradients of this iteration")
        g = self.param_groups[0]
        t.lr, t.momentum, t.weight_decay = g["lr"], g["momentum"], g["weight_decay"]
        t.solver_options = self.solver_options()
        t._update(t.all_reduce_grads())
        t.grads_ready = False

    def state_dict(self) -> dict:
        return dict(param_groups=[dict(g) for g in self.param_groups], momentum=self.model.trainer().export_optimizer_state())

    def load_state_dict(self, state: dict) -> None:
        groups = [dict(g) for g in state["param_groups"]]
        if len(groups) != len(self.param_groups):
            raise ValueError(f"loaded state has {len(groups)} parameter groups, this optimizer {len(self.param_groups)}")
        self.param_groups = groups
        self.model.trainer().load_optimizer_state(state["momentum"])


def build_optimizer(cfg, model) -> HipSGD:
    s = cfg.SOLVER
    wd_bias = s.get("WEIGHT_DECAY_BIAS", None)
    clip = None
    cg = s.get("CLIP_GRADIENTS", None)
    if cg is not None and cg.get("ENABLED", False):
        clip = (cg.CLIP_TYPE, cg.CLIP_VALUE, cg.NORM_TYPE)
    return HipSGD(model, s.BASE_LR, s.MOMENTUM, s.WEIGHT_DECAY, nesterov=bool(s.get("NESTEROV", False)),
                  bias_lr_factor=float(s.get("BIAS_LR_FACTOR", 1.0)), weight_decay_bias=None if wd_bias is None else float(wd_bias), clip=clip)


# ---- schedules: [d2] LRMultiplier(WarmupParamScheduler(sched, WARMUP_FACTOR, min(WARMUP_ITERS / MAX_ITER, 1), METHOD), MAX_ITER) ----
_WHERE_EPSILON = 1e-6  # fvcore ParamScheduler.WHERE_EPSILON


def cosine_multiplier(end_value: float) -> Callable[[float], float]:
    """fvcore CosineParamScheduler(1, end_value)."""
    return lambda where: end_value + 0.5 * (1.0 - end_value) * (1.0 + math.cos(math.pi * where))


def multistep_multiplier(steps, gamma: float, max_iter: int) -> Callable[[float], float]:
    """fvcore MultiStepParamScheduler(values=[gamma ** k], milestones=steps, num_updates=max_iter), as [d2] builds it."""
    steps = [x for x in steps if x <= max_iter]
    values = [gamma ** k for k in range(len(steps) + 1)]
    return lambda where: values[bisect.bisect_right(steps, int((where + _WHERE_EPSILON) * max_iter))]


def warmup_multiplier(sched: Callable[[float], float], warmup_factor: float, warmup_length: float, method: str) -> Callable[[float], float]:
    """[d2] WarmupParamScheduler: fvcore CompositeParamScheduler([warmup, sched], interval_scaling=[rescaled, fixed],
    lengths=[warmup_length, 1 - warmup_length]). Linear warm-up runs from warmup_factor * sched(0) to sched(warmup_length);
    constant warm-up holds warmup_factor * sched(0)."""
    start, end = warmup_factor * sched(0.0), sched(warmup_length)
    if method == "linear":
        warm = lambda t: t * end + (1 - t) * start  # noqa: E731  (fvcore LinearParamScheduler)
    elif method == "constant":
        warm = lambda t: start  # noqa: E731
    else:
        raise ValueError(f"Unknown warmup method: {method}")

    def f(where: float) -> float:
        if where + _WHERE_EPSILON > warmup_length:
            return sched(where)
        return warm(where / warmup_length)
    return f


class _GroupScheduler:
    """Writes every group's lr = initial_lr * multiplier(iteration) ([d2] LRMultiplier), like torch's schedulers: construction sets
    the learning rate of iteration last_iter + 1."""

    def __init__(self, optimizer: HipSGD, last_iter: int = -1):
        self.optimizer = optimizer
        self.last_iter = last_iter
        self.step()

    def multiplier(self, iteration: int) -> float:
        raise NotImplementedError

    def _set_lrs(self) -> None:
        m = self.multiplier(self.last_iter)
        for g in self.optimizer.param_groups:
            g["lr"] = g["initial_lr"] * m

    def step(self) -> None:
        self.last_iter += 1
        self._set_lrs()

    def state_dict(self) -> dict:
        return dict(last_iter=self.last_iter)

    def load_state_dict(self, state: dict) -> None:
        self.last_iter = int(state["last_iter"]) - 1
        self.step()


class WarmupMultiStepLR(_GroupScheduler):
    """[d2] build_lr_scheduler for SOLVER.LR_SCHEDULER_NAME "WarmupMultiStepLR" (the default both yaml files use), linear warm-up.
    Group 0's lr is warmup_multistep_lr's; any other group's is its initial_lr times the same factor."""

    def __init__(self, optimizer: HipSGD, base_lr, steps, gamma, warmup_iters, warmup_factor, last_iter: int = -1):
        self.base_lr, self.steps, self.gamma = float(base_lr), tuple(steps), float(gamma)
        self.warmup_iters, self.warmup_factor = int(warmup_iters), float(warmup_factor)
        super().__init__(optimizer, last_iter)

    def get_lr(self) -> float:
        return warmup_multistep_lr(self.last_iter, self.base_lr, self.steps, self.gamma, self.warmup_iters, self.warmup_factor)

    def multiplier(self, iteration: int) -> float:
        return warmup_multistep_lr(iteration, 1.0, self.steps, self.gamma, self.warmup_iters, self.warmup_factor)

    def _set_lrs(self) -> None:
        super()._set_lrs()
        self.optimizer.param_groups[0]["lr"] = self.get_lr()


class WarmupParamLR(_GroupScheduler):
    """[d2] LRMultiplier over WarmupParamScheduler: WarmupCosineLR (either warm-up method) and WarmupMultiStepLR with constant
    warm-up. multiplier(it) = warmup_multiplier(sched, ...)(it / max_iter)."""

    def __init__(self, optimizer: HipSGD, sched: Callable[[float], float], max_iter: int, warmup_iters: int, warmup_factor: float,
                 method: str, last_iter: int = -1):
        self.max_iter = int(max_iter)
        self._mult = warmup_multiplier(sched, float(warmup_factor), min(int(warmup_iters) / self.max_iter, 1.0), method)
        super().__init__(optimizer, last_iter)

    def multiplier(self, iteration: int) -> float:
        return self._mult(iteration / self.max_iter)


def build_lr_scheduler(cfg, optimizer: HipSGD, last_iter: int = -1) -> _GroupScheduler:
    s = cfg.SOLVER
    name, method = s.LR_SCHEDULER_NAME, s.WARMUP_METHOD
    if method not in ("linear", "constant"):
        raise ValueError(f"Unknown warmup method: {method}")
    if name == "WarmupMultiStepLR":
        if method == "linear":
            return WarmupMultiStepLR(optimizer, s.BASE_LR, s.STEPS, s.GAMMA, s.WARMUP_ITERS, s.WARMUP_FACTOR, last_iter)
        sched = multistep_multiplier(s.STEPS, float(s.GAMMA), int(s.MAX_ITER))
    elif name == "WarmupCosineLR":
        end_value = float(s.get("BASE_LR_END", 0.0)) / float(s.BASE_LR)
        if not 0.0 <= end_value <= 1.0:
            raise ValueError(f"SOLVER.BASE_LR_END / BASE_LR = {end_value}: must be in [0, 1]")
        sched = cosine_multiplier(end_value)
    elif name == "WarmupStepWithFixedGammaLR":
        raise NotImplementedError("SOLVER.LR_SCHEDULER_NAME WarmupStepWithFixedGammaLR")
    else:
        raise ValueError(f"Unknown LR scheduler: {name}")
    return WarmupParamLR(optimizer, sched, s.MAX_ITER, s.WARMUP_ITERS, s.WARMUP_FACTOR, method, last_iter)
