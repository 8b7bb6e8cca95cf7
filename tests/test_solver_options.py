"""CPU tests of the [d2] solver options beyond one plain SGD group (host/solver.py): SOLVER.CLIP_GRADIENTS, BIAS_LR_FACTOR /
WEIGHT_DECAY_BIAS parameter groups, NESTEROV, and the schedules of build_lr_scheduler (WarmupCosineLR, constant warm-up),
checked against formulas written out here."""
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(extra=()):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "voc_coco.yaml"))
    cfg.merge_from_list(list(extra))
    return cfg


def test_config_has_the_clip_section_and_cosine_end(osr):
    cfg = _cfg()
    cg = cfg.SOLVER.CLIP_GRADIENTS
    assert (cg.ENABLED, cg.CLIP_TYPE, cg.CLIP_VALUE, cg.NORM_TYPE) == (False, "value", 1.0, 2.0)
    assert cfg.SOLVER.BASE_LR_END == 0.0
    cfg = _cfg(["SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm", "SOLVER.CLIP_GRADIENTS.NORM_TYPE", "inf"])
    assert cfg.SOLVER.CLIP_GRADIENTS.ENABLED and math.isinf(cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE)


def test_default_config_is_one_plain_group(osr):
    from openset_rcnn_amd.host.solver import build_optimizer
    cfg = _cfg()
    opt = build_optimizer(cfg, None)
    assert len(opt.param_groups) == 1 and opt.clip is None
    assert opt.solver_options() is None  # the update runs the plain launches
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["momentum"], g["nesterov"]) == (cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY, cfg.SOLVER.MOMENTUM, False)


def test_build_optimizer_accepts_clip_bias_and_nesterov(osr):
    from openset_rcnn_amd.host.solver import build_optimizer
    cfg = _cfg(["SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", "0.5",
                "SOLVER.BIAS_LR_FACTOR", "2.0", "SOLVER.WEIGHT_DECAY_BIAS", "0.0", "SOLVER.NESTEROV", "True"])
    opt = build_optimizer(cfg, None)
    base, bias = opt.param_groups
    lr, wd = cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY
    assert (base["lr"], base["initial_lr"], base["weight_decay"], base["nesterov"]) == (lr, lr, wd, True)  # group 0 is the base group
    assert bias["lr"] == pytest.approx(2.0 * lr) and bias["weight_decay"] == 0.0 and bias["nesterov"]
    o = opt.solver_options()
    assert o.clip == "norm" and o.clip_value == 0.5 and o.norm_type == 2.0
    assert o.bias_lr_factor == pytest.approx(2.0) and o.weight_decay_bias == 0.0 and o.nesterov
    # each option alone leaves the plain path
    for extra in (["SOLVER.NESTEROV", "True"], ["SOLVER.BIAS_LR_FACTOR", "2.0"], ["SOLVER.WEIGHT_DECAY_BIAS", "0.0"],
                  ["SOLVER.CLIP_GRADIENTS.ENABLED", "True"]):
        assert build_optimizer(_cfg(extra), None).solver_options() is not None, extra
    # WEIGHT_DECAY_BIAS None means WEIGHT_DECAY: one group
    cfg = _cfg()
    cfg.SOLVER.WEIGHT_DECAY_BIAS = None
    assert len(build_optimizer(cfg, None).param_groups) == 1
    # value clipping: the default type
    o = build_optimizer(_cfg(["SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", "0.25"]), None).solver_options()
    assert (o.clip, o.clip_value, o.bias_lr_factor, o.nesterov) == ("value", 0.25, 1.0, False)


def test_unknown_clip_type_raises_value_error(osr):
    from openset_rcnn_amd.host.solver import build_optimizer
    with pytest.raises(ValueError):
        build_optimizer(_cfg(["SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model"]), None)
    # off: not looked at ([d2] builds no clipper)
    build_optimizer(_cfg(["SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model"]), None)


def test_optimizer_state_round_trips_the_groups(osr):
    from openset_rcnn_amd.host.solver import HipSGD, build_lr_scheduler

    class _T:
        def export_optimizer_state(self):
            return {}

        def load_optimizer_state(self, s):
            self.loaded = s

    class _M:
        t = _T()

        def trainer(self):
            return self.t

    cfg = _cfg(["SOLVER.BIAS_LR_FACTOR", "3.0"])
    opt = HipSGD(_M(), 0.01, 0.9, 1e-4, nesterov=True, bias_lr_factor=3.0, weight_decay_bias=0.0)
    build_lr_scheduler(cfg, opt, last_iter=99)
    st = opt.state_dict()
    opt2 = HipSGD(_M(), 0.01, 0.9, 1e-4, nesterov=True, bias_lr_factor=3.0, weight_decay_bias=0.0)
    opt2.load_state_dict(st)
    assert opt2.param_groups == opt.param_groups and opt2.solver_options() == opt.solver_options()
    with pytest.raises(ValueError):
        HipSGD(_M(), 0.01, 0.9, 1e-4).load_state_dict(st)


# ---- schedules ----------------------------------------------------------------------------------------------
def _cosine(it, base, max_iter, wi, wf, method, end=0.0):
    """[d2] v0.6 WarmupCosineLR, written out: cos(w) = e + 0.5 (1 - e)(1 + cos(pi w)), w = it / MAX_ITER; warm-up over
    L = WARMUP_ITERS / MAX_ITER from WARMUP_FACTOR * cos(0) (linear: to cos(L); constant: held)."""
    e = end / base
    cos = lambda w: e + 0.5 * (1 - e) * (1 + math.cos(math.pi * w))  # noqa: E731
    w, L = it / max_iter, min(wi / max_iter, 1.0)
    if w + 1e-6 > L:
        return base * cos(w)
    t = w / L
    if method == "constant":
        return base * wf * cos(0.0)
    return base * (t * cos(L) + (1 - t) * wf * cos(0.0))


def _checkpoints(wi, max_iter):
    return [0, wi // 2, wi - 1, wi, (wi + max_iter) // 2, max_iter - 1]


@pytest.mark.parametrize("method", ["linear", "constant"])
@pytest.mark.parametrize("end", [0.0, 0.0005])
def test_warmup_cosine_matches_the_formula(osr, method, end):
    from openset_rcnn_amd.host.solver import HipSGD, build_lr_scheduler
    base, max_iter, wi, wf = 0.02, 1000, 100, 0.001
    cfg = _cfg(["SOLVER.LR_SCHEDULER_NAME", "WarmupCosineLR", "SOLVER.WARMUP_METHOD", method, "SOLVER.BASE_LR", str(base),
                "SOLVER.MAX_ITER", str(max_iter), "SOLVER.WARMUP_ITERS", str(wi), "SOLVER.WARMUP_FACTOR", str(wf), "SOLVER.BASE_LR_END", str(end),
                "SOLVER.BIAS_LR_FACTOR", "2.0"])
    opt = HipSGD(None, base, 0.9, 1e-4, bias_lr_factor=2.0)
    sch = build_lr_scheduler(cfg, opt)
    marks = set(_checkpoints(wi, max_iter))
    for it in range(max_iter):
        if it in marks:
            want = _cosine(it, base, max_iter, wi, wf, method, end)
            assert opt.param_groups[0]["lr"] == pytest.approx(want, rel=1e-12, abs=1e-15), it
            assert opt.param_groups[1]["lr"] == pytest.approx(2.0 * want, rel=1e-12, abs=1e-15), it  # same factor on every group
        sch.step()
    # the warm-up really ramps (linear) / holds (constant), and the run ends near BASE_LR_END
    assert _cosine(wi // 2, base, max_iter, wi, wf, method, end) != _cosine(0, base, max_iter, wi, wf, method, end) or method == "constant"
    assert _cosine(max_iter - 1, base, max_iter, wi, wf, method, end) == pytest.approx(end, abs=1e-6)
    # resume: a scheduler built at last_iter = it - 1 gives iteration it's lr, and steps on from there
    for it in _checkpoints(wi, max_iter):
        opt2 = HipSGD(None, base, 0.9, 1e-4, bias_lr_factor=2.0)
        sch2 = build_lr_scheduler(cfg, opt2, last_iter=it - 1)
        assert opt2.param_groups[0]["lr"] == pytest.approx(_cosine(it, base, max_iter, wi, wf, method, end), rel=1e-12, abs=1e-15)
        sch2.step()
        assert opt2.param_groups[0]["lr"] == pytest.approx(_cosine(it + 1, base, max_iter, wi, wf, method, end), rel=1e-12, abs=1e-15)
        sd = sch2.state_dict()
        sch.load_state_dict(sd)
        assert opt.param_groups[0]["lr"] == opt2.param_groups[0]["lr"]


def test_linear_warmup_is_not_schedule_times_ramp(osr):
    """Linear warm-up runs from WARMUP_FACTOR * sched(0) to sched(L): at mid warm-up that differs from sched(w) * ramp(w)."""
    from openset_rcnn_amd.host.solver import HipSGD, build_lr_scheduler
    base, max_iter, wi, wf = 1.0, 100, 50, 0.1
    cfg = _cfg(["SOLVER.LR_SCHEDULER_NAME", "WarmupCosineLR", "SOLVER.BASE_LR", str(base), "SOLVER.MAX_ITER", str(max_iter),
                "SOLVER.WARMUP_ITERS", str(wi), "SOLVER.WARMUP_FACTOR", str(wf)])
    opt = HipSGD(None, base, 0.9, 1e-4)
    build_lr_scheduler(cfg, opt, last_iter=24)
    cos = lambda w: 0.5 * (1 + math.cos(math.pi * w))  # noqa: E731
    lin = 0.5 * cos(0.5) + 0.5 * wf  # halfway from wf * cos(0) to cos(L = 0.5)
    product = cos(0.25) * (wf + (1 - wf) * 0.5)
    assert opt.param_groups[0]["lr"] == pytest.approx(lin, rel=1e-12)
    assert abs(lin - product) > 1e-2


def test_constant_warmup_of_multistep(osr):
    from openset_rcnn_amd.host.solver import HipSGD, build_lr_scheduler
    base, wi, wf = 0.01, 200, 0.05
    cfg = _cfg(["SOLVER.WARMUP_METHOD", "constant", "SOLVER.BASE_LR", str(base), "SOLVER.MAX_ITER", "1000", "SOLVER.STEPS", "(600, 800)",
                "SOLVER.WARMUP_ITERS", str(wi), "SOLVER.WARMUP_FACTOR", str(wf), "SOLVER.GAMMA", "0.1"])
    want = lambda it: base * (wf if it < wi else 1.0) * 0.1 ** sum(it >= s for s in (600, 800))  # noqa: E731
    for it in (0, 100, 199, 200, 599, 600, 799, 800, 999):
        opt = HipSGD(None, base, 0.9, 1e-4)
        build_lr_scheduler(cfg, opt, last_iter=it - 1)
        assert opt.param_groups[0]["lr"] == pytest.approx(want(it), rel=1e-12), it


def test_linear_multistep_is_unchanged_and_scales_every_group(osr):
    from openset_rcnn_amd.host.solver import HipSGD, build_lr_scheduler
    from openset_rcnn_amd.host.train import warmup_multistep_lr
    cfg = _cfg(["SOLVER.BIAS_LR_FACTOR", "2.0"])
    s = cfg.SOLVER
    opt = HipSGD(None, s.BASE_LR, 0.9, 1e-4, bias_lr_factor=2.0)
    sch = build_lr_scheduler(cfg, opt)
    kw = dict(base_lr=s.BASE_LR, steps=tuple(s.STEPS), gamma=s.GAMMA, warmup_iters=s.WARMUP_ITERS, warmup_factor=s.WARMUP_FACTOR)
    for it in range(0, 600):
        assert opt.param_groups[0]["lr"] == warmup_multistep_lr(it, **kw)
        assert opt.param_groups[1]["lr"] == pytest.approx(2.0 * warmup_multistep_lr(it, **kw), rel=1e-12)
        sch.step()


def test_unknown_schedule_names_are_refused(osr):
    from openset_rcnn_amd.host.solver import HipSGD, build_lr_scheduler
    with pytest.raises(ValueError):
        build_lr_scheduler(_cfg(["SOLVER.WARMUP_METHOD", "exponential"]), HipSGD(None, 0.01, 0.9, 1e-4))
    with pytest.raises(ValueError):
        build_lr_scheduler(_cfg(["SOLVER.LR_SCHEDULER_NAME", "NoSuchLR"]), HipSGD(None, 0.01, 0.9, 1e-4))
