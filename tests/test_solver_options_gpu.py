"""GPU tests of the [d2] solver options (csrc/osr_solver.hip, host/solver.py): per-parameter gradient clipping, a bias parameter
group and Nesterov momentum.
  * kernel level: osr_grad_norm_partials + osr_sgd_step_multi_ex against a float64 restatement, every clip type and norm;
  * whole step, both trainers: `model(data)` / `backward` / `step` against torch.nn.utils.clip_grad_* + torch.optim.SGD applied per
    detectron2 parameter to the exported fp32 parameters;
  * with every option off the update is the same launch with the neutral options: one plan, the same bits (what that launch computed
    before it became the only one is pinned in tests/test_update_pin.py);
  * run_net.py's loop trains with clipping, a bias group, Nesterov and WarmupCosineLR on."""
import logging
import math
import os

import pytest
import torch

from tests.test_run_net import toy_voc_root  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF = float("inf")


# ---- kernel level ---------------------------------------------------------------------------------------------
def _masters(seed=0):
    """Four masters: a conv with a folded FrozenBN row scale and an fp16 working copy, a (5, 256) matrix holding two parameters
    (rows 0-3, row 4), its (5,) bias (two parameters), and a 40 000-element matrix (three chunks)."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(6, 3, 3, 16), (5, 256), (5,), (100, 400)]
    out = []
    for i, sh in enumerate(shapes):
        p = torch.randn(sh, generator=g) * 0.05
        gr = torch.randn(sh, generator=g) * 3.0
        v = torch.randn(sh, generator=g) * 0.01
        rs = (torch.rand(sh[0], generator=g) + 0.5) if i == 0 else None
        out.append(dict(p=p, g=gr, v=v, rs=rs))
    return out


def _segments(ms):
    """(master index, row0, row1, is_bias)."""
    return [(0, 0, 6, False), (1, 0, 4, False), (1, 4, 5, False), (2, 0, 4, True), (2, 4, 5, True), (3, 0, 100, False)]


def _run_kernel(osr, ms, lr, mu, gs, clip, cv, p, nesterov, bias_factor, wd, wd_bias, flag_value=1):
    ops = osr.ops
    dev = []
    for m in ms:
        d = dict(p=m["p"].to(DEV), g=m["g"].to(DEV), v=m["v"].to(DEV), rs=m["rs"].to(DEV) if m["rs"] is not None else None)
        d["lp"] = torch.zeros(m["p"].shape, dtype=torch.float16, device=DEV) if m["rs"] is not None else None
        dev.append(d)
    entries = [(dev[i]["p"], dev[i]["g"], dev[i]["v"], dev[i]["rs"], dev[i]["lp"], r0, r1, bias_factor if b else 1.0, wd_bias if b else wd, nesterov)
               for i, r0, r1, b in _segments(ms)]
    plan = ops.sgd_segment_plan(entries, torch.device(DEV))
    flag = torch.full((1,), flag_value, dtype=torch.int32, device=DEV)
    if clip == "norm":
        ops.grad_norm_partials_(plan, gs, p, flag)
    ops.sgd_step_multi_ex_(plan, lr, mu, gs, clip, cv, p, flag)
    torch.cuda.synchronize()
    return [{k: (t.cpu() if t is not None else None) for k, t in d.items()} for d in dev], plan


def _reference(ms, lr, mu, gs, clip, cv, p, nesterov, bias_factor, wd, wd_bias):
    """float64 restatement of [d2] maybe_add_gradient_clipping + torch.optim.SGD, per segment. Returns (masters, coefficients)."""
    out = [dict(p=m["p"].double().clone(), v=m["v"].double().clone()) for m in ms]
    coefs = []
    for i, r0, r1, b in _segments(ms):
        m = ms[i]
        rs = m["rs"].double()[r0:r1].view(-1, *([1] * (m["p"].dim() - 1))) if m["rs"] is not None else 1.0
        d = m["g"].double()[r0:r1] * gs * rs
        c = 1.0
        if clip == "value":
            d = d.clamp(-cv, cv)
        elif clip == "norm":
            n = float(d.abs().max()) if math.isinf(p) else float((d.abs() ** p).sum() ** (1.0 / p))
            c = cv / (n + 1e-6)
            if c < 1:
                d = d * c
        coefs.append(c)
        pm, v = out[i]["p"][r0:r1], out[i]["v"][r0:r1]
        d = d + (wd_bias if b else wd) * pm
        v.mul_(mu).add_(d)
        step = d + mu * v if nesterov else v.clone()
        pm.sub_(lr * (bias_factor if b else 1.0) * step)
    for i, m in enumerate(ms):
        if m["rs"] is not None:
            out[i]["lp"] = out[i]["p"] * m["rs"].double().view(-1, *([1] * (m["p"].dim() - 1)))
    return out, coefs


def _check(got, want, ms):
    for i, (gd, wt) in enumerate(zip(got, want)):
        torch.testing.assert_close(gd["v"].double(), wt["v"], rtol=2e-5, atol=1e-7, msg=f"momentum of master {i}")
        torch.testing.assert_close(gd["p"].double(), wt["p"], rtol=2e-5, atol=1e-7, msg=f"param of master {i}")
        if "lp" in wt:
            torch.testing.assert_close(gd["lp"].double(), wt["lp"], rtol=2e-3, atol=1e-5, msg=f"fp16 copy of master {i}")


CASES = [(None, 0.0, 2.0), ("value", 2e-4, 2.0), ("norm", 1e-3, 1.0), ("norm", 1e-3, 2.0), ("norm", 1e-3, 2.5), ("norm", 1e-3, INF)]


@pytest.mark.parametrize("clip,cv,p", CASES)
@pytest.mark.parametrize("nesterov", [False, True])
def test_segment_sgd_matches_float64_reference(osr, clip, cv, p, nesterov):
    ms = _masters()
    ms[3]["g"][7:9] = 0.0  # rows without gradient
    args = dict(lr=0.02, mu=0.9, gs=1.0 / (1024.0 * 2), clip=clip, cv=cv, p=p, nesterov=nesterov, bias_factor=2.0, wd=1e-4, wd_bias=0.0)
    got, _ = _run_kernel(osr, ms, **args)
    want, coefs = _reference(ms, **args)
    _check(got, want, ms)
    if clip == "norm":
        assert sum(c < 1 for c in coefs) >= 4, coefs  # the threshold bites on most segments
        assert coefs[1] != pytest.approx(coefs[2], rel=1e-3)  # two parameters of one master: a norm each


@pytest.mark.parametrize("p", [1.0, 2.0, 2.5, INF])
def test_norm_threshold_zero_gradient_and_huge_element(osr, p):
    ms = _masters(1)
    ms[1]["g"][4:5] = 0.0                 # a zero-gradient parameter: coefficient cv / 1e-6, nothing clipped
    gs, cv = 1.0 / 1024.0, 0.05
    # segment (1, 0-4): norm just below the threshold; segment (3): just above; segment (0): row-scaled, far above
    def scale_to(x, rs, target):
        d = x.double() * gs * (rs.double().view(-1, *([1] * (x.dim() - 1))) if rs is not None else 1.0)
        n = float(d.abs().max()) if math.isinf(p) else float((d.abs() ** p).sum() ** (1.0 / p))
        return (x.double() * (target / n)).float()
    ms[1]["g"][0:4] = scale_to(ms[1]["g"][0:4], None, cv * (1 - 1e-3))
    ms[3]["g"] = scale_to(ms[3]["g"], None, cv * (1 + 1e-3))
    if p != 2.5:  # (|g|^2.5 of 1e30 is outside fp32: the generic power is taken in fp32, documented)
        ms[2]["g"][1] = 1e30
    args = dict(lr=0.05, mu=0.9, gs=gs, clip="norm", cv=cv, p=p, nesterov=False, bias_factor=1.0, wd=1e-4, wd_bias=1e-4)
    got, _ = _run_kernel(osr, ms, **args)
    want, coefs = _reference(ms, **args)
    assert coefs[1] > 1 and coefs[5] < 1 and coefs[2] > 1e4
    _check(got, want, ms)


def test_apply_flag_zero_changes_nothing_and_nan_clears_the_flag(osr):
    ms = _masters(2)
    args = dict(lr=0.05, mu=0.9, gs=1.0, clip="norm", cv=1e-3, p=2.0, nesterov=True, bias_factor=2.0, wd=1e-4, wd_bias=0.0)
    got, _ = _run_kernel(osr, ms, flag_value=0, **args)
    for gd, m in zip(got, ms):
        assert torch.equal(gd["p"], m["p"]) and torch.equal(gd["v"], m["v"])
    ms[3]["g"][50, 3] = float("nan")  # the norm pass is the overflow check of this path
    got, _ = _run_kernel(osr, ms, **args)
    for gd, m in zip(got, ms):
        assert torch.equal(gd["p"], m["p"]) and torch.equal(gd["v"], m["v"])


@pytest.mark.parametrize("clip,p", [("norm", 2.0), ("norm", 2.5), ("value", 2.0)])
def test_two_runs_give_identical_bits(osr, clip, p):
    ms = _masters(3)
    args = dict(lr=0.02, mu=0.9, gs=0.5, clip=clip, cv=1e-2, p=p, nesterov=True, bias_factor=2.0, wd=1e-4, wd_bias=0.0)
    a, pa = _run_kernel(osr, ms, **args)
    b, pb = _run_kernel(osr, ms, **args)
    for x, y in zip(a, b):
        assert all(torch.equal(x[k], y[k]) for k in x if x[k] is not None)
    if clip == "norm":
        assert torch.equal(pa.partials.cpu(), pb.partials.cpu())


def test_plan_refuses_bad_rows(osr):
    p = torch.zeros((5, 8), device=DEV)
    with pytest.raises(osr.ops.OsrError):
        osr.ops.sgd_segment_plan([(p, p.clone(), p.clone(), None, None, 3, 6, 1.0, 0.0, False)], torch.device(DEV))


# ---- whole step, both trainers ------------------------------------------------------------------------------
def _cfg(yaml, *opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "SOLVER.BASE_LR", "0.01", "SOLVER.WARMUP_ITERS", "0", "OPENDET_BENCHMARK", "True"] + list(opts))
    return cfg


# masters that hold several detectron2 parameters: master -> [(name, rows)] (export_state_dict's split)
MULTI = {
    "voc_coco.yaml": {"rpn_tail.w": [("proposal_generator.rpn_head.anchor_deltas.weight", (0, 4)), ("proposal_generator.rpn_head.centerness.weight", (4, 5))],
                      "pred.w": [("roi_heads.box_predictor.bbox_pred.weight", (0, 4)), ("roi_heads.box_predictor.iou_pred.weight", (4, 5))]},
    "base_rcnn_fpn.yaml": {"rpn_tail.w": [("proposal_generator.rpn_head.objectness_logits.weight", (0, 3)),
                                          ("proposal_generator.rpn_head.anchor_deltas.weight", (3, 15))]},
}


def _d2_grads(t, gs):
    """The gradient of every detectron2 parameter: the flat buffer times gs (and the folded FrozenBN scale per row), exported
    through the trainer's own name / layout map (export_state_dict reads self.master)."""
    masters = t.master
    g = {}
    for k, pm in masters.items():
        x = t.grad[k].double() * gs
        if k in t.row_scale:
            x = x * t.row_scale[k].double().view(-1, *([1] * (pm.dim() - 1)))
        g[k] = x.float()
    t.master = g
    try:
        return {k: v.double() for k, v in t.export_state_dict().items()}, {k: v.double() for k, v in g.items()}
    finally:
        t.master = masters


@pytest.mark.parametrize("yaml", ["voc_coco.yaml", "base_rcnn_fpn.yaml"])
@pytest.mark.parametrize("clip,p,nesterov", [("norm", 2.0, True), ("norm", INF, False), ("value", 2.0, True)])
def test_whole_step_matches_torch_per_parameter(osr, yaml, clip, p, nesterov):
    from tests.test_train_loop import _data
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.solver import build_optimizer
    cfg = _cfg(yaml, "SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", clip, "SOLVER.CLIP_GRADIENTS.NORM_TYPE", str(p),
               "SOLVER.BIAS_LR_FACTOR", "2.0", "SOLVER.WEIGHT_DECAY_BIAS", "0.0", "SOLVER.NESTEROV", str(nesterov))
    torch.manual_seed(0)
    model = M.build_model(cfg)
    model.train()
    opt = build_optimizer(cfg, model)
    data = _data(list(range(20)))
    losses = model(data)
    total = sum(losses.values())
    assert torch.isfinite(total)
    opt.zero_grad()
    total.backward()
    t = model.trainer()
    gs = 1.0 / t._scale_used
    before = {k: v.clone() for k, v in t.export_state_dict().items()}
    grads, _ = _d2_grads(t, gs)
    assert set(grads) == set(before)
    # a clip value that bites on most parameters
    if clip == "norm":
        norms = sorted(float(g.abs().max()) if math.isinf(p) else float(g.norm(p)) for g in grads.values())
    else:
        norms = sorted(float(g.abs().max()) for g in grads.values())
    cv = 0.5 * norms[len(norms) // 2]
    opt.clip = (clip, cv, p)
    opt.step()
    assert not t.poll_overflow(wait=True)
    after = t.export_state_dict()
    # reference: detectron2's clipper and torch's SGD, per group, on the exported fp32 parameters
    params = {k: torch.nn.Parameter(v.clone().float()) for k, v in before.items()}
    clipped = 0
    for k, prm in params.items():
        prm.grad = grads[k].float().clone()
        if clip == "norm":
            n = torch.nn.utils.clip_grad_norm_([prm], cv, p)
            clipped += float(n) + 1e-6 > cv
        else:
            clipped += bool((prm.grad.abs() > cv).any())
            torch.nn.utils.clip_grad_value_([prm], cv)
    assert clipped > 0.5 * len(params), (clipped, len(params))
    bias = [v for k, v in params.items() if k.endswith(".bias")]
    rest = [v for k, v in params.items() if not k.endswith(".bias")]
    s = cfg.SOLVER
    sgd = torch.optim.SGD([dict(params=rest), dict(params=bias, lr=2.0 * s.BASE_LR, weight_decay=0.0)], lr=s.BASE_LR, momentum=s.MOMENTUM,
                          weight_decay=s.WEIGHT_DECAY, nesterov=nesterov)
    sgd.step()
    eps = torch.finfo(torch.float32).eps
    for k, prm in params.items():
        want, got, p0 = prm.detach(), after[k], before[k]
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-7, msg=k)
        # the update itself, to the rounding of the parameter
        dw, dg = (want - p0).double(), (got - p0).double()
        bound = 1e-3 * dw.abs() + 4 * eps * p0.double().abs() + 1e-12
        assert bool(((dg - dw).abs() <= bound).all()), (k, float((dg - dw).abs().max()), float(dw.abs().max()))
    # the parameters that share a master are clipped on their own (the reference above clips each alone): their coefficients differ
    if clip == "norm":
        for master, parts in MULTI[yaml].items():
            cs = [min(1.0, cv / (float(grads[name].abs().max() if math.isinf(p) else grads[name].norm(p)) + 1e-6)) for name, _ in parts]
            assert rows_of(t, master) == [r for _, r in parts], master
            assert cs[0] != cs[1] or cs[0] == 1.0, (master, cs)


def rows_of(t, master):
    b = t._param_rows()[master]
    return list(zip(b[:-1], b[1:]))


def _twin(cfg):
    from openset_rcnn_amd.host import modeling as M
    torch.manual_seed(0)
    a = M.build_model(cfg)
    b = M.build_model(cfg)
    b.load_state_dict(a.state_dict())
    return a, b


@pytest.mark.parametrize("yaml", ["voc_coco.yaml", "base_rcnn_fpn.yaml"])
def test_options_off_is_the_plain_update_bit_for_bit(osr, yaml):
    """Every option off (solver_options None) and the neutral SolverOptions() (factor 1, one weight decay, no clip, no Nesterov) share
    one plan and give the same parameters after three steps. (tests/test_update_pin.py holds both to the plain update's bits.)"""
    from tests.test_train_loop import _data
    from openset_rcnn_amd.host.solver import SolverOptions, build_optimizer
    cfg = _cfg(yaml)
    ma, mb = _twin(cfg)
    data = _data(list(range(20)))
    outs = []
    for model, forced in ((ma, None), (mb, SolverOptions())):
        model.train()
        model.sampler_generator.manual_seed(5)
        opt = build_optimizer(cfg, model)
        assert opt.solver_options() is None
        for _ in range(3):
            total = sum(model(data).values())
            opt.zero_grad()
            total.backward()
            if forced is None:
                opt.step()
            else:  # the same step, the neutral options spelled out
                t = model.trainer()
                g = opt.param_groups[0]
                t.lr, t.momentum, t.weight_decay = g["lr"], g["momentum"], g["weight_decay"]
                t.solver_options = forced
                t._update(t.all_reduce_grads())
                t.grads_ready = False
        t = model.trainer()
        assert len(t._sgd_plans[1]) == 1
        outs.append(({k: v.clone() for k, v in t.master.items()}, {k: v.clone() for k, v in t.mom.items()}))
    for k in outs[0][0]:
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


# ---- run_net.py ------------------------------------------------------------------------------------------------
def test_run_net_trains_with_every_option_on(osr, toy_voc_root, tmp_path, monkeypatch, caplog):  # noqa: F811
    import run_net
    monkeypatch.setenv("DETECTRON2_DATASETS", toy_voc_root)
    out = str(tmp_path / "out")
    base, max_iter = 0.0005, 3
    args = ["--config-file", os.path.join(ROOT, "configs", "voc_coco.yaml"), "--opendet-benchmark", "--test-batch", "2",
            "OUTPUT_DIR", out, "SEED", "3", "DATASETS.TRAIN", "('voc_2007_train',)", "DATASETS.TEST", "('voc_2007_test',)",
            "SOLVER.IMS_PER_BATCH", "2", "SOLVER.BASE_LR", str(base), "SOLVER.WARMUP_ITERS", "0", "SOLVER.CHECKPOINT_PERIOD", "0",
            "SOLVER.MAX_ITER", str(max_iter), "INPUT.MIN_SIZE_TRAIN", "(96,)", "INPUT.MAX_SIZE_TRAIN", "128", "INPUT.MIN_SIZE_TEST", "96",
            "INPUT.MAX_SIZE_TEST", "128",
            "SOLVER.CLIP_GRADIENTS.ENABLED", "True", "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", "0.01",
            "SOLVER.BIAS_LR_FACTOR", "2.0", "SOLVER.NESTEROV", "True", "SOLVER.LR_SCHEDULER_NAME", "WarmupCosineLR"]
    with caplog.at_level(logging.INFO, logger="openset_rcnn"):
        assert run_net.main(args) == 0
    blob = torch.load(os.path.join(out, "model_final.pth"), map_location="cpu", weights_only=False)
    assert all(torch.isfinite(v).all() for v in blob["model"].values() if v.is_floating_point())
    # the last iteration's logged lr follows the cosine schedule: BASE_LR * 0.5 * (1 + cos(pi * it / MAX_ITER))
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith(f"iter {max_iter} ")]
    assert lines, [r.getMessage() for r in caplog.records][:20]
    lr = float(lines[-1].split(" lr ")[1].split()[0])
    assert lr == pytest.approx(base * 0.5 * (1 + math.cos(math.pi * (max_iter - 1) / max_iter)), abs=1e-6)
