"""OpensetRCNNTrainer(box_head="split"): the box head trained on the reference's fp32 operands -- pooled, h1 and box_feats saved in
fp32, FC1 / FC2 forward, data gradients and weight gradients on the split-precision kernels (ops.linear_split, linear_split_dgrad,
linear_split_wgrad). Four seeded 256 x 384 images through the detectron2-shaped model (tests/test_train_loop.py's set-up), a split
model and a default twin with the same parameters and the same sampling keys.

The box-head-local gradient check: g[fc1.w], g[fc2.w], both biases and d_pooled of a trainer against float64 on the CPU of the two
layers' backward, from that trainer's OWN saved pooled rows, the d_bf it fed in (both carry the loss scale) and its fp32 masters.
The float64 backward takes the two ReLU masks from the trainer's saved h1 / box_feats: an activation within rounding of zero may
come out on the other side of it in float64, and such a flip is a property of the forward, not of the gradient arithmetic checked
here. Errors are e(y) = max|y - y64| / max|y64|; the split trainer meets A = 1e-4, the default (fp16) trainer is farther away."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N, H, W = 4, 256, 384
A_BOUND = 1e-4
LOSS_KEYS = ("loss_rpn_loc", "loss_rpn_ctr", "loss_box_reg", "loss_iou", "loss_dml", "loss_cls")
QUANTITIES = ("fc1.w", "fc1.b", "fc2.w", "fc2.b", "d_pooled")


def _cfg(yaml="voc_coco.yaml"):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "SOLVER.BASE_LR", "0.0001", "SOLVER.WARMUP_ITERS", "0", "OPENDET_BENCHMARK", "True"])
    return cfg


def _data(seed=3):
    from openset_rcnn_amd.host.structures import Boxes, Instances
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(N):
        k = 2 + i
        ctr = torch.rand(k, 2, generator=g) * torch.tensor([W * 0.6, H * 0.6]) + 24
        size = torch.rand(k, 2, generator=g) * 80 + 24
        b = torch.cat((ctr - size / 2, ctr + size / 2), dim=1)
        b[:, 0::2].clamp_(0, W)
        b[:, 1::2].clamp_(0, H)
        inst = Instances((H, W), gt_boxes=Boxes(b), gt_classes=torch.tensor([(i + j) % 20 for j in range(k)], dtype=torch.int64))
        out.append({"image": torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8), "height": H, "width": W, "instances": inst})
    return out


def _err(y, y64):
    y = y.detach().cpu().double()
    assert y.numel() == y64.numel()
    return float((y.reshape(y64.shape) - y64).abs().max() / y64.abs().max().clamp(min=1e-300))  # (the fp16 path's d_pooled is a 1x1-conv view)


def _box_head_bwd64(tr, saved, probe):
    """The two layers' backward in float64 on the CPU (see the module docstring)."""
    f64 = lambda t: t.detach().cpu().double()  # noqa: E731
    pooled = f64(saved["pooled"]).reshape(saved["pooled"].shape[0], -1)
    w1, b1, w2 = f64(tr.master["fc1.w"]), f64(tr.master["fc1.b"]), f64(tr.master["fc2.w"])
    h1 = (pooled @ w1.t() + b1).clamp(min=0)
    d2 = f64(probe["d_bf"]) * (f64(saved["box_feats"]) > 0)
    dh1 = (d2 @ w2) * (f64(saved["h1"]) > 0)
    return {"fc2.w": d2.t() @ h1, "fc2.b": d2.sum(0), "fc1.w": dh1.t() @ pooled, "fc1.b": dh1.sum(0), "d_pooled": dh1 @ w1}


def _run(model, data, counters):
    """One forward + backward (no update) of the model's trainer: saved dtypes, losses, the box head's gradients and their errors."""
    ops = counters["ops"]
    tr = model.make_trainer(lr=1e-4)
    tr.box_head_probe = {}
    tensors = model._train_tensors(data, torch.Generator().manual_seed(9))
    ops.LINEAR_SPLIT_COUNT, ops.LINEAR_SPLIT_DGRAD_COUNT, ops.LINEAR_SPLIT_WGRAD_COUNT = ({"launches": 0, "flops": 0.0} for _ in range(3))
    with torch.no_grad():
        losses, saved = tr._forward(*tensors)
        tr._backward(saved, N)
    torch.cuda.synchronize()
    launches = (ops.LINEAR_SPLIT_COUNT["launches"], ops.LINEAR_SPLIT_DGRAD_COUNT["launches"], ops.LINEAR_SPLIT_WGRAD_COUNT["launches"])
    ops.LINEAR_SPLIT_COUNT = ops.LINEAR_SPLIT_DGRAD_COUNT = ops.LINEAR_SPLIT_WGRAD_COUNT = None
    probe, tr.box_head_probe = tr.box_head_probe, None
    ref = _box_head_bwd64(tr, saved, probe)
    got = {k: tr.grad[k] for k in QUANTITIES[:4]}
    got["d_pooled"] = probe["d_pooled"]
    errs = {k: _err(got[k], ref[k]) for k in QUANTITIES}
    dtypes = {k: saved[k].dtype for k in ("pooled", "h1", "box_feats")}
    return dict(tr=tr, tensors=tensors, losses={k: float(v) for k, v in losses.items()}, errs=errs, dtypes=dtypes, launches=launches,
                d_pooled_dtype=probe["d_pooled"].dtype, grad=tr.grad_flat.clone())


@pytest.fixture(scope="module")
def world(osr):
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    from openset_rcnn_amd.host import modeling as M
    cfg = _cfg()
    torch.manual_seed(0)
    split_model = M.build_model(cfg)
    default_model = M.build_model(cfg)
    default_model.load_state_dict(split_model.state_dict())
    split_model.roi_heads.box_head_precision = "split"
    data = _data()
    counters = dict(ops=osr.ops)
    return dict(split_model=split_model, data=data, split=_run(split_model, data, counters), default=_run(default_model, data, counters))


def test_make_trainer_follows_the_models_box_head_precision(osr, world):
    from openset_rcnn_amd.host import modeling as M
    s, d = world["split"], world["default"]
    assert s["tr"].box_head == "split" and s["tr"].eng.box_head == "split"
    assert all(dt == torch.float32 for dt in s["dtypes"].values()), s["dtypes"]
    assert s["d_pooled_dtype"] == torch.float32
    assert s["tr"].lowp.get("fc1.w") is None and s["tr"].lowp.get("fc2.w") is None
    assert s["launches"] == (2, 2, 2)  # FC1 and FC2: forward, data gradient, weight gradient
    assert d["tr"].box_head == "storage" and d["dtypes"]["pooled"] == torch.float16 and d["dtypes"]["h1"] == torch.float16
    assert d["launches"] == (0, 0, 0)  # a default-mode trainer in the same process launches no split kernel
    assert list(s["tr"].master) == list(d["tr"].master)  # same gradient layout and bucket order
    stock = M.build_model(_cfg("base_rcnn_fpn.yaml"))
    stock.roi_heads.box_head_precision = "split"
    with pytest.raises(ValueError, match="stock Faster R-CNN engine keeps its box head"):
        stock.make_trainer()


def test_box_head_gradients_meet_a_and_beat_the_default_trainer(world):
    s, d = world["split"]["errs"], world["default"]["errs"]
    print("\n[box head gradients against float64, 4 x 256x384, " + str(world["split"]["tr"].grad["fc1.w"].shape[0]) + " hidden units]")
    for k in QUANTITIES:
        print(f"  {k:9s} split {s[k]:.3e}   default (fp16) {d[k]:.3e}")
    for k in QUANTITIES:
        assert s[k] <= A_BOUND, (k, s[k])
    for k in QUANTITIES:
        assert d[k] > s[k], (k, d[k], s[k])


def test_losses_are_finite_and_agree_with_the_default_trainer(world):
    s, d = world["split"]["losses"], world["default"]["losses"]
    print("\n" + "  ".join(f"{k} {s[k]:.5f}/{d[k]:.5f}" for k in LOSS_KEYS))
    for k in LOSS_KEYS:
        assert s[k] == s[k] and abs(s[k]) != float("inf"), (k, s[k])
        assert s[k] == pytest.approx(d[k], rel=3e-2, abs=1e-4), k  # the tolerance of tests/test_train_step.py


def test_three_stream_and_single_stream_schedules_give_equal_gradients(world):
    tr, tensors = world["split"]["tr"], world["split"]["tensors"]

    def grads(side: bool):
        tr.side_wgrad = tr.overlap_targets = side
        tr.grad_flat.zero_()
        tr.step(*tensors, update=False)
        torch.cuda.synchronize()
        return tr.grad_flat.clone()

    g1, g3 = grads(False), grads(True)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(g1, g3), "the three-stream schedule changes the gradients"
    assert torch.equal(g3, world["split"]["grad"])


def test_update_refreshes_the_planes_and_the_model_evaluates(osr, world):
    from openset_rcnn_amd.host.weights import split_fp32_rows, split_fp32_rows_t
    tr, model, tensors = world["split"]["tr"], world["split_model"], world["split"]["tensors"]
    before = {k: tr.master[k].clone() for k in ("fc1.w", "fc2.w")}
    tr.lr = 0.01
    tr.step(*tensors)
    torch.cuda.synchronize()
    assert not tr.poll_overflow(wait=True)
    for k, fwd, wt in (("fc1.w", tr.eng.fc1_split, tr.wt_split["fc1"]), ("fc2.w", tr.eng.fc2_split, tr.wt_split["fc2"])):
        assert not torch.equal(tr.master[k], before[k]), k
        m = tr.master[k].cpu()
        hi, lo, _ = split_fp32_rows(m)
        thi, tlo, _ = split_fp32_rows_t(m)
        assert torch.equal(fwd[0].cpu(), hi) and torch.equal(fwd[1].cpu(), lo), k
        assert torch.equal(wt[0].cpu(), thi) and torch.equal(wt[1].cpu(), tlo), k
    model.load_trainer_state(tr)
    model.eval()
    eng = model.engine()
    assert eng.box_head == "split"
    hi, _, _ = split_fp32_rows(tr.master["fc2.w"].cpu())
    assert torch.equal(eng.fc2_split[0].cpu(), hi)  # the evaluation engine was packed from the trained masters
    osr.ops.LINEAR_SPLIT_COUNT = {"launches": 0, "flops": 0.0}
    out = model.inference(world["data"])
    torch.cuda.synchronize()
    launches = osr.ops.LINEAR_SPLIT_COUNT["launches"]
    osr.ops.LINEAR_SPLIT_COUNT = None
    assert launches == 2 and len(out) == N and all("instances" in o for o in out)
