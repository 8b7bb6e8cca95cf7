"""MODEL.BACKBONE.FREEZE_AT reaches the trainer ([d2] ResNet.freeze: >= 1 freezes the stem, >= k freezes stage res<k>).

CPU: the value's checks (negative refused when the model is built, above 5 acts as 5). GPU: the trainable parameter count for every
value and both trainers; every master's gradient against autograd over the oracle forward at FREEZE_AT 0 (the stem trains:
csrc/osr_stem_bwd.hip), 1 (res2 trains through the per-conv path) and 4; the module loop (model(data) / backward / optimizer.step)
at FREEZE_AT 0, 1 and 5 for the Openset and the stock heads; the gradient buckets' schedule with the stem and res2 in the buffer; the
frozen-prefix prefetch at FREEZE_AT 1; momentum state keyed by name. The stem kernels themselves: tests/test_stem_bwd.py."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# trainable parameters of the VOC-COCO model (41 621 279 at FREEZE_AT 2), +- stem 9 408, res2 212 992, res3 1 212 416,
# res4 7 077 888, res5 14 942 208 (test_counts_are_the_module_arithmetic sums them from the module's parameter shapes)
COUNTS = {0: 41_843_679, 1: 41_834_271, 2: 41_621_279, 3: 40_408_863, 4: 33_330_975, 5: 18_388_767}


def _cfg(yaml, *opts, device=DEV):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", device, "SOLVER.BASE_LR", "0.0001", "SOLVER.WARMUP_ITERS", "0", "OPENDET_BENCHMARK", "True"] + list(opts))
    return cfg


def _stage_params(model, stage: str) -> int:
    return sum(p.numel() for n, p in model.named_parameters() if n.startswith(f"backbone.bottom_up.{stage}.") and not n.endswith(".norm.weight")
               and not n.endswith(".norm.bias"))


# ---- CPU -------------------------------------------------------------------------------------------------------
def test_freeze_at_is_read_from_the_config(osr):
    from openset_rcnn_amd.host import modeling as M
    for yaml in ("voc_coco.yaml", "base_rcnn_fpn.yaml"):
        for v, want in ((0, 0), (1, 1), (2, 2), (5, 5), (6, 5), (100, 5)):
            model = M.build_model(_cfg(yaml, "MODEL.BACKBONE.FREEZE_AT", str(v), device="cpu"))
            assert model._freeze_at == want, (yaml, v)
        with pytest.raises(ValueError, match="FREEZE_AT"):
            M.build_model(_cfg(yaml, "MODEL.BACKBONE.FREEZE_AT", "-1", device="cpu"))


def test_trainer_refuses_negative_values(osr):
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    from openset_rcnn_amd.host.train_std import StandardRCNNTrainer
    for cls in (OpensetRCNNTrainer, StandardRCNNTrainer):
        with pytest.raises(ValueError):  # (checked before anything is built: no parameters, no GPU needed)
            cls({}, device="cpu", freeze_at=-1)
    assert OpensetRCNNTrainer._check_freeze_at(9) == 5 and OpensetRCNNTrainer._check_freeze_at(2) == 2
    assert OpensetRCNNTrainer._check_freeze_at(0) == 0


def test_counts_are_the_module_arithmetic(osr):
    """COUNTS against the module's parameter shapes (FrozenBN affine terms are buffers in [d2]; here they are not trained either)."""
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(_cfg("voc_coco.yaml", device="cpu"))
    per = {s: _stage_params(model, s) for s in ("stem", "res2", "res3", "res4", "res5")}
    assert per == {"stem": 9_408, "res2": 212_992, "res3": 1_212_416, "res4": 7_077_888, "res5": 14_942_208}
    assert COUNTS[0] == COUNTS[1] + per["stem"]
    assert COUNTS[1] == COUNTS[2] + per["res2"]
    assert COUNTS[3] == COUNTS[2] - per["res3"]
    assert COUNTS[4] == COUNTS[3] - per["res4"]
    assert COUNTS[5] == COUNTS[4] - per["res5"]


# ---- GPU: parameter counts and master layout -----------------------------------------------------------------
@pytest.mark.gpu
def test_trainable_parameter_counts_follow_freeze_at(osr):
    from openset_rcnn_amd.host import modeling as M
    std_at2 = None
    for v in (0, 1, 2, 3, 4, 5, 7):
        torch.manual_seed(0)
        model = M.build_model(_cfg("voc_coco.yaml", "MODEL.BACKBONE.FREEZE_AT", str(v)))
        tr = model.trainer()
        assert tr.freeze_at == min(v, 5) and tr.num_params == COUNTS[min(v, 5)], (v, tr.num_params)
        bb = [k for k in tr.master if k.startswith("backbone.bottom_up.")]
        stages = sorted({k.split(".")[2] for k in bb})
        assert stages == [f"res{s}" for s in range(max(2, min(v, 5) + 1), 6)] + (["stem"] if v == 0 else []), (v, stages)
        # the bottom-up masters sit at the start of the flat buffer, lowest stage first (they complete last in the backward)
        assert list(tr.master)[: len(bb)] == bb
        if v == 0:
            assert bb[0] == "backbone.bottom_up.stem.conv1.w" and tuple(tr.master[bb[0]].shape) == (64, 8, 1, 32)
        if v == 1:
            assert bb[:4] == [f"backbone.bottom_up.res2.0.{c}.w" for c in ("shortcut", "conv1", "conv2", "conv3")]
        del model, tr
        smodel = M.build_model(_cfg("base_rcnn_fpn.yaml", "MODEL.BACKBONE.FREEZE_AT", str(v)))
        n = smodel.trainer().num_params
        if v == 2:
            std_at2 = n
        del smodel
    torch.cuda.empty_cache()
    assert std_at2 is not None
    # the stock heads share the trunk: the same per-stage differences
    smodel = M.build_model(_cfg("base_rcnn_fpn.yaml", "MODEL.BACKBONE.FREEZE_AT", "4"))
    assert smodel.trainer().num_params == std_at2 - (COUNTS[2] - COUNTS[4])
    smodel = M.build_model(_cfg("base_rcnn_fpn.yaml", "MODEL.BACKBONE.FREEZE_AT", "1"))
    assert smodel.trainer().num_params == std_at2 + (COUNTS[1] - COUNTS[2])
    smodel = M.build_model(_cfg("base_rcnn_fpn.yaml", "MODEL.BACKBONE.FREEZE_AT", "0"))
    assert smodel.trainer().num_params == std_at2 + (COUNTS[0] - COUNTS[2])


@pytest.mark.gpu
def test_default_trainer_layout_is_unchanged(osr):
    """The constructors' default (bench.py, the tests) and a yaml that leaves FREEZE_AT alone: the same masters, in the same order."""
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    from openset_rcnn_amd.host.weights import random_params
    tr = OpensetRCNNTrainer(random_params(0), dtype=torch.float16, device=DEV)
    assert tr.freeze_at == 2 and tr.num_params == COUNTS[2]
    assert list(tr.master)[0] == "backbone.bottom_up.res3.0.shortcut.w"
    torch.manual_seed(0)
    model = M.build_model(_cfg("voc_coco.yaml"))
    mt = model.trainer()
    assert list(mt.master) == list(tr.master)
    assert mt.grad_flat.numel() == tr.grad_flat.numel()
    assert all(mt.grad[k].data_ptr() - mt.grad_flat.data_ptr() == tr.grad[k].data_ptr() - tr.grad_flat.data_ptr() for k in tr.grad)
    assert [(b["lo"], b["hi"], b["names"]) for b in mt.buckets.buckets] == [(b["lo"], b["hi"], b["names"]) for b in tr.buckets.buckets]


# ---- GPU: one step's gradients against autograd over the oracle -----------------------------------------------
@pytest.fixture(scope="module")
def batch(osr):
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    from oracle import osr_oracle as O
    from openset_rcnn_amd.host.weights import random_params
    g = torch.Generator().manual_seed(23)
    n, h, w, gmax = 2, 128, 160, 4
    images = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8)
    gt = torch.zeros(n, gmax, 4)
    gcls = torch.zeros(n, gmax, dtype=torch.int64)
    gcnt = [3, 2]
    for i, c in enumerate(gcnt):
        ctr = torch.rand(c, 2, generator=g) * torch.tensor([w * 0.7, h * 0.7]) + 16
        size = torch.rand(c, 2, generator=g) * 60 + 24
        b = torch.cat((ctr - size / 2, ctr + size / 2), dim=1)
        b[:, 0::2].clamp_(0, w)
        b[:, 1::2].clamp_(0, h)
        gt[i, :c] = b
        gcls[i, :c] = torch.randint(0, 20, (c,), generator=g)
    shapes = O.level_shapes(h, w)
    r = sum(a * b for a, b in shapes)
    cap = sum(min(2000, a * b) for a, b in shapes)
    keys = dict(rpn_reg=torch.rand(n, r, generator=g), rpn_obj=torch.rand(n, r, generator=g), roi=torch.rand(n, cap + gmax, generator=g))
    dev = dict(images=images.to(DEV), hw=torch.tensor([(h, w)] * n, dtype=torch.int32).to(DEV), gt=gt.to(DEV), gcls=gcls.to(DEV),
               gcnt=torch.tensor(gcnt, dtype=torch.int32).to(DEV), keys={k: v.to(DEV) for k, v in keys.items()})
    return dict(params=random_params(0), images=images, shapes=shapes, n=n, h=h, w=w, dev=dev)


def _args(b):
    d = b["dev"]
    return (d["images"], d["hw"], b["h"], b["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])


@pytest.mark.gpu
@pytest.mark.parametrize("freeze_at", [0, 1, 4])
def test_gradients_match_autograd_at_freeze_at(batch, freeze_at):
    """Tolerance as tests/test_train_step.py: per tensor cosine >= 0.999 and norm within 1 % (fp16 activations and gradients,
    loss-scaled, against the fp32 oracle with fp16-rounded weights and activations)."""
    from tests.test_train_step import _oracle_grads
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    from openset_rcnn_amd.host.weights import pack_conv_weight, pack_fc1_weight, pack_stem_weight
    tr = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=0.002, loss_scale=512.0, freeze_at=freeze_at)
    n = batch["n"]
    losses, saved = tr._forward(*_args(batch))
    tr._backward(saved, n)
    torch.cuda.synchronize()
    s = dict(labels=saved["labels"].cpu(), obj_labels=saved["obj_labels"].cpu(), matched_boxes=saved["matched_boxes"].cpu(),
             ctr_target=saved["ctr_target"].cpu(), boxes=saved["boxes"].cpu(), batch_idx=saved["smp"]["batch_idx"].cpu(), cls=saved["cls"].cpu(),
             ious=saved["ious"].cpu(), gt_boxes=saved["smp"]["gt_boxes"].view(-1, 4).cpu())
    ref_losses, ref = _oracle_grads(batch["params"], batch["images"], batch["shapes"], s, tr.eng.cfg, n)
    for k, v in ref_losses.items():
        assert float(losses[k]) == pytest.approx(float(v), rel=3e-2, abs=1e-4), k
    S = tr.loss_scale
    names = {"fc1.b": "roi_heads.box_head.fc1.bias", "fc2.w": "roi_heads.box_head.fc2.weight", "fc2.b": "roi_heads.box_head.fc2.bias",
             "enc.w": "roi_heads.dml.encoder.weight", "enc.b": "roi_heads.dml.encoder.bias", "dec.w": "roi_heads.dml.decoder.weight",
             "dec.b": "roi_heads.dml.decoder.bias", "cls.w": "roi_heads.softmaxcls.cls_score.weight", "cls.b": "roi_heads.softmaxcls.cls_score.bias",
             "protos": "roi_heads.dml.representatives"}
    report, bad = [], []
    for k, gten in tr.grad.items():
        got = gten.detach().cpu() / S
        if k == "rpn_tail.w":
            want = torch.cat((ref["proposal_generator.rpn_head.anchor_deltas.weight"].view(4, 256), ref["proposal_generator.rpn_head.centerness.weight"].view(1, 256)))
        elif k == "rpn_tail.b":
            want = torch.cat((ref["proposal_generator.rpn_head.anchor_deltas.bias"], ref["proposal_generator.rpn_head.centerness.bias"]))
        elif k == "pred.w":
            want = torch.cat((ref["roi_heads.box_predictor.bbox_pred.weight"], ref["roi_heads.box_predictor.iou_pred.weight"]))
        elif k == "pred.b":
            want = torch.cat((ref["roi_heads.box_predictor.bbox_pred.bias"], ref["roi_heads.box_predictor.iou_pred.bias"]))
        elif k == "fc1.w":
            want = pack_fc1_weight(ref["roi_heads.box_head.fc1.weight"], 256, 7, torch.float32)
        elif k in names:
            want = ref[names[k]]
        elif k == "backbone.bottom_up.stem.conv1.w":
            want = pack_stem_weight(ref["backbone.bottom_up.stem.conv1.weight"], torch.float32)
            assert float(got.view(64, 8, 8, 4)[:, 7].abs().max()) == 0 and float(got.view(64, 8, 8, 4)[:, :, 7].abs().max()) == 0
            assert float(got.view(64, 8, 8, 4)[..., 3].abs().max()) == 0
        elif k.endswith(".w"):
            want = pack_conv_weight(ref[k[:-2] + ".weight"], torch.float32)
        else:
            want = ref[k[:-2] + ".bias"]
        assert got.shape == want.shape, k
        cos = float(F.cosine_similarity(got.flatten(), want.flatten(), dim=0))
        ratio = float(got.norm() / want.norm().clamp(min=1e-20))
        report.append(f"{k:48s} cos {cos:.4f}  |got|/|ref| {ratio:.3f}  |ref| {float(want.norm()):.3e}")
        # (the stem's gradient goes through the max pool's argmax over fp16 stem outputs, which the fp32-accumulated oracle can break
        # the other way at near-ties: a few gradients land one pixel away; measured cos 0.9988, norm within 0.1 %. The kernels
        # themselves agree with fp64 on the same inputs to 1e-6: tests/test_stem_bwd.py)
        cos_min = 0.995 if k == "backbone.bottom_up.stem.conv1.w" else 0.999
        if not (cos >= cos_min and 0.99 <= ratio <= 1.01):
            bad.append(report[-1])
    print("\n".join(report))
    stages = {k.split(".")[2] for k in tr.grad if k.startswith("backbone.bottom_up.")}
    assert stages == {f"res{s}" for s in range(max(2, freeze_at + 1), 6)} | ({"stem"} if freeze_at == 0 else set())
    assert not bad, "gradient mismatch:\n" + "\n".join(bad)


@pytest.mark.gpu
def test_freeze_at_5_backward_ends_at_the_laterals(batch):
    """No bottleneck is saved or differentiated: the backward stops after the FPN, every lateral (of a frozen stage) still trains."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    tr = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=0.002, loss_scale=512.0, freeze_at=5)
    assert not any(k.startswith("backbone.bottom_up.") for k in tr.master)
    losses, saved = tr._forward(*_args(batch))
    assert saved["blocks"] == []
    tr._backward(saved, batch["n"])
    torch.cuda.synchronize()
    assert torch.isfinite(tr.grad_flat).all()
    for lvl in (2, 3, 4, 5):
        assert float(tr.grad[f"backbone.fpn_lateral{lvl}.w"].abs().sum()) > 0, lvl
    hist = [sum(float(v) for v in tr.step(*_args(batch)).values()) for _ in range(3)]
    assert all(h == h for h in hist) and hist[-1] < hist[0], hist


@pytest.mark.gpu
def test_freeze_at_1_prefetch_of_the_stem_gives_the_same_step(batch):
    """At FREEZE_AT 1 the frozen prefix is the fused stem alone: taking it from the previous step's prefetch changes nothing."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer

    def run(prefetch):
        tr = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0, freeze_at=1)
        tr.step(*_args(batch), next_images=batch["dev"]["images"] if prefetch else None)
        took = tr._prefetched is not None
        out = tr.step(*_args(batch))
        torch.cuda.synchronize()
        return {k: float(v) for k, v in out.items()}, took

    a, took_a = run(False)
    b, took_b = run(True)
    assert took_b and not took_a
    # (the second step's inputs are the first update's parameters, which carry RoIAlign's atomic summation order)
    assert b == pytest.approx(a, rel=1e-3), (a, b)


@pytest.mark.gpu
def test_momentum_state_is_keyed_by_freeze_at(batch):
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    t1 = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0, freeze_at=1)
    t1.step(*_args(batch))
    state = t1.export_optimizer_state()
    assert "backbone.bottom_up.res2.0.conv1.w" in state and float(state["backbone.bottom_up.res2.0.conv1.w"].abs().sum()) > 0
    sd = t1.export_state_dict()
    assert "backbone.bottom_up.res2.2.conv3.weight" in sd and "backbone.bottom_up.stem.conv1.weight" not in sd
    t1b = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0, freeze_at=1)
    t1b.load_optimizer_state(state)
    assert all(torch.equal(t1b.mom[k].cpu(), v) for k, v in state.items() if k in t1b.mom)
    t2 = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0)
    with pytest.raises(KeyError):
        t2.load_optimizer_state(state)


@pytest.mark.gpu
def test_freeze_at_0_checkpoint_round_trips(batch):
    """A FREEZE_AT 0 trainer exports the stem under its detectron2 name and layout, its momentum (stem included) loads into another
    FREEZE_AT 0 trainer, not into a FREEZE_AT 2 one; the view's padding stays exactly zero through the updates."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    stem = "backbone.bottom_up.stem.conv1"
    t0 = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0, freeze_at=0)
    w0 = t0.eng.w[stem + ".w"].clone()
    for _ in range(2):
        t0.step(*_args(batch))
    torch.cuda.synchronize()
    assert t0.overflow_steps == 0
    v = t0.eng.w[stem + ".w"].view(64, 8, 8, 4)
    assert not torch.equal(t0.eng.w[stem + ".w"], w0), "the working stem view was not refreshed"
    assert float(v[:, 7].abs().max()) == 0 and float(v[:, :, 7].abs().max()) == 0 and float(v[..., 3].abs().max()) == 0
    m = t0.master[stem + ".w"].view(64, 8, 8, 4)
    assert float(m[:, 7].abs().max()) == 0 and float(m[:, :, 7].abs().max()) == 0 and float(m[..., 3].abs().max()) == 0
    sd = t0.export_state_dict()
    assert tuple(sd[stem + ".weight"].shape) == (64, 3, 7, 7)
    assert torch.equal(sd[stem + ".weight"], t0.master[stem + ".w"].view(64, 8, 8, 4)[:, :7, :7, :3].permute(0, 3, 1, 2).cpu())
    assert not torch.equal(sd[stem + ".weight"], batch["params"][stem + ".weight"].float())
    state = t0.export_optimizer_state()
    assert float(state[stem + ".w"].abs().sum()) > 0
    t0b = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0, freeze_at=0)
    t0b.load_optimizer_state(state)
    assert all(torch.equal(t0b.mom[k].cpu(), v_) for k, v_ in state.items() if k in t0b.mom)
    t2 = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0)
    with pytest.raises(KeyError):
        t2.load_optimizer_state(state)


# ---- GPU: the module loop ---------------------------------------------------------------------------------------
def _bottom_up(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k.startswith("backbone.bottom_up.")}


@pytest.mark.gpu
@pytest.mark.parametrize("yaml", ["voc_coco.yaml", "base_rcnn_fpn.yaml"])
@pytest.mark.parametrize("freeze_at", [0, 1, 5])
def test_module_loop_trains_exactly_the_unfrozen_stages(osr, yaml, freeze_at):
    from tests.test_train_loop import _data
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.solver import build_optimizer
    cfg = _cfg(yaml, "MODEL.BACKBONE.FREEZE_AT", str(freeze_at))
    torch.manual_seed(0)
    model = M.build_model(cfg)
    data = _data(list(range(20)))
    before = _bottom_up(model)
    lat_before = model.state_dict()["backbone.fpn_lateral2.weight"].detach().cpu().clone()
    model.train()
    opt = build_optimizer(cfg, model)
    for _ in range(2):
        losses = model(data)
        total = sum(losses.values())
        assert torch.isfinite(total)
        opt.zero_grad()
        total.backward()
        opt.step()
    model.eval()
    after = _bottom_up(model)
    changed = {k for k in after if after[k].is_floating_point() and not torch.equal(after[k], before[k])}
    if freeze_at == 5:
        assert not changed, sorted(changed)[:8]
    else:
        stem_changed = {k for k in changed if k.startswith("backbone.bottom_up.stem.")}
        assert stem_changed == ({"backbone.bottom_up.stem.conv1.weight"} if freeze_at == 0 else set()), stem_changed
        for b in range(3):
            for c in ("conv1", "conv2", "conv3"):
                assert f"backbone.bottom_up.res2.{b}.{c}.weight" in changed, (b, c)
        assert "backbone.bottom_up.res2.0.shortcut.weight" in changed
        assert not any(k.endswith(".norm.weight") or k.endswith(".norm.running_var") for k in changed)  # FrozenBN stays frozen
    assert not torch.equal(model.state_dict()["backbone.fpn_lateral2.weight"].detach().cpu(), lat_before)  # laterals train at every value
    if freeze_at == 0:  # the eval engine's stem view (read by the fused osr_stem_maxpool_fwd_raw) holds the trained weights
        ev = model.engine().w["backbone.bottom_up.stem.conv1.w"].float().cpu()
        trained = model.trainer().eng.w["backbone.bottom_up.stem.conv1.w"].float().cpu()
        assert torch.allclose(ev, trained, rtol=2e-3, atol=1e-6)
        assert float(ev.view(64, 8, 8, 4)[:, 7].abs().max()) == 0 and float(ev.view(64, 8, 8, 4)[:, :, 7].abs().max()) == 0
    # eval mode runs the fused stem / res2 kernels on the module's (now trained) weights
    out = model([{k: v for k, v in d.items() if k != "instances"} for d in data])
    assert len(out) == 2 and out[0]["instances"].has("pred_boxes")


# ---- GPU: gradient buckets with res2 in the buffer --------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture()
def one_rank_group():
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("freeze_at", [0, 1])
def test_buckets_with_res2_trainable_are_issued_under_the_backward(osr, batch, one_rank_group, freeze_at):
    """As tests/test_backward_schedule.py, at FREEZE_AT 1: every bucket once, before all_reduce_grads(), behind the last weight-gradient
    launch of each of its parameters; res2 (the start of the buffer) is in the last bucket, res3's goes out with res2's data gradients
    still to come."""
    from openset_rcnn_amd.host import ops, parallel
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    assert parallel.is_dist()
    tr = OpensetRCNNTrainer(batch["params"], dtype=torch.float16, device=DEV, lr=0.002, loss_scale=512.0, freeze_at=freeze_at)
    name_of = {t.data_ptr(): k for k, t in tr.grad.items()}
    log = []
    real = dict(dgrad=ops.conv2d_dgrad, wgrad=ops.conv2d_wgrad, tn=ops.gemm_f32_tn, issue=tr.buckets.issue, finish=tr.buckets.finish)

    def dgrad(*a, **k):
        log.append(("dgrad", None))
        return real["dgrad"](*a, **k)

    def wgrad(*a, **k):
        dw = k.get("dw")
        log.append(("wgrad", name_of.get(dw.data_ptr()) if dw is not None else None))
        return real["wgrad"](*a, **k)

    def tn(*a, **k):
        out = k.get("out")
        log.append(("wgrad", name_of.get(out.data_ptr()) if out is not None else None))
        return real["tn"](*a, **k)

    def issue(b):
        log.append(("issue", b))
        return real["issue"](b)

    def finish():
        log.append(("finish", None))
        return real["finish"]()

    ops.conv2d_dgrad, ops.conv2d_wgrad, ops.gemm_f32_tn = dgrad, wgrad, tn
    tr.buckets.issue, tr.buckets.finish = issue, finish
    try:
        tr.step(*_args(batch))
        torch.cuda.synchronize()
    finally:
        ops.conv2d_dgrad, ops.conv2d_wgrad, ops.gemm_f32_tn = real["dgrad"], real["wgrad"], real["tn"]

    nb = len(tr.buckets.buckets)
    fin = [i for i, e in enumerate(log) if e[0] == "finish"]
    assert len(fin) == 1
    issues = [(i, e[1]) for i, e in enumerate(log) if e[0] == "issue"]
    assert sorted(b for _, b in issues) == list(range(nb)), "every bucket exactly once"
    assert all(i < fin[0] for i, _ in issues)
    for b in range(nb):  # contiguous: a bucket's parameters are adjacent in the flat buffer
        offs = sorted(tr.buckets.buckets[b]["names"], key=lambda k: list(tr.master).index(k))
        idx = [list(tr.master).index(k) for k in offs]
        assert idx == list(range(idx[0], idx[0] + len(idx))), b
    last_wgrad = {}
    for i, e in enumerate(log):
        if e[0] == "wgrad" and e[1] is not None:
            last_wgrad[e[1]] = i
    res2 = [k for k in tr.master if k.startswith("backbone.bottom_up.res2.")]
    assert len(res2) == 10 and all(k in last_wgrad for k in res2), "every res2 weight gradient is launched"
    for i, b in issues:
        for nm in tr.buckets.buckets[b]["names"]:
            if nm in last_wgrad:
                assert last_wgrad[nm] < i, f"bucket {b} was issued before the last weight-gradient launch of {nm}"
    owner = tr.buckets.owner
    b_res2, b_res3 = owner["backbone.bottom_up.res2.0.shortcut.w"], owner["backbone.bottom_up.res3.0.conv1.w"]
    assert b_res2 == nb - 1 and b_res3 <= b_res2
    if freeze_at == 0:  # the stem opens the buffer: it completes last, in the last bucket
        assert list(tr.master)[0] == "backbone.bottom_up.stem.conv1.w" and owner["backbone.bottom_up.stem.conv1.w"] == nb - 1
    dg = [i for i, e in enumerate(log) if e[0] == "dgrad"]
    after = {b: sum(1 for j in dg if j > i) for i, b in issues}
    if b_res3 != b_res2:
        assert after[b_res3] >= 8, after  # res3.0's two input gradients, res2's lateral and its 3 + 3 + 2 data gradients
    assert sum(1 for b in range(nb) if after[b] == 0) <= 1, after
