"""A whole CascadeRCNNTrainer step (configs/cascade_rcnn_fpn.yaml) at n = 2, 128 x 160.

* Three stages: the rows every later stage trains on are the restatement's (tests/test_cascade_kernels.ref_refine: the previous stage's
  deltas decoded, clipped, empty boxes dropped, re-labelled at IOUS[s]) of the HIP run's own boxes and deltas; the six stage losses
  equal cross entropy / smooth-L1 in torch on the HIP run's logits, deltas and rows within 1e-4 relative; the gradient of EVERY
  master matches torch autograd over the oracle's forward (ResNet-50 + FPN, StandardRPNHead, ROIAlignV2, per stage the 2-FC box head
  and FastRCNNOutputLayers, [d2]'s _ScaleGradient(1 / 3) on the pooled features) on those rows at cosine >= 0.999 and norm within
  1 %, the criteria of tests/test_std_train_step.py. That covers the gradient scaling: the FPN laterals are among the masters, and
  the stages' own parameters are compared unscaled.
* One stage against the StandardRCNNTrainer step on the same batch and keys: bit-equal losses, torch.equal gradients of the head
  masters, the trunk's at the cosine / norm criteria (RoIAlign's scatter order is not deterministic).
* A few SGD iterations on a fixed batch lower the total loss; event_scalars carries the per-stage keys; with MODEL.MASK_ON and
  bitmask ground truth loss_mask is there and finite."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O
from tests.test_cascade_kernels import ref_refine
from tests.test_std_train_losses import _smooth_l1
from tests.test_std_train_step import q16

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N, H, W, GMAX = 2, 128, 160, 4
POST_TOPK = 1000
ONE_STAGE = ["MODEL.ROI_BOX_CASCADE_HEAD.IOUS", "(0.5,)", "MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS", "((10.0, 10.0, 5.0, 5.0),)"]


def _cfg(*opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cascade_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "SEED", "3", "MODEL.RPN.POST_NMS_TOPK_TRAIN", str(POST_TOPK)] + list(opts))
    return cfg


def _inputs():
    """The batch of tests/test_std_train_step.py: two images, three and two boxes, the two samplers' keys."""
    g = torch.Generator().manual_seed(23)
    images = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8)
    gt, gcls, gcnt = torch.zeros(N, GMAX, 4), torch.zeros(N, GMAX, dtype=torch.int64), [3, 2]
    for i, c in enumerate(gcnt):
        ctr = torch.rand(c, 2, generator=g) * torch.tensor([W * 0.7, H * 0.7]) + 16
        size = torch.rand(c, 2, generator=g) * 60 + 24
        b = torch.cat((ctr - size / 2, ctr + size / 2), dim=1)
        b[:, 0::2].clamp_(0, W)
        b[:, 1::2].clamp_(0, H)
        gt[i, :c] = b
        gcls[i, :c] = torch.randint(0, 80, (c,), generator=g)
    shapes = O.level_shapes(H, W)
    r = sum(x * y for x, y in shapes) * 3
    keys = dict(rpn_reg=torch.rand(N, r, generator=g).to(DEV), roi=torch.rand(N, POST_TOPK + GMAX, generator=g).to(DEV))
    hw = torch.tensor([(H, W)] * N, dtype=torch.int32).to(DEV)
    return images, gt, gcls, torch.tensor(gcnt, dtype=torch.int32), keys, hw, shapes


def _step(tr, inp):
    images, gt, gcls, gcnt, keys, hw, _ = inp
    with torch.no_grad():
        losses, saved = tr._forward(images.to(DEV), hw, H, W, gt.to(DEV), gcls.to(DEV), gcnt.to(DEV), keys)
        tr._backward(saved, N)
    torch.cuda.synchronize()
    return losses, saved


class _ScaleGradient(torch.autograd.Function):
    """[d2] detectron2.modeling.roi_heads.cascade_rcnn._ScaleGradient."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return x

    @staticmethod
    def backward(ctx, g):
        return g * ctx.scale, None


def _oracle_grads(params, images, shapes, s, cfg, stages, weights):
    """Autograd over the oracle's forward with fp16-rounded weights and stored activations where the HIP path stores fp16, on the HIP
    run's anchor labels and on every stage's rows (boxes, classes, matched boxes) as the HIP run produced them."""
    leaves = {k: v.clone().float().requires_grad_(True) for k, v in params.items()}
    pq = {k: (q16(v) if (v.dim() == 4 or k.endswith("fc1.weight") or k.endswith("fc2.weight")) and "objectness_logits" not in k
              and "anchor_deltas" not in k else v) for k, v in leaves.items()}
    batch, _ = O.preprocess_images(list(images))
    feats = O.resnet_fpn_forward(q16(batch), pq, quant=q16)
    ds, ls = [], []
    for k in ("p2", "p3", "p4", "p5", "p6"):
        d, l = O.standard_rpn_head(feats[k], pq)
        ds.append(d)
        ls.append(l)
    ds, ls = O.flatten_head_outputs(ds, ls)
    deltas, logits = torch.cat(ds, 1), torch.cat(ls, 1)
    anchors = torch.cat(O.anchor_grid(shapes, ratios=(0.5, 1.0, 2.0))).unsqueeze(0).expand(N, -1, -1)
    lab = s["labels"].long()
    pos, val = lab == 1, lab >= 0
    norm = cfg["rpn_batch_size"] * N
    losses = dict(loss_rpn_cls=F.binary_cross_entropy_with_logits(logits[val], lab[val].float(), reduction="sum") / norm * cfg["rpn_cls_weight"])
    tgt = O.b2b_get_deltas(anchors[pos], s["matched_boxes"][pos], (1.0, 1.0, 1.0, 1.0))
    losses["loss_rpn_loc"] = _smooth_l1(deltas[pos] - tgt, 0.0).sum() / norm * cfg["rpn_loc_weight"]
    k = cfg["std_num_classes"]
    for si in range(stages):
        st = s["stages"][si]
        boxes, bidx = st["boxes"], st["batch_idx"]
        valid = bidx >= 0
        lv = O.assign_levels(boxes)
        pooled = torch.zeros(boxes.shape[0], 256, 7, 7)
        for l, sc in enumerate((0.25, 0.125, 0.0625, 0.03125)):
            ids = torch.nonzero((lv == l) & valid).squeeze(1)
            if len(ids):
                rois = torch.cat((bidx[ids].float().unsqueeze(1), boxes[ids]), dim=1)
                pooled = pooled.index_put((ids,), O.roi_align_torch(feats[f"p{l + 2}"], rois, sc))
        x = _ScaleGradient.apply(q16(torch.flatten(pooled[valid], 1)), 1.0 / stages)
        bh, bp = f"roi_heads.box_head.{si}.", f"roi_heads.box_predictor.{si}."
        h1 = q16(F.relu(F.linear(x, pq[bh + "fc1.weight"], pq[bh + "fc1.bias"])))
        bf = F.relu(F.linear(h1, pq[bh + "fc2.weight"], pq[bh + "fc2.bias"]))
        cl = F.linear(bf, pq[bp + "cls_score.weight"], pq[bp + "cls_score.bias"])
        dl = F.linear(bf, pq[bp + "bbox_pred.weight"], pq[bp + "bbox_pred.bias"])
        cls = st["cls"][valid]
        losses[f"loss_cls_stage{si}"] = F.cross_entropy(cl, cls) * cfg["std_cls_loss_weight"]
        fg = torch.nonzero(cls < k).squeeze(1)
        t = O.b2b_get_deltas(boxes[valid][fg], st["gt_boxes"][valid][fg], weights[si])
        losses[f"loss_box_reg_stage{si}"] = _smooth_l1(dl[fg] - t, 0.0).sum() / max(len(cls), 1) * cfg["box_reg_weight"]
    sum(losses.values()).backward()
    return losses, {k_: v.grad for k_, v in leaves.items()}


def _reference_of(k, ref, a=3):
    """The autograd gradient of master `k` in the trainer's layout."""
    from openset_rcnn_amd.host.weights import pack_conv_weight, pack_fc1_weight
    rh = "proposal_generator.rpn_head"
    if k == "rpn_tail.w":
        return torch.cat((ref[rh + ".objectness_logits.weight"].view(a, 256), ref[rh + ".anchor_deltas.weight"].view(4 * a, 256)))
    if k == "rpn_tail.b":
        return torch.cat((ref[rh + ".objectness_logits.bias"], ref[rh + ".anchor_deltas.bias"]))
    head, _, rest = k.partition("_s")
    if rest and head in ("fc1", "fc2", "cls", "box"):
        s, kind = rest.split(".")
        long = {"fc1": f"roi_heads.box_head.{s}.fc1", "fc2": f"roi_heads.box_head.{s}.fc2", "cls": f"roi_heads.box_predictor.{s}.cls_score",
                "box": f"roi_heads.box_predictor.{s}.bbox_pred"}[head] + (".weight" if kind == "w" else ".bias")
        return pack_fc1_weight(ref[long], 256, 7, torch.float32) if (head, kind) == ("fc1", "w") else ref[long]
    if k.endswith(".w"):
        return pack_conv_weight(ref[k[:-2] + ".weight"], torch.float32)
    return ref[k[:-2] + ".bias"]


def _cos_ratio(got, want):
    return float(F.cosine_similarity(got.flatten(), want.flatten(), dim=0)), float(got.norm() / want.norm().clamp(min=1e-20))


def test_three_stage_step_rows_losses_and_every_gradient(osr):
    from openset_rcnn_amd.host.modeling import engine_cfg_from
    from openset_rcnn_amd.host.train_cascade import CascadeRCNNTrainer
    from openset_rcnn_amd.host.weights import random_cascade_params
    ecfg = engine_cfg_from(_cfg("MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", "128"))  # (the restatement pools every row of every stage in python loops)
    params = dict(random_cascade_params(0, stages=3))
    for s in range(3):  # smaller regression outputs: the boxes move a little from stage to stage, so rows stay foreground at 0.6 and 0.7
        params[f"roi_heads.box_predictor.{s}.bbox_pred.weight"] = params[f"roi_heads.box_predictor.{s}.bbox_pred.weight"] * 0.1
    tr = CascadeRCNNTrainer(params, ecfg, dtype=torch.float16, device=DEV, loss_scale=512.0)
    e = tr.eng
    assert e.num_stages == 3 and e.stage_ious == (0.5, 0.6, 0.7)
    # the masters, in reverse order of gradient completion: ..., the RPN tail, then stage 0 .. 2, inside a stage fc1, fc2, box, cls
    names = [k for k in tr.master if k.split("_s")[0] in ("fc1", "fc2", "box", "cls")]
    assert names == [f"{h}_s{s}.{p}" for s in range(3) for h in ("fc1", "fc2", "box", "cls") for p in ("w", "b")]
    assert list(tr.master)[-len(names):] == names and list(tr.master)[-len(names) - 1] == "rpn_tail.b"
    inp = _inputs()
    images, gt, gcls, gcnt, keys, hw, shapes = inp
    losses, saved = _step(tr, inp)
    assert sorted(losses) == sorted(["loss_rpn_cls", "loss_rpn_loc"] + [f"loss_{n}_stage{s}" for s in range(3) for n in ("cls", "box_reg")])
    stages = [{k: v.detach().cpu() for k, v in st.items() if k in ("boxes", "batch_idx", "cls", "gt_boxes", "logits", "deltas")} for st in saved["stages"]]
    # ---- the rows of the later stages: the restatement on the HIP run's own boxes and deltas ----
    for s in (1, 2):
        prev, cur = stages[s - 1], stages[s]
        want = ref_refine(prev["boxes"], prev["batch_idx"], prev["deltas"], N, [(H, W)] * N, e.stage_weights[s - 1], True, gt, gcls, gcnt, 80, e.stage_ious[s])
        assert torch.equal(cur["batch_idx"], want["batch_idx"]) and torch.equal(cur["cls"], want["gt_classes"])
        err = float((cur["boxes"] - want["boxes"]).abs().max())
        print(f"[stage {s} rows] {int((cur['batch_idx'] >= 0).sum())} rows, {int(((cur['cls'] >= 0) & (cur['cls'] < 80)).sum())} foreground; "
              f"max |box - ref| = {err:.3e} (bound 1e-4)")
        assert err <= 1e-4 and torch.equal(cur["gt_boxes"], want["gt_boxes"])
        assert int(((cur["cls"] >= 0) & (cur["cls"] < 80)).sum()) > 0
    # ---- the six stage losses on the HIP run's logits, deltas and rows ----
    c = e.cfg
    for s, st in enumerate(stages):
        valid = st["cls"] >= 0
        cls = st["cls"][valid]
        l_cls = F.cross_entropy(st["logits"][valid].double(), cls) * c["std_cls_loss_weight"]
        fg = torch.nonzero(cls < 80).squeeze(1)
        t = O.b2b_get_deltas(st["boxes"][valid][fg].double(), st["gt_boxes"][valid][fg].double(), e.stage_weights[s])
        l_box = (st["deltas"][valid][fg].double() - t).abs().sum() / max(len(cls), 1) * c["box_reg_weight"]
        for name, want in ((f"loss_cls_stage{s}", l_cls), (f"loss_box_reg_stage{s}", l_box)):
            rel = abs(float(losses[name]) - float(want)) / abs(float(want))
            print(f"[{name}] {float(losses[name]):.6f} against {float(want):.6f}: relative error {rel:.2e} (bound 1e-4)")
            assert rel <= 1e-4, name
    # ---- every master's gradient against autograd over the restatement ----
    s = dict(labels=saved["labels"].cpu(), matched_boxes=saved["matched_boxes"].cpu(), stages=stages)
    ref_losses, ref = _oracle_grads(params, images, shapes, s, c, 3, e.stage_weights)
    for k, v in ref_losses.items():
        assert float(losses[k]) == pytest.approx(float(v.detach()), rel=3e-2, abs=1e-4), k
    report, bad = [], []
    for k, gten in tr.grad.items():
        got, want = gten.detach().cpu() / tr.loss_scale, _reference_of(k, ref)
        assert got.shape == want.shape, k
        cos, ratio = _cos_ratio(got, want)
        report.append(f"{k:48s} cos {cos:.4f}  |got|/|ref| {ratio:.3f}  |ref| {float(want.norm()):.3e}")
        if not (cos >= 0.999 and 0.99 <= ratio <= 1.01):
            bad.append(report[-1])
    print("\n".join(report))
    assert len(report) == len(tr.master) and any(k.startswith("backbone.fpn_lateral") for k in tr.grad)
    assert not bad, "gradient mismatch:\n" + "\n".join(bad)
    # ---- export: detectron2's names, every stage ----
    sd = tr.export_state_dict()
    for k, v in params.items():
        if k.startswith("roi_heads."):
            assert k in sd and torch.allclose(sd[k], v.float()), k
    # ---- the per-stage scalars ----
    ev = tr.event_scalars()
    for k in ["roi_head/num_fg_samples", "roi_head/num_bg_samples"] + [f"stage{s}/roi_head/num_{x}_samples" for s in (1, 2) for x in ("fg", "bg")] + \
            [f"stage{s}/fast_rcnn/{x}" for s in range(3) for x in ("cls_accuracy", "fg_cls_accuracy", "false_negative")]:
        assert k in ev, (k, sorted(ev))
    assert "stage0/roi_head/num_fg_samples" not in ev
    for st_i, cur in enumerate(stages[1:], 1):
        fgn = int(((cur["cls"] >= 0) & (cur["cls"] < 80)).sum())
        assert ev[f"stage{st_i}/roi_head/num_fg_samples"] == pytest.approx(fgn / N)


def test_one_stage_step_equals_the_stock_trainer(osr):
    from openset_rcnn_amd.host.modeling import engine_cfg_from
    from openset_rcnn_amd.host.train_cascade import CascadeRCNNTrainer
    from openset_rcnn_amd.host.train_std import StandardRCNNTrainer
    from openset_rcnn_amd.host.weights import random_cascade_params, random_standard_params
    ecfg = engine_cfg_from(_cfg(*ONE_STAGE))
    assert ecfg["cls_agnostic_bbox_reg"] and tuple(ecfg["bbox_reg_weights"]) == (10.0, 10.0, 5.0, 5.0)
    std = StandardRCNNTrainer(random_standard_params(0), ecfg, dtype=torch.float16, device=DEV, loss_scale=512.0)
    cas = CascadeRCNNTrainer(random_cascade_params(0, stages=1), ecfg, dtype=torch.float16, device=DEV, loss_scale=512.0)
    inp = _inputs()
    la, _ = _step(std, inp)
    lb, _ = _step(cas, inp)
    for a, b in (("loss_rpn_cls", "loss_rpn_cls"), ("loss_rpn_loc", "loss_rpn_loc"), ("loss_cls", "loss_cls_stage0"), ("loss_box_reg", "loss_box_reg_stage0")):
        assert torch.equal(la[a], lb[b]), (a, float(la[a]), float(lb[b]))
    assert len(std.grad) == len(cas.grad)
    bad = []
    for k, g in std.grad.items():
        head, _, p = k.partition(".")
        if head in ("fc1", "fc2", "box", "cls"):
            assert torch.equal(g, cas.grad[f"{head}_s0.{p}"]), k  # the head masters: the same launches on the same operands
            continue
        cos, ratio = _cos_ratio(cas.grad[k].float().cpu(), g.float().cpu())
        if not (cos >= 0.999 and 0.99 <= ratio <= 1.01):
            bad.append(f"{k}: cos {cos:.5f} ratio {ratio:.4f}")
    assert not bad, bad


def _model(cfg, params):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(cfg)
    sd = model.state_dict()
    for k, v in params.items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)
    return model


def test_sgd_iterations_lower_the_loss(osr):
    from openset_rcnn_amd.host.structures import Boxes, Instances
    from openset_rcnn_amd.host.train_cascade import CascadeRCNNTrainer
    from openset_rcnn_amd.host.weights import random_cascade_params
    model = _model(_cfg("MODEL.RPN.POST_NMS_TOPK_TRAIN", "2000"), random_cascade_params(1, stages=3))  # (the shipped file's value)
    g = torch.Generator().manual_seed(2)
    batch = []
    for i in range(2):
        img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
        b = torch.tensor([[10.0, 12.0, 70.0, 90.0], [60.0, 30.0, 150.0, 110.0]]) + 4 * i
        batch.append({"image": img, "instances": Instances((H, W), gt_boxes=Boxes(b), gt_classes=torch.tensor([3, 17 + i]))})
    model.train()
    tr = model.trainer()
    assert type(tr) is CascadeRCNNTrainer
    tr.lr = 2e-4  # (as tests/test_std_train_step.py: the synthetic weights start far from a minimum)
    tr.scaler.growth_interval = 0
    totals = []
    for _ in range(8):
        out = tr.step(*model._train_tensors(batch, torch.Generator().manual_seed(0)))  # the same batch and the same samples every time
        totals.append(float(sum(out.values())))
    tr.poll_overflow(wait=True)
    assert tr.overflow_steps == 0 and len(out) == 8
    assert totals[-1] < totals[0], totals
    # the backward's derived copies of every stage follow the updated weights (stage 0's are repacked on the trainer's second stream)
    torch.cuda.synchronize()
    e = tr.eng
    for s in range(3):
        assert torch.equal(tr.t_cls_s[s][:, :81], e.cls_ws[s].t()) and torch.equal(tr.t_box_s[s][:, :4], e.box_ws[s].t())
        assert torch.equal(tr.wd[f"fc2_s{s}"].view(1024, 1024), e.fc2_ws[s].t())
        assert torch.equal(e.fc2_ws[s], tr.master[f"fc2_s{s}.w"].to(e.fc2_ws[s].dtype))
    # the trained masters go back into the module under detectron2's names
    model.eval()
    sd = model.state_dict()
    assert torch.equal(sd["roi_heads.box_predictor.2.cls_score.weight"].cpu(), tr.master["cls_s2.w"].cpu())


def test_mask_on_trains_with_bitmasks(osr):
    from openset_rcnn_amd.host.weights import random_cascade_params
    from tests.test_mask_train_step import _batch
    params = dict(random_cascade_params(0, stages=3, num_classes=5))
    g = torch.Generator().manual_seed(4100)
    pre = "roi_heads.mask_head."
    params[pre + "mask_fcn1.weight"] = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / (256 * 9)) ** 0.5
    params[pre + "mask_fcn1.bias"] = torch.randn(256, generator=g) * 0.02
    params[pre + "deconv.weight"] = torch.randn(256, 256, 2, 2, generator=g) * (2.0 / 256) ** 0.5
    params[pre + "deconv.bias"] = torch.randn(256, generator=g) * 0.02
    params[pre + "predictor.weight"] = torch.randn(1, 256, 1, 1, generator=g) * 0.05
    params[pre + "predictor.bias"] = torch.randn(1, generator=g) * 0.1
    model = _model(_cfg("MODEL.MASK_ON", "True", "INPUT.MASK_FORMAT", "bitmask", "MODEL.ROI_HEADS.NUM_CLASSES", "5", "MODEL.ROI_MASK_HEAD.NUM_CONV", "1"), params)
    model.train()
    tr = model.trainer()
    before = tr.master["mask_pred.w"].clone()
    out = model.train_step(tr, _batch(), torch.Generator().manual_seed(0))
    tr.poll_overflow(wait=True)
    assert sorted(out) == sorted(["loss_rpn_cls", "loss_rpn_loc", "loss_mask"] + [f"loss_{n}_stage{s}" for s in range(3) for n in ("cls", "box_reg")])
    assert all(bool(torch.isfinite(v)) for v in out.values()) and float(out["loss_mask"]) > 0
    assert tr.overflow_steps == 0 and not torch.equal(before, tr.master["mask_pred.w"])
    assert "mask_rcnn/accuracy" in tr.event_scalars()
