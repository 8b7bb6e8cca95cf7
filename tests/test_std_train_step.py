"""A whole StandardRCNNTrainer step (Base-RCNN-FPN.yaml's stock heads) at n = 2, 128 x 160: the gradient of EVERY master against torch
autograd over the oracle's forward (ResNet-50 + FPN, StandardRPNHead, ROIAlignV2, box head, FastRCNNOutputLayers) on the anchors and
proposals the HIP run sampled, class-agnostic and class-specific (cosine >= 0.999, norm within 1 %: the test_train_step.py criteria);
a few SGD iterations on a fixed batch lower the total loss and keep the derived copies current; a sparse list that does not fit its cap
poisons (skips) the update."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O
from tests.test_std_train_losses import _smooth_l1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _base_cfg():
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "SEED", "3"])
    return cfg


def _model_and_batch(seed=0):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.structures import Boxes, Instances
    from openset_rcnn_amd.host.weights import random_standard_params
    cfg = _base_cfg()
    model = M.build_model(cfg)
    sd = model.state_dict()
    for k, v in random_standard_params(seed).items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(seed + 1)
    batch = []
    for i in range(2):
        img = torch.randint(0, 256, (3, 128, 160), generator=g, dtype=torch.uint8)
        b = torch.tensor([[10.0, 12.0, 70.0, 90.0], [60.0, 30.0, 150.0, 110.0]]) + 4 * i
        batch.append({"image": img, "instances": Instances((128, 160), gt_boxes=Boxes(b), gt_classes=torch.tensor([3, 17 + i]))})
    return model, batch


def q16(t):
    return t.half().float()


def _oracle_grads(params, images, shapes, s, cfg, n, a):
    """Autograd over the oracle's forward ([d2] ResNet-50 + FPN, StandardRPNHead, ROIAlignV2, the 2-FC box head, FastRCNNOutputLayers)
    with fp16-rounded weights and stored activations where the HIP path stores fp16, on the HIP run's anchor labels, matched boxes and
    sampled proposals."""
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
    deltas, logits = torch.cat(ds, 1), torch.cat(ls, 1)  # (n, R, 4), (n, R): image-major, (level, y, x, a)
    anchors = torch.cat(O.anchor_grid(shapes, ratios=(0.5, 1.0, 2.0))).unsqueeze(0).expand(n, -1, -1)
    lab = s["labels"].long()
    pos, val = lab == 1, lab >= 0
    norm = cfg["rpn_batch_size"] * n
    l_rpn_cls = F.binary_cross_entropy_with_logits(logits[val], lab[val].float(), reduction="sum") / norm * cfg["rpn_cls_weight"]
    tgt = O.b2b_get_deltas(anchors[pos], s["matched_boxes"][pos], (1.0, 1.0, 1.0, 1.0))
    l_rpn_loc = _smooth_l1(deltas[pos] - tgt, 0.0).sum() / norm * cfg["rpn_loc_weight"]
    # RoI heads on the engine's sampled rows
    boxes, bidx = s["boxes"], s["batch_idx"]
    valid = bidx >= 0
    lv = O.assign_levels(boxes)
    pooled = torch.zeros(boxes.shape[0], 256, 7, 7)
    for l, sc in enumerate((0.25, 0.125, 0.0625, 0.03125)):
        ids = torch.nonzero((lv == l) & valid).squeeze(1)
        if len(ids):
            rois = torch.cat((bidx[ids].float().unsqueeze(1), boxes[ids]), dim=1)
            pooled = pooled.index_put((ids,), O.roi_align_torch(feats[f"p{l + 2}"], rois, sc))
    x = q16(torch.flatten(pooled[valid], 1))
    h1 = q16(F.relu(F.linear(x, pq["roi_heads.box_head.fc1.weight"], pq["roi_heads.box_head.fc1.bias"])))
    bf = F.relu(F.linear(h1, pq["roi_heads.box_head.fc2.weight"], pq["roi_heads.box_head.fc2.bias"]))
    cl = F.linear(bf, pq["roi_heads.box_predictor.cls_score.weight"], pq["roi_heads.box_predictor.cls_score.bias"])
    dl = F.linear(bf, pq["roi_heads.box_predictor.bbox_pred.weight"], pq["roi_heads.box_predictor.bbox_pred.bias"])
    cls = s["cls"][valid]
    k = cfg["std_num_classes"]
    l_cls = F.cross_entropy(cl, cls) * cfg["std_cls_loss_weight"]
    fg = torch.nonzero(cls < k).squeeze(1)
    sel = dl[fg] if dl.shape[1] == 4 else dl.view(-1, k, 4)[fg, cls[fg]]
    t = O.b2b_get_deltas(boxes[valid][fg], s["gt_boxes"][valid][fg], cfg["bbox_reg_weights"])
    l_box = _smooth_l1(sel - t, 0.0).sum() / max(len(cls), 1) * cfg["box_reg_weight"]
    losses = dict(loss_rpn_cls=l_rpn_cls, loss_rpn_loc=l_rpn_loc, loss_cls=l_cls, loss_box_reg=l_box)
    sum(losses.values()).backward()
    return losses, {k_: v.grad for k_, v in leaves.items()}


def _reference_of(k, ref, a):
    """The autograd gradient of master `k` in the trainer's layout."""
    from openset_rcnn_amd.host.weights import pack_conv_weight, pack_fc1_weight
    rh, bp = "proposal_generator.rpn_head", "roi_heads.box_predictor"
    if k == "rpn_tail.w":
        return torch.cat((ref[rh + ".objectness_logits.weight"].view(a, 256), ref[rh + ".anchor_deltas.weight"].view(4 * a, 256)))
    if k == "rpn_tail.b":
        return torch.cat((ref[rh + ".objectness_logits.bias"], ref[rh + ".anchor_deltas.bias"]))
    heads = {"fc1.b": "roi_heads.box_head.fc1.bias", "fc2.w": "roi_heads.box_head.fc2.weight", "fc2.b": "roi_heads.box_head.fc2.bias",
             "cls.w": bp + ".cls_score.weight", "cls.b": bp + ".cls_score.bias", "box.w": bp + ".bbox_pred.weight", "box.b": bp + ".bbox_pred.bias"}
    if k == "fc1.w":
        return pack_fc1_weight(ref["roi_heads.box_head.fc1.weight"], 256, 7, torch.float32)
    if k in heads:
        return ref[heads[k]]
    if k.endswith(".w"):
        return pack_conv_weight(ref[k[:-2] + ".weight"], torch.float32)
    return ref[k[:-2] + ".bias"]


@pytest.mark.gpu
@pytest.mark.parametrize("agnostic", [True, False], ids=["agnostic", "class-specific"])
def test_std_train_step_gradients_of_every_master_match_autograd(osr, agnostic):
    """Every master of a whole StandardRCNNTrainer step (backbone res3..res5, FPN, RPN head, box head, both output layers)
    against autograd over the oracle's forward on the same samples: cosine >= 0.999 and norm within 1 % per tensor."""
    from openset_rcnn_amd.host.modeling import engine_cfg_from
    from openset_rcnn_amd.host.train_std import StandardRCNNTrainer
    from openset_rcnn_amd.host.weights import random_standard_params
    cfg = _base_cfg()
    ecfg = engine_cfg_from(cfg)
    ecfg["cls_agnostic_bbox_reg"] = agnostic
    params = random_standard_params(0, cls_agnostic=agnostic)
    tr = StandardRCNNTrainer(params, ecfg, dtype=torch.float16, device=DEV, loss_scale=512.0)
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
        gcls[i, :c] = torch.randint(0, 80, (c,), generator=g)
    shapes = O.level_shapes(h, w)
    a = 3
    r = sum(x * y for x, y in shapes) * a
    keys = dict(rpn_reg=torch.rand(n, r, generator=g).to(DEV), roi=torch.rand(n, ecfg["post_nms_topk_train"] + gmax, generator=g).to(DEV))
    hw = torch.tensor([(h, w)] * n, dtype=torch.int32).to(DEV)
    with torch.no_grad():
        losses, saved = tr._forward(images.to(DEV), hw, h, w, gt.to(DEV), gcls.to(DEV), torch.tensor(gcnt, dtype=torch.int32).to(DEV), keys)
        tr._backward(saved, n)
    torch.cuda.synchronize()
    s = dict(labels=saved["labels"].cpu(), matched_boxes=saved["matched_boxes"].cpu(), boxes=saved["boxes"].cpu(),
             batch_idx=saved["smp"]["batch_idx"].cpu(), cls=saved["cls"].cpu(), gt_boxes=saved["smp"]["gt_boxes"].view(-1, 4).cpu())
    assert int((s["labels"] == 1).sum()) > 0 and int(((s["cls"] >= 0) & (s["cls"] < 80)).sum()) > 0
    ref_losses, ref = _oracle_grads(params, images, shapes, s, tr.eng.cfg, n, a)
    for k, v in ref_losses.items():
        assert float(losses[k]) == pytest.approx(float(v.detach()), rel=3e-2, abs=1e-4), k
    S = tr.loss_scale
    report, bad = [], []
    for k, gten in tr.grad.items():
        got, want = gten.detach().cpu() / S, _reference_of(k, ref, a)
        assert got.shape == want.shape, k
        cos = float(F.cosine_similarity(got.flatten(), want.flatten(), dim=0))
        ratio = float(got.norm() / want.norm().clamp(min=1e-20))
        report.append(f"{k:48s} cos {cos:.4f}  |got|/|ref| {ratio:.3f}  |ref| {float(want.norm()):.3e}")
        if not (cos >= 0.999 and 0.99 <= ratio <= 1.01):
            bad.append(report[-1])
    print("\n".join(report))
    assert len(report) == len(tr.master) and any(k.startswith("backbone.bottom_up.res3") for k in tr.grad)
    assert not bad, "gradient mismatch:\n" + "\n".join(bad)


@pytest.mark.gpu
def test_std_sgd_iterations_lower_the_loss_and_an_overflowing_list_skips_the_update(osr):
    model, batch = _model_and_batch(1)
    model.train()
    tr = model.trainer()
    tr.lr = 2e-4  # (the synthetic weights start far from a minimum: larger steps diverge within a few iterations)
    tr.scaler.growth_interval = 0
    totals = []
    for _ in range(8):
        tensors = model._train_tensors(batch, torch.Generator().manual_seed(0))  # the same batch and the same samples every time
        out = tr.step(*tensors)
        totals.append(float(sum(out.values())))
    tr.poll_overflow(wait=True)
    assert tr.overflow_steps == 0
    assert totals[-1] < totals[0], totals
    # the backward's derived copies follow the updated weights (refreshed after every update)
    e = tr.eng
    assert torch.equal(tr.t_cls[:, : e.cls_w.shape[0]], e.cls_w.t()) and torch.equal(tr.t_box[:, : e.box_w.shape[0]], e.box_w.t())
    assert torch.equal(tr.w3_t, e.w["proposal_generator.rpn_head.conv.w"].view(256, -1).t())
    # a list that does not fit the cap: the update is skipped (parameters unchanged), counted as an overflow step
    before = {k: v.detach().clone() for k, v in tr.master.items()}
    tr.sparse_rows_cap = 1
    tr.step(*model._train_tensors(batch, torch.Generator().manual_seed(0)))
    tr.poll_overflow(wait=True)
    assert tr.overflow_steps == 1
    assert all(torch.equal(before[k], v) for k, v in tr.master.items())
