"""Whole training step on the GPU (host/train.py): gradients of every trainable parameter against torch autograd over the oracle's
forward, evaluated on the SAME sampled anchors / proposals (taken from the HIP run, so that fp16 noise cannot change the sampled
sets), and a few SGD iterations on a fixed batch.

Tolerance: the HIP path stores activations and activation gradients in fp16 (loss-scaled) and runs ~50 layers deep; the oracle is
fp32 with fp16-rounded weights and activations. Per parameter tensor: cosine similarity >= 0.999 and norm within 1 % (measured:
>= 0.9997 and within 0.4 %)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def q16(t):
    return t.half().float()


@pytest.fixture(scope="module")
def setup(osr):
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    from openset_rcnn_amd.host.weights import random_params
    params = random_params(0)
    tr = OpensetRCNNTrainer(params, dtype=torch.float16, device=DEV, lr=0.002, loss_scale=512.0)
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
    return dict(tr=tr, params=params, images=images, shapes=shapes, n=n, h=h, w=w, dev=dev)


def _oracle_grads(params, images, shapes, s, cfg, n):
    leaves = {k: v.clone().float().requires_grad_(True) for k, v in params.items()}
    pq = {k: (q16(v) if (v.dim() == 4 or k.endswith("fc1.weight") or k.endswith("fc2.weight")) and "anchor_deltas" not in k and "centerness" not in k else v)
          for k, v in leaves.items()}
    batch, _ = O.preprocess_images(list(images))
    feats = O.resnet_fpn_forward(q16(batch), pq, quant=q16)
    ds, cs = [], []
    for k in ("p2", "p3", "p4", "p5", "p6"):
        d, c = O.cfrpn_head(feats[k], pq)
        ds.append(d)
        cs.append(c)
    ds, cs = O.flatten_head_outputs(ds, cs)
    anchors = torch.cat(O.anchor_grid(shapes))
    rl = O.rpn_losses(anchors, torch.cat(ds, 1), torch.cat(cs, 1), s["labels"], s["obj_labels"], s["matched_boxes"], s["ctr_target"],
                      cfg["rpn_batch_size"], cfg["rpn_loc_weight"], cfg["rpn_ctr_weight"])
    # RoI heads on the engine's sampled rows
    boxes, bidx = s["boxes"], s["batch_idx"]
    valid = bidx >= 0
    lv = O.assign_levels(boxes)
    m = boxes.shape[0]
    pooled = torch.zeros(m, 256, 7, 7)
    for l, sc in enumerate((0.25, 0.125, 0.0625, 0.03125)):
        ids = torch.nonzero((lv == l) & valid).squeeze(1)
        if len(ids):
            rois = torch.cat((bidx[ids].float().unsqueeze(1), boxes[ids]), dim=1)
            pooled = pooled.index_put((ids,), O.roi_align_torch(feats[f"p{l + 2}"], rois, sc))
    x = q16(torch.flatten(pooled[valid], 1))
    h1 = q16(F.relu(F.linear(x, pq["roi_heads.box_head.fc1.weight"], pq["roi_heads.box_head.fc1.bias"])))
    bf = F.relu(F.linear(h1, pq["roi_heads.box_head.fc2.weight"], pq["roi_heads.box_head.fc2.bias"]))
    d, iou = O.box_predictor(bf, pq)
    cls, ious = s["cls"][valid], s["ious"][valid]
    lb, li = O.roi_box_losses(d, iou.view(-1), boxes[valid], s["gt_boxes"][valid], cls, ious, cfg["num_classes"], cfg["box_reg_weight"], cfg["iou_reg_weight"])
    _, rec, ldml = O.pln_loss(bf, cls, ious, pq, cfg["pln_alpha"], cfg["pln_beta"], cfg["pln_loss_weight"], cfg["num_known"], cfg["pln_iou_threshold"])
    logits = F.linear(rec, pq["roi_heads.softmaxcls.cls_score.weight"], pq["roi_heads.softmaxcls.cls_score.bias"])
    lce = O.softmax_ce_loss(logits, cls, cfg["num_classes"], cfg["num_known"], cfg["cls_loss_weight"])
    losses = dict(loss_rpn_loc=rl["loss_rpn_loc"], loss_rpn_ctr=rl["loss_rpn_ctr"], loss_box_reg=lb, loss_iou=li, loss_dml=ldml, loss_cls=lce)
    sum(losses.values()).backward()
    return losses, {k: v.grad for k, v in leaves.items()}


def test_gradients_match_autograd_on_the_same_samples(setup):
    from openset_rcnn_amd.host.weights import pack_conv_weight, pack_fc1_weight
    tr, d, n = setup["tr"], setup["dev"], setup["n"]
    losses, saved = tr._forward(d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    tr._backward(saved, n)
    torch.cuda.synchronize()
    s = dict(labels=saved["labels"].cpu(), obj_labels=saved["obj_labels"].cpu(), matched_boxes=saved["matched_boxes"].cpu(),
             ctr_target=saved["ctr_target"].cpu(), boxes=saved["boxes"].cpu(), batch_idx=saved["smp"]["batch_idx"].cpu(), cls=saved["cls"].cpu(),
             ious=saved["ious"].cpu(), gt_boxes=saved["smp"]["gt_boxes"].view(-1, 4).cpu())
    assert int((s["labels"] == 1).sum()) > 0 and int(((s["cls"] >= 0) & (s["cls"] < 20)).sum()) > 0
    ref_losses, ref = _oracle_grads(setup["params"], setup["images"], setup["shapes"], s, tr.eng.cfg, n)
    for k, v in ref_losses.items():
        assert float(losses[k]) == pytest.approx(float(v), rel=3e-2, abs=1e-4), k
    S = tr.loss_scale
    names = {"rpn_tail.w": None, "fc1.w": "roi_heads.box_head.fc1.weight", "fc1.b": "roi_heads.box_head.fc1.bias",
             "fc2.w": "roi_heads.box_head.fc2.weight", "fc2.b": "roi_heads.box_head.fc2.bias", "enc.w": "roi_heads.dml.encoder.weight",
             "enc.b": "roi_heads.dml.encoder.bias", "dec.w": "roi_heads.dml.decoder.weight", "dec.b": "roi_heads.dml.decoder.bias",
             "cls.w": "roi_heads.softmaxcls.cls_score.weight", "cls.b": "roi_heads.softmaxcls.cls_score.bias", "protos": "roi_heads.dml.representatives"}
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
            want = pack_fc1_weight(ref[names[k]], 256, 7, torch.float32)
        elif k in names:
            want = ref[names[k]]
        elif k.endswith(".w"):
            want = pack_conv_weight(ref[k[:-2] + ".weight"], torch.float32)
        else:
            want = ref[k[:-2] + ".bias"]
        assert got.shape == want.shape, k
        cos = float(F.cosine_similarity(got.flatten(), want.flatten(), dim=0))
        ratio = float(got.norm() / want.norm().clamp(min=1e-20))
        report.append(f"{k:48s} cos {cos:.4f}  |got|/|ref| {ratio:.3f}  |ref| {float(want.norm()):.3e}")
        if not (cos >= 0.999 and 0.99 <= ratio <= 1.01):  # measured: cos >= 0.9997, norms within 0.4 %
            bad.append(report[-1])
    print("\n".join(report))
    assert not bad, "gradient mismatch:\n" + "\n".join(bad)


def test_sgd_steps_reduce_the_loss_and_are_reproducible(setup, osr):
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]

    def run():
        # random-init weights give gradient norms in the hundreds: a small step keeps the fixed-batch descent monotone enough
        tr = OpensetRCNNTrainer(setup["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0)
        hist = []
        for _ in range(6):
            losses = tr.step(d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
            hist.append(sum(float(v) for v in losses.values()))
        return hist, tr

    h1, tr = run()
    assert all(torch.isfinite(torch.tensor(h1))), h1
    assert h1[-1] < 0.9 * h1[0], f"total loss did not decrease on a fixed batch: {h1}"
    h2, _ = run()
    # the forward is bitwise deterministic; in the backward only RoIAlign's atomic scatter is not order-deterministic, and its
    # fp32 round-off differences grow over the following updates
    assert h2[0] == h1[0]
    assert h2[:3] == pytest.approx(h1[:3], rel=2e-2), (h1, h2)
    assert h2 == pytest.approx(h1, rel=6e-2), (h1, h2)  # (six updates on random-init weights amplify the round-off noise of the first)
    assert tr.num_params == 41_621_279  # trainable parameters with FREEZE_AT = 2


def test_bf16_training_step(setup):
    """The same step with bf16 activations / gradients and no loss scaling (bf16 has fp32's exponent range)."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]
    tr = OpensetRCNNTrainer(setup["params"], dtype=torch.bfloat16, device=DEV, lr=5e-5, loss_scale=1.0)
    hist = []
    for _ in range(5):
        losses = tr.step(d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
        hist.append(sum(float(v) for v in losses.values()))
    assert all(torch.isfinite(torch.tensor(hist))), hist
    assert hist[-1] < 0.9 * hist[0], hist


def test_training_step_with_the_other_reference_losses(setup):
    """The whole step with the losses the yaml files do not select (MODEL.RPN.BBOX_REG_LOSS_TYPE "giou" + CTR_SMOOTH_L1_BETA 0.1,
    MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE "diou" + IOU_SMOOTH_L1_BETA 0.05; box_regression_w_iou.py:62-82): they reach the kernels
    through the trainer's cfg, the six losses are finite, differ from the default's where they should, and SGD reduces their sum."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]
    args = (d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    base = OpensetRCNNTrainer(setup["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0)
    l0 = {k: float(v) for k, v in base.step(*args, update=False).items()}
    cfg = dict(loss_types=dict(rpn_box=("giou", 0.0), rpn_ctr=("smooth_l1", 0.1), roi_box=("diou", 0.0), roi_iou=("smooth_l1", 0.05)))
    tr = OpensetRCNNTrainer(setup["params"], cfg=cfg, dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0)
    hist = []
    for i in range(5):
        losses = tr.step(*args)
        if i == 0:
            l1 = {k: float(v) for k, v in losses.items()}
        hist.append(sum(float(v) for v in losses.values()))
    assert all(torch.isfinite(torch.tensor(hist))), hist
    assert l1["loss_cls"] == pytest.approx(l0["loss_cls"], rel=1e-6) and l1["loss_dml"] == pytest.approx(l0["loss_dml"], rel=1e-6)
    assert l1["loss_rpn_loc"] > l0["loss_rpn_loc"]              # GIoU loss >= IoU loss pair by pair
    assert l1["loss_rpn_ctr"] < l0["loss_rpn_ctr"]              # smooth L1 with beta > 0 <= L1
    assert l1["loss_iou"] < l0["loss_iou"] and l1["loss_box_reg"] != pytest.approx(l0["loss_box_reg"], rel=1e-3)
    assert hist[-1] < 0.95 * hist[0], hist


def test_training_step_with_l2_distance_and_two_prototypes_per_class(setup):
    """MODEL.PLN.DISTANCE_TYPE 'L2' with REPS_PER_CLASS 2 through the whole step (prototype_learning_network.py:155-180): the
    (40, 256) prototype parameter trains, losses stay finite and fall."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]
    args = (d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    params = dict(setup["params"])
    rep = params["roi_heads.dml.representatives"]
    params["roi_heads.dml.representatives"] = torch.cat((rep, rep + 0.3 * torch.randn(rep.shape, generator=torch.Generator().manual_seed(5))), 1).reshape(-1, rep.shape[1])
    tr = OpensetRCNNTrainer(params, cfg=dict(reps_per_class=2, pln_distance="L2", pln_alpha=0.6, pln_beta=1.2), dtype=torch.float16, device=DEV, lr=5e-5,
                            loss_scale=512.0)
    assert tuple(tr.master["protos"].shape) == (2 * rep.shape[0], rep.shape[1])
    before = tr.master["protos"].clone()
    hist = []
    for _ in range(4):
        losses = tr.step(*args)
        hist.append({k: float(v) for k, v in losses.items()})
    tot = [sum(h.values()) for h in hist]
    assert all(torch.isfinite(torch.tensor(tot))), tot
    assert hist[0]["loss_dml"] > 0 and tot[-1] < tot[0]
    assert not torch.equal(tr.master["protos"], before)
    out = tr.export_state_dict()["roi_heads.dml.representatives"]
    assert tuple(out.shape) == (2 * rep.shape[0], rep.shape[1])


def test_weight_gradients_on_the_second_stream_are_the_same_gradients(setup):
    """The trainer runs the weight / bias gradient launches on a second stream beside the chain of data gradients (train._wg).
    Same batch, same weights, with and without it: every parameter whose gradient does not pass through RoIAlign's atomic scatter
    is bit-identical, the rest agree to the scatter's fp32 summation order; three iterations in a row reuse the buffers."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]
    args = (d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    grads = {}
    for side in (True, False):
        tr = OpensetRCNNTrainer(setup["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0)
        tr.side_wgrad = side
        for _ in range(3):
            tr.grad_flat.fill_(float("nan"))
            tr.step(*args, update=False)
        torch.cuda.synchronize()
        grads[side] = {k: v.clone() for k, v in tr.grad.items()}
    exact = ("fc1.w", "fc1.b", "fc2.w", "fc2.b", "pred.w", "enc.w", "dec.w", "cls.w", "protos", "rpn_tail.w", "proposal_generator.rpn_head.conv.w")
    for k, a in grads[True].items():
        b = grads[False][k]
        assert bool(torch.isfinite(a).all()), k
        if k in exact:
            assert torch.equal(a, b), k
        else:
            assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max()) + 1e-6, k


def test_multi_tensor_update_is_bit_identical_to_one_launch_per_tensor(setup):
    """The trainer's update as two launches (osr_sgd_step_multi_ex over its segment table, osr_pack_dgrad_weight_multi over its pack
    table) against ~145 launches built here -- ops.sgd_step_ per master (a one-entry plan each) and ops.pack_dgrad_weight per tensor --
    from the SAME gradients, masters and momentum: two updates in a row -- masters, momentum buffers, the low-precision working copies
    and the backward-data weights agree bit for bit, which holds the big tables' pointers, row ranges and chunk lists to the trivially
    built ones; an overflowed iteration (flag 0) changes nothing in either form."""
    from openset_rcnn_amd.host import ops
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]
    args = (d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    tr = OpensetRCNNTrainer(setup["params"], dtype=torch.float16, device=DEV, lr=0.01, loss_scale=512.0)
    tr.step(*args, update=False)  # gradients of a real step
    torch.cuda.synchronize()
    snap = dict(master={k: v.clone() for k, v in tr.master.items()}, mom={k: v.clone() for k, v in tr.mom.items()}, grad=tr.grad_flat.clone())
    ok = torch.ones((1,), dtype=torch.int32, device=DEV)

    def per_tensor_update():
        e = tr.eng
        ok.fill_(1)
        ops.check_finite_(tr.grad_flat, ok)
        for k, pm in tr.master.items():
            ops.sgd_step_(pm, tr.grad[k], tr.mom[k], tr.lr, tr.momentum, tr.weight_decay, 1.0 / tr._scale_used, tr.row_scale.get(k), tr.lowp.get(k), ok)
        for n in tr.conv_names:
            ops.pack_dgrad_weight(e.w[n + ".w"], tr.wd[n])
        for fc, w in (("fc1", e.fc1_w), ("fc2", e.fc2_w)):
            ops.pack_dgrad_weight(w, tr.wd[fc].view(w.shape[1], w.shape[0]))

    state = {}
    for multi in (True, False):
        update = (lambda: tr._update(1)) if multi else per_tensor_update
        for k in snap["master"]:
            tr.master[k].copy_(snap["master"][k])
            tr.mom[k].copy_(snap["mom"][k])
        for _ in range(2):
            tr.grad_flat.copy_(snap["grad"])
            update()
        # a poisoned gradient: the overflow flag gates the whole update
        before = {k: v.clone() for k, v in tr.master.items()}
        tr.grad_flat.fill_(float("inf"))
        update()
        torch.cuda.synchronize()
        assert all(torch.equal(before[k], tr.master[k]) for k in before), "an overflowed update must not touch the masters"
        assert tr.poll_overflow(wait=True) if multi else int(ok) == 0
        state[multi] = dict(master={k: v.clone() for k, v in tr.master.items()}, mom={k: v.clone() for k, v in tr.mom.items()},
                            lowp={k: v.clone() for k, v in tr.lowp.items() if v is not None}, wd={k: v.clone() for k, v in tr.wd.items()})
    moved = sum(int(not torch.equal(state[True]["master"][k], snap["master"][k])) for k in snap["master"])
    assert moved == len(snap["master"]), "every parameter tensor must have been updated"
    assert sorted(state[True]["wd"]) == sorted(tr.conv_names + ["fc1", "fc2"])  # (the per-tensor form above repacks every one of them)
    for group in ("master", "mom", "lowp", "wd"):
        for k, a in state[True][group].items():
            assert torch.equal(a, state[False][group][k]), (group, k)


def test_sparse_row_list_overflow_poisons_the_gradient_and_skips_the_update(setup):
    """'the sparse CF-RPN row list did not fit' is a rank-local verdict; it must reach every rank. It is folded into the
    gradient (inf in the head conv's bias gradient, in front of that bucket's all-reduce), so the finiteness check of the reduced
    buffer fails everywhere. Here, one rank: an iteration whose list exceeds the (lowered) cap leaves a non-finite bias gradient,
    changes no parameter and counts as an overflow; with the cap back the same trainer steps normally."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]
    args = (d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    tr = OpensetRCNNTrainer(setup["params"], dtype=torch.float16, device=DEV, lr=0.01, loss_scale=512.0)
    rn = "proposal_generator.rpn_head.conv"
    before = {k: v.clone() for k, v in tr.master.items()}
    tr.sparse_rows_cap = 3  # every real iteration lists more rows than this
    tr.step(*args)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(tr.grad[rn + ".b"]).all()), "the verdict must be visible in the gradient itself"
    assert all(torch.equal(before[k], tr.master[k]) for k in before), "an iteration whose list did not fit must not touch the masters"
    assert tr.poll_overflow(wait=True)
    tr.sparse_rows_cap = None
    tr.step(*args)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.grad_flat).all())
    assert not tr.poll_overflow(wait=True)
    assert sum(int(not torch.equal(before[k], tr.master[k])) for k in before) == len(before)


def test_null_update_changes_nothing(setup):
    """bench.py's no-collective timing (config 4's `all_reduce_hidden_fraction`) runs the update's launches with nothing to apply
    (it used to apply the LOCAL gradient on every rank): masters, momentum, low-precision copies and backward-data weights
    are bit for bit unchanged after a real step's momentum is in place, and no verdict reaches the loss scaler."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]
    args = (d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    tr = OpensetRCNNTrainer(setup["params"], dtype=torch.float16, device=DEV, lr=0.01, loss_scale=512.0)
    tr.step(*args)  # non-zero momentum
    tr.poll_overflow(wait=True)
    torch.cuda.synchronize()
    snap = dict(master={k: v.clone() for k, v in tr.master.items()}, mom={k: v.clone() for k, v in tr.mom.items()},
                lowp={k: v.clone() for k, v in tr.lowp.items() if v is not None}, wd={k: v.clone() for k, v in tr.wd.items()})
    assert any(float(v.abs().max()) > 0 for v in snap["mom"].values())
    pending = len(tr.scaler.pending) if hasattr(tr.scaler, "pending") else None
    tr.step(*args, update=False)
    tr.buckets.reset()
    tr.grad_flat.zero_()
    tr.null_update()
    torch.cuda.synchronize()
    for group, cur in (("master", tr.master), ("mom", tr.mom), ("lowp", tr.lowp), ("wd", tr.wd)):
        for k, a in snap[group].items():
            assert torch.equal(a, cur[k]), (group, k)
    if pending is not None:
        assert len(tr.scaler.pending) == pending
    assert not tr.poll_overflow(wait=True)


def test_chained_res3_forward_gives_the_same_step(setup):
    """The trainer's res3 blocks run conv2 -> conv3 + shortcut as one launch that also stores conv2's output
    (osr_conv2d_chain_fwd_ex); against the two launches: identical losses and gradients, bit for bit (the chain kernel is bit-identical
    to the pair, and what it stores is what the pair's first launch stores)."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]
    args = (d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    res = {}
    for chain in (True, False):
        tr = OpensetRCNNTrainer(setup["params"], dtype=torch.float16, device=DEV, lr=5e-5, loss_scale=512.0)
        tr.chain_forward = chain
        out = tr.step(*args, update=False)
        torch.cuda.synchronize()
        res[chain] = ({k: float(v) for k, v in out.items()}, {k: v.clone() for k, v in tr.grad.items()})
    assert res[True][0] == res[False][0]
    for k, a in res[True][1].items():
        assert torch.equal(a, res[False][1][k]), k


def test_prefetched_frozen_prefix_gives_the_same_steps(setup):
    """step(next_images=...) computes the next batch's frozen prefix (stem + res2) under the current backward; the next step() that is
    handed that tensor uses it. Three updates on alternating batches with and without the hand-over: identical losses and parameters,
    bit for bit; a step given ANOTHER tensor than the announced one recomputes (and is still right)."""
    from openset_rcnn_amd.host.train import OpensetRCNNTrainer
    d = setup["dev"]
    imgs_a = d["images"]
    imgs_b = torch.flip(d["images"], dims=(3,)).contiguous()
    rest = (d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    seq = [imgs_a, imgs_b, imgs_a, imgs_b]
    res = {}
    for mode in ("plain", "pipelined", "wrong_announcement"):
        tr = OpensetRCNNTrainer(setup["params"], dtype=torch.float16, device=DEV, lr=0.002, loss_scale=512.0)
        losses = []
        for i in range(3):
            nxt = None if mode == "plain" else (seq[i + 1] if mode == "pipelined" else imgs_a.clone())
            out = tr.step(seq[i], *rest, next_images=nxt)
            losses.append({k: float(v) for k, v in out.items()})
            if mode == "pipelined":
                assert tr._prefetched is not None and tr._prefetched[0] is seq[i + 1]
        torch.cuda.synchronize()
        res[mode] = (losses, {k: v.clone() for k, v in tr.master.items()})
    for mode in ("pipelined", "wrong_announcement"):
        assert res[mode][0] == res["plain"][0], mode
        for k, a in res[mode][1].items():
            assert torch.equal(a, res["plain"][1][k]), (mode, k)


def test_event_scalars_follow_the_reference_definitions(setup):
    """The ten EventStorage scalars of a training iteration (classification_free_rpn.py:459-463,553-554; osrcnn_roi_heads.py:226-228;
    softmax_classifier.py:18-45) from OpensetRCNNTrainer.event_scalars(), recomputed here from the forward's saved tensors."""
    tr, d, n = setup["tr"], setup["dev"], setup["n"]
    _, saved = tr._forward(d["images"], d["hw"], setup["h"], setup["w"], d["gt"], d["gcls"], d["gcnt"], d["keys"])
    sc = tr.event_scalars()
    assert set(sc) == {"rpn/num_pos_anchors", "rpn/num_neg_anchors", "rpn/obj_num_pos_anchors", "rpn/obj_num_neg_anchors", "rpn/num_proposals",
                       "roi_head/num_fg_samples", "roi_head/num_bg_samples", "softmax_classifier/cls_accuracy", "softmax_classifier/fg_cls_accuracy",
                       "softmax_classifier/false_negative"}
    labels, obj = saved["labels"].cpu(), saved["obj_labels"].cpu()
    assert sc["rpn/num_pos_anchors"] == pytest.approx(float((labels == 1).sum()) / n) and sc["rpn/num_neg_anchors"] == pytest.approx(float((labels == 0).sum()) / n)
    assert sc["rpn/obj_num_pos_anchors"] == pytest.approx(float((obj == 1).sum()) / n) and sc["rpn/obj_num_neg_anchors"] == pytest.approx(float((obj == 0).sum()) / n)
    cnt = saved["smp"]["counts"].cpu().float()  # per image: sampled, foreground, background
    assert sc["roi_head/num_fg_samples"] == pytest.approx(float(cnt[:, 1].mean())) and sc["roi_head/num_bg_samples"] == pytest.approx(float(cnt[:, 2].mean()))
    assert sc["roi_head/num_fg_samples"] + sc["roi_head/num_bg_samples"] == pytest.approx(float(cnt[:, 0].mean()))
    valid = saved["smp"]["batch_idx"].view(-1).cpu() >= 0
    cls = saved["cls"].cpu()[valid]
    t = torch.where(cls < 20, cls, torch.where(cls == 81, torch.full_like(cls, 20), torch.full_like(cls, -1)))  # id_map (softmax_classifier.py:224-229)
    pred = saved["logits"].cpu()[valid].argmax(1)
    fg = (t >= 0) & (t < 20)
    assert sc["softmax_classifier/cls_accuracy"] == pytest.approx(float((pred == t).sum()) / len(t))
    assert sc["softmax_classifier/fg_cls_accuracy"] == pytest.approx(float((pred[fg] == t[fg]).sum()) / int(fg.sum()))
    assert sc["softmax_classifier/false_negative"] == pytest.approx(float((pred[fg] == 20).sum()) / int(fg.sum()))
