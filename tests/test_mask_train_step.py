"""Training the mask branch of the stock heads end to end (MODEL.MASK_ON, INPUT.MASK_FORMAT "bitmask") at 2 images of 128 x 160,
NUM_CLASSES 3:

  one step    the branch rebuilt in torch-CPU float64 from the trainer's own saved mask rows (boxes, classes, matched indices), p2..p5
              and the weights as the kernels read them -- oracle RoIAlign 14, mask_fcn*, deconv, predictor, BCE, the stored fp16
              activations taking the trainer's values so that both sides take the same ReLU branches: loss_mask (1e-3), every
              mask master's gradient and the branch's share of the p2..p5 gradient (2e-3 of the tensor's largest magnitude); the four other
              losses and the head-side gradients (cls, box, fc1, fc2, rpn_tail) bit-identical to the same step with MASK_ON False
  round trip  export_state_dict into a fresh model changes its eval-mode pred_masks; the optimizer state survives export and load
  it learns   40 steps on one fixed two-object image: loss_mask ends below, mask_rcnn/accuracy above, its first value
  mirror      model(data) / losses.backward() / optimizer.step() train roi_heads.mask_head.deconv.weight; a batch without any
              foreground steps without NaN"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import osr_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
K = 3
PRE = "roi_heads.mask_head."
SCALES = (0.25, 0.125, 0.0625, 0.03125)


def _cfg(mask_on: bool, agnostic: bool = True, num_conv: int = 1):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "SEED", "3", "MODEL.MASK_ON", str(mask_on), "INPUT.MASK_FORMAT", "bitmask",
                         "MODEL.ROI_HEADS.NUM_CLASSES", str(K), "MODEL.ROI_MASK_HEAD.CLS_AGNOSTIC_MASK", str(agnostic),
                         "MODEL.ROI_MASK_HEAD.NUM_CONV", str(num_conv)])
    return cfg


@functools.lru_cache(maxsize=None)
def _params(agnostic: bool, num_conv: int):
    from openset_rcnn_amd.host.weights import random_standard_params
    p = dict(random_standard_params(0, num_classes=K))
    g = torch.Generator().manual_seed(4100)
    for i in range(1, num_conv + 1):
        p[f"{PRE}mask_fcn{i}.weight"] = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / (256 * 9)) ** 0.5
        p[f"{PRE}mask_fcn{i}.bias"] = torch.randn(256, generator=g) * 0.02
    p[PRE + "deconv.weight"] = torch.randn(256, 256, 2, 2, generator=g) * (2.0 / 256) ** 0.5
    p[PRE + "deconv.bias"] = torch.randn(256, generator=g) * 0.02
    rows = 1 if agnostic else K
    p[PRE + "predictor.weight"] = torch.randn(rows, 256, 1, 1, generator=g) * 0.05
    p[PRE + "predictor.bias"] = torch.randn(rows, generator=g) * 0.1
    return p


def _build(mask_on: bool, agnostic: bool = True, num_conv: int = 1):
    from openset_rcnn_amd.host import modeling as M
    cfg = _cfg(mask_on, agnostic, num_conv)
    model = M.build_model(cfg)
    sd = model.state_dict()
    for k, v in _params(agnostic, num_conv).items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)
    return cfg, model


def _batch(n: int = 2, empty_last: bool = False):
    """Images of 128 x 160 with two objects each: a filled rectangle and a disc, their boxes, classes and full-image bitmasks."""
    from openset_rcnn_amd.host.structures import BitMasks, Boxes, Instances
    g = torch.Generator().manual_seed(7)
    h, w = 128, 160
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    out = []
    for i in range(n):
        img = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
        if empty_last and i == n - 1:
            inst = Instances((h, w), gt_boxes=Boxes(torch.zeros(0, 4)), gt_classes=torch.zeros(0, dtype=torch.int64),
                             gt_masks=BitMasks(torch.zeros(0, h, w)))
        else:
            b = torch.tensor([[10.0, 12.0, 70.0, 90.0], [60.0, 30.0, 150.0, 110.0]]) + 4 * i
            rect = (xx >= b[0, 0]) & (xx < b[0, 2]) & (yy >= b[0, 1]) & (yy < b[0, 3])
            cx, cy, rx, ry = (b[1, 0] + b[1, 2]) / 2, (b[1, 1] + b[1, 3]) / 2, (b[1, 2] - b[1, 0]) / 2, (b[1, 3] - b[1, 1]) / 2
            disc = ((xx + 0.5 - cx) / rx) ** 2 + ((yy + 0.5 - cy) / ry) ** 2 <= 1.0
            img[:, rect] = 220  # (the objects are visible: the branch has something to learn)
            img[:, disc] = 40
            inst = Instances((h, w), gt_boxes=Boxes(b), gt_classes=torch.tensor([0, 1 + i % 2]), gt_masks=BitMasks(torch.stack((rect, disc))))
        out.append({"image": img, "instances": inst})
    return out


def _rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-30))


def _one_step(mask_on, agnostic, num_conv):
    cfg, model = _build(mask_on, agnostic, num_conv)
    model.train()
    tr = model.trainer()
    if mask_on:  # keep what _mask_head_bwd returns: the branch's own share of the p2..p5 gradient
        inner, tr.mask_share = tr._mask_head_bwd, None

        def keep_share(*args):
            tr.mask_share = [t.clone() for t in inner(*args)]
            return tr.mask_share
        tr._mask_head_bwd = keep_share
    tensors = model._train_tensors(_batch(), torch.Generator().manual_seed(0))
    with torch.no_grad():
        losses, saved = tr._forward(*tensors[:8], **model._mask_kwargs(tensors))
        tr._backward(saved, 2)
    torch.cuda.synchronize()
    return model, tr, tensors, losses, saved


def _float64_branch(tr, saved, gt_planes):
    """loss_mask and its gradients in float64 from what the trainer saved."""
    from openset_rcnn_amd.host.weights import unpack_deconv_weight
    from tests.test_mask_train_kernels import roi_align_plane64
    e, ms = tr.eng, saved["mask"]
    res = e.cfg["mask_pooler_resolution"]
    boxes, bidx, cls = ms["boxes"].cpu(), ms["batch_idx"].cpu(), ms["cls"].cpu()
    live = torch.nonzero(bidx >= 0).squeeze(1)
    assert len(live) >= 4, "precondition: the batch has foreground rows"
    feats = [saved["p"][k].detach().cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for k in ("p2", "p3", "p4", "p5")]
    lv = O.assign_levels(boxes[live])
    pooled = torch.zeros(len(live), 256, res, res, dtype=torch.float64)
    for l, sc in enumerate(SCALES):
        ids = torch.nonzero(lv == l).squeeze(1)
        if len(ids):
            rois = torch.cat((bidx[live][ids].float().unsqueeze(1), boxes[live][ids]), dim=1)
            pooled = pooled.index_put((ids,), O.roi_align_torch(feats[l], rois, sc, res))
    # Every stored activation takes the VALUE the trainer saved (the fp16 tensor its backward reads), gradients flowing through the
    # float64 expression: both sides then differentiate the same ReLU branches. (A pre-activation within fp16's rounding of zero
    # takes the other branch in float64 -- about 2e-4 of them, each moving 2304 elements of the layer's data gradient by a full term.)
    # Before a value is substituted it is compared: the float64 pooling / layer must agree with what the trainer's forward stored to
    # fp16's rounding, 2^-10 of the tensor's largest magnitude (one fp16 rounding of the output is 2^-11 of the element; the layer's
    # input is the stored one on both sides). This is the forward check of the 14 x 14 pooler (options, levels) and of mask_fcn*.
    def stored(value64, saved_rows, what):
        kept = saved_rows.detach().cpu().double().permute(0, 3, 1, 2)[live]
        gap = float((kept - value64.detach()).abs().max() / value64.detach().abs().max().clamp(min=1e-30))
        print(f"  forward, {what}: max |stored - float64| / max |float64| = {gap:.2e}")
        assert gap <= 2.0 ** -10, f"{what}: the trainer's forward differs from the float64 rebuild by {gap:.3e}"
        return value64 + (kept - value64).detach()
    pooled = stored(pooled, ms["pooled"], "pooled rows")
    pooled.retain_grad()
    leaves = {}

    def leaf(name, t):
        leaves[name] = t.detach().cpu().double().requires_grad_(True)
        return leaves[name]
    x = pooled
    for i in range(e.mask_num_conv):
        n_ = f"{PRE}mask_fcn{i + 1}"
        x = stored(F.relu(F.conv2d(x, leaf(n_ + ".w", e.w[n_ + ".w"]).permute(0, 3, 1, 2), leaf(n_ + ".b", e.w[n_ + ".b"]), padding=1)), ms["acts"][i], f"mask_fcn{i + 1}")
    u = F.relu(F.conv_transpose2d(x, leaf("mask_deconv.w", unpack_deconv_weight(e.mask_deconv_w)), leaf("mask_deconv.b", e.mask_deconv_b), stride=2))
    z = F.conv2d(u, leaf("mask_pred.w", e.mask_pred_w)[:, :, None, None], leaf("mask_pred.b", e.mask_pred_b))
    rows = torch.zeros(len(live), dtype=torch.int64) if e.mask_pred_w.shape[0] == 1 else cls[live]
    z = z[torch.arange(len(live)), rows]
    # the targets from the matched instances' bitmasks, by the float64 loop of the kernel's own test
    planes, gidx = gt_planes.cpu().numpy(), ms["gt_idx"].reshape(-1).cpu()
    avg = np.stack([roi_align_plane64(planes[int(bidx[r]), int(gidx[r])], boxes[r].numpy(), 2 * res) for r in live.tolist()])
    got_t = ms["targets"].cpu().numpy()[live.numpy()] != 0
    off = (got_t != (avg >= 0.5)) & (np.abs(avg - 0.5) > 1e-5)
    assert not off.any(), f"{int(off.sum())} target pixels differ from the float64 crop_and_resize away from the threshold"
    t = torch.from_numpy(got_t).double()
    assert 0.05 < float(t.mean()) < 0.95
    loss = F.binary_cross_entropy_with_logits(z, t, reduction="mean")
    loss.backward()
    return float(loss.detach()), leaves, feats, (live, pooled.grad)


@pytest.mark.parametrize("agnostic,num_conv", [(True, 1), (False, 4)], ids=["agnostic-1conv", "class-specific-4conv"])
def test_one_step_against_float64_and_against_mask_off(osr, agnostic, num_conv):
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    model, tr, tensors, losses, saved = _one_step(True, agnostic, num_conv)
    assert set(losses) == {"loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask"}
    ref_loss, leaves, feats, (live, d_pooled) = _float64_branch(tr, saved, tensors[8])
    got_loss = float(losses["loss_mask"])
    print(f"loss_mask {got_loss:.6f} (float64 {ref_loss:.6f}), {len(live)} foreground rows")
    assert abs(got_loss - ref_loss) <= 1e-3 * abs(ref_loss)
    S = tr.loss_scale
    bad = []
    for name, lf in leaves.items():
        want = lf.grad
        key = name
        if name == "mask_deconv.w":
            want = pack_deconv_weight(want, torch.float64, frag_elems=8)
        err = _rel(tr.grad[key] / S, want.reshape(tr.grad[key].shape))
        print(f"  {key:44s} rel err {err:.2e}")
        if err > 2e-3:
            bad.append((key, err))
    for l, (got, f64) in enumerate(zip(tr.mask_share, feats)):
        if f64.grad is None:  # no mask row on this level
            assert float(got.abs().max()) == 0.0
            continue
        err = _rel(got / S, f64.grad.permute(0, 2, 3, 1))
        print(f"  share of p{l + 2}: rel err {err:.2e} (max |ref| {float(f64.grad.abs().max()):.3e})")
        if err > 2e-3:
            bad.append((f"p{l + 2}", err))
    assert not bad, bad
    # the same step without the mask branch: same samples, so the box and RPN sides do not move by a bit
    _, tr0, tensors0, losses0, _ = _one_step(False, agnostic, num_conv)
    assert len(tensors0) == 8 and all(torch.equal(tensors[7][k], tensors0[7][k]) for k in tensors0[7])
    for k in ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg"):
        assert torch.equal(losses[k], losses0[k]), k
    for k in ("cls.w", "cls.b", "box.w", "box.b", "fc1.w", "fc1.b", "fc2.w", "fc2.b", "rpn_tail.w", "rpn_tail.b"):
        assert torch.equal(tr.grad[k], tr0.grad[k]), k
    assert set(tr.master) - set(tr0.master) == {k for k in tr.master if k.startswith("mask_") or k.startswith(PRE)}
    sc = tr.event_scalars()
    assert {"mask_rcnn/accuracy", "mask_rcnn/false_positive", "mask_rcnn/false_negative"} <= set(sc) and 0.0 <= sc["mask_rcnn/accuracy"] <= 1.0
    assert "mask_rcnn/accuracy" not in tr0.event_scalars()


def test_round_trip_through_a_fresh_model_and_the_optimizer_state(osr):
    from openset_rcnn_amd.host import modeling as M
    cfg, model = _build(True, False, 1)
    batch = _batch()
    model.eval()
    # the mask head on FIXED boxes (the ground truth's): what changes is the head, not the list of detections
    from openset_rcnn_amd.host.structures import Boxes, Instances
    given = [Instances(d["instances"].image_size, pred_boxes=Boxes(d["instances"].gt_boxes.tensor.to(DEV)),
                       pred_classes=d["instances"].gt_classes.to(DEV)) for d in batch]

    def masks_of(m):
        return torch.cat([o["instances"].pred_masks.flatten() for o in m.inference(batch, detected_instances=given, do_postprocess=False)]).cpu()
    before = masks_of(model)
    assert before.numel() == 4 * 28 * 28
    model.train()
    tr = model.trainer()
    tr.lr = 2e-4
    for _ in range(3):
        tensors = model._train_tensors(batch, torch.Generator().manual_seed(0))
        tr.step(*tensors[:8], **model._mask_kwargs(tensors))
    tr.poll_overflow(wait=True)
    assert tr.overflow_steps == 0
    sd = tr.export_state_dict()
    names = {PRE + "mask_fcn1.weight", PRE + "mask_fcn1.bias", PRE + "deconv.weight", PRE + "deconv.bias", PRE + "predictor.weight", PRE + "predictor.bias"}
    assert names <= set(sd)
    p0 = _params(False, 1)
    for k in names:
        assert tuple(sd[k].shape) == tuple(p0[k].shape) and not torch.equal(sd[k], p0[k]), f"{k} must have been trained"
    # the packed copies the kernels read follow the masters
    from openset_rcnn_amd.host.weights import pack_deconv_weight
    assert torch.equal(tr.eng.mask_deconv_w, pack_deconv_weight(sd[PRE + "deconv.weight"], torch.float16).to(DEV))
    assert torch.equal(tr.mask_deconv_wt, pack_deconv_weight(sd[PRE + "deconv.weight"].half().transpose(0, 1), torch.float16).to(DEV))
    fresh = M.build_model(cfg)
    model.eval()  # (leaving training mode writes the masters back into the module)
    fresh.load_state_dict(model.state_dict())
    assert torch.equal(fresh.state_dict()[PRE + "deconv.weight"].cpu(), sd[PRE + "deconv.weight"])
    fresh.eval()
    after = masks_of(fresh)
    assert after.shape == before.shape and float((after - before).abs().max()) > 0.0, "the trained mask head predicts other masks on the same boxes"
    assert torch.equal(masks_of(model), after), "the fresh model is the trained one"
    opt = tr.export_optimizer_state()
    assert {"mask_deconv.w", "mask_deconv.b", "mask_pred.w", "mask_pred.b", PRE + "mask_fcn1.w", PRE + "mask_fcn1.b"} <= set(opt)
    assert float(opt["mask_deconv.w"].abs().max()) > 0.0
    fresh.train()
    tr2 = fresh.trainer()
    tr2.load_optimizer_state(opt)
    for k in tr.mom:
        assert torch.equal(tr2.mom[k], tr.mom[k]), k


def test_it_learns_a_fixed_image(osr):
    cfg, model = _build(True, True, 1)
    batch = _batch(1)
    model.train()
    tr = model.trainer()
    tr.lr = 2e-4  # (the synthetic weights start far from a minimum: larger steps diverge within a few iterations)
    tr.scaler.growth_interval = 0
    first = last = None
    for it in range(40):
        tensors = model._train_tensors(batch, torch.Generator().manual_seed(0))
        out = tr.step(*tensors[:8], **model._mask_kwargs(tensors))
        if it in (0, 39):
            rec = (float(out["loss_mask"]), tr.event_scalars()["mask_rcnn/accuracy"])
            first, last = (rec, last) if it == 0 else (first, rec)
    tr.poll_overflow(wait=True)
    print(f"loss_mask {first[0]:.4f} -> {last[0]:.4f}, mask_rcnn/accuracy {first[1]:.4f} -> {last[1]:.4f}")
    assert tr.overflow_steps == 0
    assert last[0] < first[0] and last[1] > first[1]


def test_mirror_trains_the_mask_head_and_survives_a_batch_without_foreground(osr):
    from openset_rcnn_amd.host.solver import build_optimizer
    cfg, model = _build(True, True, 1)
    model.train()
    optimizer = build_optimizer(cfg, model)
    w0 = model.state_dict()[PRE + "deconv.weight"].detach().cpu().clone()
    loss_dict = model(_batch())
    assert "loss_mask" in loss_dict and loss_dict["loss_mask"].is_cuda and float(loss_dict["loss_mask"]) > 0.0
    losses = sum(loss_dict.values())
    optimizer.zero_grad()
    losses.backward()
    optimizer.step()
    assert {"mask_rcnn/accuracy", "mask_rcnn/false_positive", "mask_rcnn/false_negative"} <= set(model.event_scalars())
    # no instance anywhere: no foreground row, loss_mask exactly 0, every mask gradient exactly 0, nothing turns NaN
    empty = _batch(2)
    for d in empty:
        d["instances"] = _batch(1, empty_last=True)[0]["instances"]
    loss_dict = model(empty)
    assert float(loss_dict["loss_mask"]) == 0.0 and all(bool(torch.isfinite(v)) for v in loss_dict.values())
    optimizer.zero_grad()
    sum(loss_dict.values()).backward()
    tr = model.trainer()
    for k in tr.grad:
        if k.startswith("mask_") or k.startswith(PRE):
            assert float(tr.grad[k].abs().max()) == 0.0, k
    optimizer.step()
    tr.poll_overflow(wait=True)
    assert tr.overflow_steps == 0 and all(bool(torch.isfinite(v).all()) for v in tr.master.values())
    model.eval()
    assert not torch.equal(model.state_dict()[PRE + "deconv.weight"].detach().cpu(), w0)
