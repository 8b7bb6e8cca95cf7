"""META_ARCHITECTURE "RetinaNet" on the engine (host/engine_retinanet.py) against a torch-CPU fp32 network written here with F.conv2d:
the R-50 trunk with folded FrozenBN, the FPN on res3..res5, LastLevelP6P7 on res5 (the ReLU only on p7's input), the two towers, cls_score
and bbox_pred, and behind them the contract of include/osr.h restated by tests/test_retinanet_select.py's reference plus a greedy per-class
NMS. Two images of different sizes within a 128 x 160 pad, K = 5.

Bounds: max |got - ref| / max |ref| < 1e-4 per tensor for the fp32 engine (the project's fp32 contract) and < 2e-2 for the fp16 engine
(the bound of the deform trunk test); the parity engine's detections equal the reference's in count, class and order, boxes within
1e-4 * max(1, |coordinate|)."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_retinanet_select import A, reference as select_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
R50_BLOCKS = (3, 4, 6, 3)
K, TOPK, DETS = 5, 1000, 60
SIZES = [(128, 160), (112, 144)]
HP, WP = 128, 160
STRIDES = (8, 16, 32, 64, 128)
SCORE_THRESH, NMS_THRESH = 0.05, 0.5
# cls_score's bias and the seed: chosen on the CPU so that the reference alone yields >= 50 detections per image and none of its candidate
# logits lies within 1e-3 of the threshold (both asserted in test_reference_is_well_conditioned), and so that the 60 detections' scores
# lie at least 1e-4 apart (their order is compared exactly; fp32 sums in another order move a score by about 1e-6)
CLS_BIAS, CLS_GAIN, SEED = -9.8, 3.0, 7
MEAN = (103.53, 116.28, 123.675)


def logit_thresh():
    return float(np.float32(math.log(SCORE_THRESH / (1.0 - SCORE_THRESH))))


def rel(a, b):
    return float((a.detach().float().cpu() - b).abs().max() / b.abs().max())


def cpu_network(P, x):
    """x (n,3,HP,WP) normalised, zero padded -> (pyramid p3..p7 NCHW, logits per level (n,h,w,A*K), deltas per level (n,h,w,A*4))."""
    def conv(x, name, stride=1, pad=0, relu=False):
        y = F.conv2d(x, P[name + ".weight"], P[name + ".bias"], stride, pad)
        return F.relu(y) if relu else y
    bu = "backbone.bottom_up."
    x = F.max_pool2d(conv(x, bu + "stem.conv1", 2, 3, True), 3, 2, 1)
    feats = {}
    for si, nb in enumerate(R50_BLOCKS):
        for b in range(nb):
            pre, st = f"{bu}res{si + 2}.{b}", 2 if (b == 0 and si > 0) else 1
            sc = conv(x, pre + ".shortcut", st) if b == 0 else x
            o = conv(conv(conv(x, pre + ".conv1", st, 0, True), pre + ".conv2", 1, 1, True), pre + ".conv3")
            x = F.relu(o + sc)
        feats[si + 2] = x
    lat = conv(feats[5], "backbone.fpn_lateral5")
    out = {"p5": conv(lat, "backbone.fpn_output5", 1, 1)}
    for lvl in (4, 3):
        lat = conv(feats[lvl], f"backbone.fpn_lateral{lvl}") + F.interpolate(lat, scale_factor=2, mode="nearest")
        out[f"p{lvl}"] = conv(lat, f"backbone.fpn_output{lvl}", 1, 1)
    out["p6"] = conv(feats[5], "backbone.top_block.p6", 2, 1)
    out["p7"] = conv(F.relu(out["p6"]), "backbone.top_block.p7", 2, 1)
    logits, deltas = [], []
    for k in ("p3", "p4", "p5", "p6", "p7"):
        tc = tb = out[k]
        for i in range(4):
            tc = conv(tc, f"head.cls_subnet.{2 * i}", 1, 1, True)
            tb = conv(tb, f"head.bbox_subnet.{2 * i}", 1, 1, True)
        logits.append(conv(tc, "head.cls_score", 1, 1).permute(0, 2, 3, 1).contiguous())
        deltas.append(conv(tb, "head.bbox_pred", 1, 1).permute(0, 2, 3, 1).contiguous())
    return out, logits, deltas


def cpu_nms(boxes, scores, cls, cand, thr, topk):
    """Greedy per-class NMS on the padded candidate list: score descending (ties: lower row first), IoU > thr suppresses."""
    rows = torch.nonzero(cand > 0).reshape(-1)
    rows = rows[torch.sort(-scores[rows].double(), stable=True).indices]
    kept = []
    for r in rows.tolist():
        b = boxes[r]
        ok = True
        for q in kept:
            if cls[q] != cls[r]:
                continue
            c = boxes[q]
            iw = (torch.min(b[2], c[2]) - torch.max(b[0], c[0])).clamp(min=0)
            ih = (torch.min(b[3], c[3]) - torch.max(b[1], c[1])).clamp(min=0)
            inter = iw * ih
            union = (b[2] - b[0]) * (b[3] - b[1]) + (c[2] - c[0]) * (c[3] - c[1]) - inter
            if inter / union > thr:
                ok = False
                break
        if ok:
            kept.append(r)
            if len(kept) == topk:
                break
    return kept


@functools.lru_cache(maxsize=None)
def setup():
    """The parameters, the images and the CPU reference, computed once and shared by the tests below (read-only)."""
    from openset_rcnn_amd.host.engine_std import cell_anchor_table
    from openset_rcnn_amd.host.weights import random_retinanet_params
    P = random_retinanet_params(SEED, num_classes=K, cls_bias=CLS_BIAS)
    P["head.cls_score.weight"] = P["head.cls_score.weight"] * CLS_GAIN  # (logits spread over several units: scores from the threshold up to ~0.9)
    g = torch.Generator().manual_seed(21)
    images = [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in SIZES]
    x = torch.zeros(len(images), 3, HP, WP)
    mean = torch.tensor(MEAN).view(3, 1, 1)
    for i, im in enumerate(images):
        x[i, :, : im.shape[1], : im.shape[2]] = im.float() - mean
    with torch.no_grad():
        pyr, logits, deltas = cpu_network(P, x)
    levels = [(l.shape[1], l.shape[2], s) for l, s in zip(logits, STRIDES)]
    sizes = [[x_ * 2 ** (i / 3) for i in range(3)] for x_ in (32, 64, 128, 256, 512)]
    anchors = cell_anchor_table(sizes, (0.5, 1.0, 2.0))
    cands = select_reference(levels, len(images), K, TOPK, logit_thresh(), (1.0,) * 4, logits, deltas, anchors)
    dets = []
    for i in range(len(images)):
        keep = cpu_nms(cands["c_boxes"][i], cands["c_scores"][i], cands["c_cls"][i], cands["c_cand"][i], NMS_THRESH, DETS)
        dets.append(dict(boxes=cands["c_boxes"][i][keep], scores=cands["c_scores"][i][keep], cls=cands["c_cls"][i][keep]))
    return dict(P=P, images=images, pyr=pyr, logits=logits, deltas=deltas, levels=levels, anchors=anchors, cands=cands, dets=dets, sizes=sizes)


def engine_cfg():
    return dict(retina_num_classes=K, retina_topk=TOPK, retina_score_thresh=SCORE_THRESH, retina_nms_thresh=NMS_THRESH, std_detections_per_image=DETS,
                pixel_mean=MEAN, pixel_std=(1.0, 1.0, 1.0))


def run_engine(dtype, profile=False):
    from openset_rcnn_amd.host.engine_retinanet import RetinaNetEngine
    s = setup()
    eng = RetinaNetEngine(s["P"], engine_cfg(), dtype, DEV)
    batch = torch.full((2, 3, HP, WP), 0.0)
    batch[:] = torch.tensor(MEAN).view(1, 3, 1, 1)  # (padding = the pixel mean: zero once normalised)
    for i, im in enumerate(s["images"]):
        batch[i, :, : im.shape[1], : im.shape[2]] = im.float()
    batch = batch.to(DEV)
    hw = torch.tensor(SIZES, dtype=torch.int32, device=DEV)
    keep = {}
    if profile:
        eng.profile, eng.profile_hbm = [], []
    out = eng.forward_device(batch, hw, HP, WP, keep)
    torch.cuda.synchronize()
    return eng, batch, hw, out, keep


def test_reference_is_well_conditioned(osr):
    s = setup()
    th = logit_thresh()
    for i, d in enumerate(s["dets"]):
        assert len(d["scores"]) >= 50, (i, len(d["scores"]))
    gap = min(float((l[..., :A * K].float() - th).abs().min()) for l in s["logits"])
    assert gap > 1e-3, gap
    assert s["cands"]["flag"] == 0
    for d in s["dets"]:
        assert float((d["scores"][:-1] - d["scores"][1:]).min()) >= 1e-4


def level_views(flat, levels, n, pitch, width):
    out, off = [], 0
    for h, w, _ in levels:
        out.append(flat[off:off + n * h * w * pitch].view(n, h, w, pitch)[..., :width])
        off += n * h * w * pitch
    return out


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.float16, 2e-2)], ids=["fp32", "fp16"])
def test_pyramid_logits_and_deltas_match_the_cpu_network(osr, dtype, tol):
    s = setup()
    eng, _, _, _, keep = run_engine(dtype)
    assert eng.pitch_cls == 48 and eng.pitch_box == 40  # A*K = 45 and A*4 = 36, padded to the next multiple of 8
    for k in ("p3", "p4", "p5", "p6", "p7"):
        got = keep["feats"][k].permute(0, 3, 1, 2)
        assert got.shape == s["pyr"][k].shape, k
        r = rel(got, s["pyr"][k])
        print(f"[rel] {str(dtype)[6:]} {k}: {r:.3e} (bound {tol:g})")
        assert r < tol, (k, r)
    assert float(keep["feats"]["p6"].min()) < 0  # p6 is handed on without the ReLU
    assert keep["logits"].dtype == dtype and keep["deltas"].dtype == torch.float32
    for name, flat, pitch, width, ref in (("logits", keep["logits"], eng.pitch_cls, A * K, s["logits"]), ("deltas", keep["deltas"], eng.pitch_box, A * 4, s["deltas"])):
        for li, (got, want) in enumerate(zip(level_views(flat, s["levels"], 2, pitch, width), ref)):
            scale = max(float(w_.abs().max()) for w_ in ref)
            r = float((got.float().cpu() - want).abs().max()) / scale
            print(f"[rel] {str(dtype)[6:]} {name} level {li}: {r:.3e} (bound {tol:g})")
            assert r < tol, (name, li, r)


def test_parity_engine_detections_equal_the_reference(osr):
    s = setup()
    _, _, _, (ob, osc, ocl, cnt), keep = run_engine(torch.float32)
    assert int(keep["cands"]["status_flags"].item()) == 0
    for i, d in enumerate(s["dets"]):
        k = int(cnt[i])
        assert k == len(d["scores"]), (i, k, len(d["scores"]))
        assert torch.equal(ocl[i, :k].cpu(), d["cls"].to(torch.int64)), i
        assert bool((ocl[i, k:] == -1).all())
        err = (ob[i, :k].cpu().double() - d["boxes"]).abs()
        assert bool((err <= 1e-4 * d["boxes"].abs().clamp(min=1.0)).all()), float(err.max())
        assert float((osc[i, :k].cpu() - d["scores"]).abs().max()) <= 1e-4
        assert bool((osc[i, :k - 1] >= osc[i, 1:k]).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_eager_and_captured_passes_are_bit_identical(osr, dtype):
    eng, batch, hw, out, _ = run_engine(dtype)
    eager = [t.clone() for t in out]
    again = eng.forward_device(batch, hw, HP, WP)
    graph, cap = eng.capture(batch, hw, HP, WP)
    for t in cap:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(cap) == 4 and int(eager[3].sum()) > 0
    for a, b, c in zip(cap, eager, again):
        assert torch.equal(a, b) and torch.equal(c, b)


def test_profile_lists_the_eight_tower_launches(osr):
    eng, _, _, _, _ = run_engine(torch.float16, profile=True)
    names = [e[0] for e in eng.profile]
    towers = [n for n in names if "subnet" in n]
    assert towers == [f"head.{sub}.{2 * i} (p3-p7, one launch)" for sub in ("cls_subnet", "bbox_subnet") for i in range(4)], towers
    assert sum(n == "head.cls_score" for n in names) == 5 and sum(n == "head.bbox_pred" for n in names) == 5
    assert "backbone.fpn_output3-5 (three levels, one launch)" in names and "backbone.top_block.p6" in names and "backbone.top_block.p7" in names
    assert not [n for n in names if "fpn_lateral2" in n or "fpn_output2" in n or "rpn_head" in n]
    hbm = [e[0] for e in eng.profile_hbm]
    assert "retinanet_select" in hbm and "nms_topk(retinanet, per class)" in hbm


def _cfg(yaml, *opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", DEV] + list(opts))
    return cfg


def test_model_returns_instances_at_the_requested_size(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.structures import Instances
    s = setup()
    model = M.build_model(_cfg("retinanet_fpn.yaml", "MODEL.RETINANET.NUM_CLASSES", str(K), "TEST.DETECTIONS_PER_IMAGE", str(DETS)))
    sd = model.state_dict()
    for k, v in s["P"].items():
        if k in sd:
            assert sd[k].shape == v.shape, k
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
        else:
            raise AssertionError(k)
    model.load_state_dict(sd)
    model.eval()
    model.kernel_dtype = torch.float32
    outs_hw = [(256, 320), (56, 72)]  # twice and half the inputs' sizes
    outs = model([{"image": im, "height": h, "width": w} for im, (h, w) in zip(s["images"], outs_hw)])
    assert len(outs) == 2
    for i, (o, (h, w), (hi, wi)) in enumerate(zip(outs, outs_hw, SIZES)):
        inst = o["instances"]
        assert isinstance(inst, Instances) and inst.image_size == (h, w)
        assert set(inst.get_fields()) == {"pred_boxes", "scores", "pred_classes"}
        b = inst.pred_boxes.tensor
        assert 0 < len(inst) <= DETS and bool((b[:, 0::2] >= 0).all()) and bool((b[:, 0::2] <= w).all()) and bool((b[:, 1::2] >= 0).all()) and bool((b[:, 1::2] <= h).all())
        assert bool((inst.pred_classes >= 0).all()) and bool((inst.pred_classes < K).all())
        # the reference's detections, rescaled and clipped as detector_postprocess does, empties dropped
        d = s["dets"][i]
        rb = d["boxes"].clone() * torch.tensor([w / wi, h / hi, w / wi, h / hi], dtype=torch.float64)
        rb[:, 0::2] = rb[:, 0::2].clamp(0, w)
        rb[:, 1::2] = rb[:, 1::2].clamp(0, h)
        ok = (rb[:, 2] > rb[:, 0]) & (rb[:, 3] > rb[:, 1])
        assert len(inst) == int(ok.sum())
        assert torch.equal(inst.pred_classes.cpu(), d["cls"][ok].to(torch.int64))
        assert float((b.cpu().double() - rb[ok]).abs().max()) <= 1e-3
    with pytest.raises(NotImplementedError, match="RetinaNet"):
        model.train()([{"image": s["images"][0]}])


def test_stock_engine_launches_are_unchanged(osr):
    """The stock Faster R-CNN of base_rcnn_fpn.yaml, built through build_model from a configuration that now carries MODEL.RETINANET,
    launches what a StandardRCNNEngine built directly on the same parameters launches, name for name, with the same bits -- and nothing
    of the one-stage path."""
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
    from openset_rcnn_amd.host.weights import random_standard_params
    P = random_standard_params(0, num_classes=K)
    model = M.build_model(_cfg("base_rcnn_fpn.yaml", "MODEL.ROI_HEADS.NUM_CLASSES", str(K)))
    sd = model.state_dict()
    for k, v in P.items():
        if k in sd:
            sd[k] = v
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
        else:
            raise AssertionError(k)
    model.load_state_dict(sd)
    model.eval()
    eng = model.engine()
    assert type(eng) is StandardRCNNEngine
    direct = StandardRCNNEngine(P, dict(model._eng_cfg), torch.float16, DEV)
    images = torch.randint(0, 256, (2, 3, 128, 160), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(DEV)
    hw = torch.tensor([(128, 160)] * 2, dtype=torch.int32, device=DEV)
    res, names = [], []
    for e in (eng, direct):
        e.profile, e.profile_hbm = [], []
        res.append(e.forward_device(images, hw, 128, 160))
        torch.cuda.synchronize()
        names.append([x[0] for x in e.profile] + [x[0] for x in e.profile_hbm])
        e.profile = e.profile_hbm = None
    assert names[0] == names[1] and len(names[0]) > 40
    assert not [n for n in names[0] if "head." in n and "rpn_head" not in n and "box_head" not in n and "mask_head" not in n]
    assert not [n for n in names[0] if "top_block" in n or "retinanet" in n]
    assert "backbone.fpn_output2-5 (four levels, one launch)" in names[0]
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
