"""CascadeROIHeads at inference on the HIP path, n = 2 images of 128 x 160 with seeded synthetic weights:

* a one-stage cascade carrying the StandardROIHeads (CLS_AGNOSTIC_BBOX_REG True) weights gives the stock heads' detections bit for
  bit, and their masks with MODEL.MASK_ON;
* three stages in the fp32 parity mode against a torch restatement of detectron2's CascadeROIHeads._forward_box (written here) over
  the oracle's backbone, RPN, pooler and box-head helpers: at least 95 % of the detections agree (tests/test_standard_rcnn.py's
  criterion: IoU >= 0.99, score within 1e-2, same class); every stage's pooled features, logits, deltas and input boxes meet the
  1e-4 fp32 contract, each stage computed from the engine's own inputs to that stage;
* the fp16 pass runs and returns finite detections."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import c_binding as CO
from oracle import osr_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
H, W, N = 128, 160, 2
POST_TOPK = 300
STAGE_WEIGHTS = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))


def _cfg(yaml, *opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.RPN.POST_NMS_TOPK_TEST", str(POST_TOPK)] + list(opts))
    return cfg


def _one_stage(*opts):
    return _cfg("cascade_rcnn_fpn.yaml", "MODEL.ROI_BOX_CASCADE_HEAD.IOUS", "(0.5,)", "MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS",
                "((10.0, 10.0, 5.0, 5.0),)", *opts)


@functools.lru_cache(maxsize=None)
def _images():
    g = torch.Generator().manual_seed(7)
    return torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8)


def _mask_params(k):
    g = torch.Generator().manual_seed(4000)
    pre, p = "roi_heads.mask_head.", {}
    for i in range(1, 5):
        p[f"{pre}mask_fcn{i}.weight"] = torch.randn(256, 256, 3, 3, generator=g) * (2.0 / (256 * 9)) ** 0.5
        p[f"{pre}mask_fcn{i}.bias"] = torch.randn(256, generator=g) * 0.02
    p[pre + "deconv.weight"] = torch.randn(256, 256, 2, 2, generator=g) * (2.0 / 256) ** 0.5
    p[pre + "deconv.bias"] = torch.randn(256, generator=g) * 0.02
    p[pre + "predictor.weight"] = torch.randn(1, 256, 1, 1, generator=g) * 0.05
    p[pre + "predictor.bias"] = torch.randn(1, generator=g) * 0.1
    return p


def _model(cfg, params, dtype=torch.float16):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(cfg)
    sd = model.state_dict()
    loaded = 0
    for k, v in params.items():
        if k in sd:
            sd[k] = v
            loaded += 1
        elif k.endswith(".bias") and k[:-5] + ".norm.bias" in sd:
            sd[k[:-5] + ".norm.bias"] = v
    assert loaded >= len([k for k in sd if k.startswith("roi_heads.")])
    model.load_state_dict(sd)
    model.kernel_dtype = dtype
    return model.eval()


@pytest.mark.parametrize("mask", [False, True], ids=["boxes", "mask"])
def test_one_stage_cascade_equals_the_stock_heads(osr, mask):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.engine_cascade import CascadeRCNNEngine
    from openset_rcnn_amd.host.weights import random_cascade_params, random_standard_params
    opts = ("MODEL.MASK_ON", "True") if mask else ()
    std_p, cas_p = dict(random_standard_params(0)), dict(random_cascade_params(0, stages=1))
    for k, v in std_p.items():  # the very same tensors under the two heads' names
        ck = k.replace("roi_heads.box_head.", "roi_heads.box_head.0.").replace("roi_heads.box_predictor.", "roi_heads.box_predictor.0.")
        assert torch.equal(cas_p[ck], v), k
    if mask:
        std_p.update(_mask_params(80))
        cas_p.update(_mask_params(80))
    std = _model(_cfg("base_rcnn_fpn.yaml", *opts), std_p)
    cas = _model(_one_stage(*opts), cas_p)
    assert type(cas.roi_heads) is M.CascadeROIHeads and type(cas.engine()) is CascadeRCNNEngine and cas.engine().num_stages == 1
    sizes = [(H, W)] * N
    a = std.engine().forward(_images().to(DEV), sizes)
    b = cas.engine().forward(_images().to(DEV), sizes)
    torch.cuda.synchronize()
    assert len(a) == len(b) == (5 if mask else 4)
    assert torch.equal(a[3], b[3]) and int(a[3].min()) > 0
    for i, c in enumerate(a[3].cpu().tolist()):
        for x, y in zip(a, b):
            if x.dim() > 1:
                assert torch.equal(x[i, :c], y[i, :c])
    # and through the model: Instances with the same fields
    inputs = [{"image": im, "height": H, "width": W} for im in _images()]
    for ra, rb in zip(std(inputs), cas(inputs)):
        ia, ib = ra["instances"], rb["instances"]
        assert torch.equal(ia.pred_boxes.tensor.cpu(), ib.pred_boxes.tensor.cpu()) and torch.equal(ia.scores.cpu(), ib.scores.cpu())
        assert torch.equal(ia.pred_classes.cpu(), ib.pred_classes.cpu())
        if mask:
            assert torch.equal(ia.pred_masks.cpu(), ib.pred_masks.cpu())


# ---- three stages against detectron2's _forward_box, restated -----------------------------------------------------------------------
def _stage_ref(feats, boxes_per_image, p, s, roi_align_fn=None):
    """One stage of [d2] CascadeROIHeads._run_stage at inference on per-image boxes: pooler, box_head[s], box_predictor[s].
    -> (pooled (M, 256, 7, 7), logits (M, K+1), deltas (M, 4))."""
    pooled = O.roi_pooler_ref([feats[k] for k in ("p2", "p3", "p4", "p5")], boxes_per_image, roi_align_fn=roi_align_fn or CO.roi_align)
    x = O.box_head(pooled, p, prefix=f"roi_heads.box_head.{s}")
    bp = f"roi_heads.box_predictor.{s}."
    return pooled, F.linear(x, p[bp + "cls_score.weight"], p[bp + "cls_score.bias"]), F.linear(x, p[bp + "bbox_pred.weight"], p[bp + "bbox_pred.bias"])


def _cascade_forward_box_ref(feats, proposals, sizes, p, stages=3, score_thresh=0.05, nms_thresh=0.5, topk=100):
    """[d2] CascadeROIHeads._forward_box, inference branch: every stage on the previous stage's predict_boxes (clipped, none dropped),
    scores = sum of the stages' softmax * (1 / stages), boxes = the last stage's predict_boxes, then fast_rcnn_inference."""
    boxes = [pr[0] for pr in proposals]
    counts = [len(b) for b in boxes]
    probs = []
    for s in range(stages):
        if s > 0:
            boxes = [O.box_clip(O.b2b_apply_deltas(d, b, STAGE_WEIGHTS[s - 1]), size) for d, b, size in zip(deltas.split(counts), boxes, sizes)]
        _, logits, deltas = _stage_ref(feats, boxes, p, s)
        probs.append(F.softmax(logits, dim=-1))
    scores = sum(probs) * (1.0 / stages)
    out = []
    for sc, d, b, size in zip(scores.split(counts), deltas.split(counts), boxes, sizes):
        fb = O.b2b_apply_deltas(d, b, STAGE_WEIGHTS[stages - 1])
        valid = torch.isfinite(fb).all(dim=1) & torch.isfinite(sc).all(dim=1)
        fb, sc = O.box_clip(fb[valid], size), sc[valid][:, :-1]
        mask = sc > score_thresh
        idx = mask.nonzero()
        cb, cs = fb[idx[:, 0]], sc[mask]
        keep = torch.from_numpy(O.batched_nms_ref(cb.numpy(), cs.numpy(), idx[:, 1].numpy(), nms_thresh))[:topk]
        out.append((cb[keep], cs[keep], idx[keep, 1]))
    return out


def _nchw(t):
    return t.detach().cpu().float().permute(0, 3, 1, 2).contiguous()


def _within(got, ref, what):
    err, scale = float((got - ref).abs().max()), max(1.0, float(ref.abs().max()))
    print(f"[{what}] max |got - ref| = {err:.3e} (bound {1e-4 * scale:.3e})")
    assert err <= 1e-4 * scale, what


def test_three_stages_in_parity_mode_match_the_restatement(osr):
    from openset_rcnn_amd.host.weights import random_cascade_params
    params = random_cascade_params(0, stages=3)
    model = _model(_cfg("cascade_rcnn_fpn.yaml"), params, torch.float32)
    eng = model.engine()
    assert eng.num_stages == 3 and eng.stage_weights == STAGE_WEIGHTS
    keep = {}
    sizes = [(H, W)] * N
    res = eng.forward(_images().to(DEV), sizes, keep=keep)
    torch.cuda.synchronize()
    # ---- every stage from the engine's own inputs to it: its boxes and the engine's pyramid ----
    feats = {k: _nchw(v) for k, v in keep["feats"].items()}
    sel = keep["sel"]
    counts = [int(c) for c in sel["counts"].cpu()]
    cap = sel["cap"]
    assert min(counts) > 50
    for s in range(3):
        eb = keep[f"boxes_s{s}"].cpu().view(N, cap, 4)
        per_image = [eb[i, :counts[i]] for i in range(N)]
        pooled, logits, deltas = _stage_ref(feats, per_image, params, s)
        rows = torch.cat([torch.arange(counts[i]) + i * cap for i in range(N)])
        _within(keep[f"pooled_s{s}"].cpu().float().permute(0, 3, 1, 2)[rows], pooled, f"stage {s} pooled")
        _within(keep[f"logits_s{s}"].cpu()[rows], logits, f"stage {s} logits")
        _within(keep[f"deltas_s{s}"].cpu()[rows], deltas, f"stage {s} deltas")
        if s < 2:  # the boxes the next stage gets: this stage's deltas on this stage's boxes, clipped; every row stays
            nxt = keep[f"boxes_s{s + 1}"].cpu()[rows]
            want = O.box_clip(O.b2b_apply_deltas(keep[f"deltas_s{s}"].cpu()[rows], torch.cat(per_image), STAGE_WEIGHTS[s]), (H, W))
            _within(nxt, want, f"stage {s + 1} input boxes")
        pad = torch.ones(N * cap, dtype=torch.bool)
        pad[rows] = False
        assert not bool(keep[f"pooled_s{s}"].cpu()[pad].any())  # rows that do not exist pool zeros
    # ---- the whole network against the fp32 restatement ----
    batch, _ = O.preprocess_images(list(_images()))
    rfeats = O.resnet_fpn_forward(batch, params)
    props, _ = O.standard_rpn_inference(rfeats, sizes, params, dict(O.BASE_RCNN_CFG, post_nms_topk_test=POST_TOPK))
    ref = _cascade_forward_box_ref(rfeats, props, sizes, params)
    matched = total = 0
    for i in range(N):
        m = int(res[3][i])
        gb, gs, gc = res[0][i, :m].cpu(), res[1][i, :m].cpu(), res[2][i, :m].cpu()
        rb, rs, rc = ref[i]
        assert m > 0 and len(rb) > 0
        iou = O.pairwise_iou(rb, gb)
        used = torch.zeros(m, dtype=torch.bool)
        for j in range(len(rb)):
            ok = (iou[j] >= 0.99) & ((gs - rs[j]).abs() <= 1e-2) & (gc == rc[j]) & ~used
            if bool(ok.any()):
                used[int(torch.nonzero(ok)[0])] = True
                matched += 1
        total += max(m, len(rb))
    print(f"[cascade, parity mode] {matched}/{total} detections agree with the fp32 restatement")
    assert matched >= 0.95 * total


def test_fp16_pass_returns_finite_detections(osr):
    from openset_rcnn_amd.host.weights import random_cascade_params
    model = _model(_cfg("cascade_rcnn_fpn.yaml"), random_cascade_params(0, stages=3), torch.float16)
    out = model([{"image": im, "height": H, "width": W} for im in _images()])
    assert len(out) == N
    for o in out:
        inst = o["instances"]
        assert 0 < len(inst) <= 100
        b, s, c = inst.pred_boxes.tensor.cpu(), inst.scores.cpu(), inst.pred_classes.cpu()
        assert bool(torch.isfinite(b).all()) and bool(torch.isfinite(s).all()) and bool(((c >= 0) & (c < 80)).all())
        assert bool((s > 0.05).all()) and bool((b[:, 2] > b[:, 0]).all()) and bool((b[:, 3] > b[:, 1]).all())
        assert bool((b[:, 2] <= W).all()) and bool((b[:, 3] <= H).all())
    # forward_device(mask=False) works as for the parent
    eng = model.engine()
    res = eng.forward_device(_images().to(DEV), torch.tensor([(H, W)] * N, dtype=torch.int32, device=DEV), H, W, mask=False)
    assert len(res) == 4 and int(res[3].min()) > 0
