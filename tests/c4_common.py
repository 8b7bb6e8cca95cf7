"""Shared by the C4 tests: seeded parameters under detectron2's faster_rcnn_R_50_C4 names and the CPU reference of the model,
composed from oracle.osr_oracle (frozen_bn_fold's folded form, anchor_grid, standard_rpn_head, standard_find_top_rpn_proposals,
roi_align_torch, fast_rcnn_inference_from_outputs) with F.conv2d for the trunk and res5. Every stage is a function of its own, so a
test can feed it the engine's intermediates."""
import re

import torch
import torch.nn.functional as F

from oracle import osr_oracle as O

SIZES, RATIOS, STRIDE = (32, 64, 128, 256, 512), (0.5, 1.0, 2.0), 16
A = len(SIZES) * len(RATIOS)
IMAGE_SIZES = [(96, 128), (128, 160)]
PIXEL_MEAN = (103.53, 116.28, 123.675)
RES5 = "roi_heads.res5"


def make_c4_params(seed=0, num_classes=80, res_gain=0.5):
    """O.make_r50_fpn_params' BN-folded trunk (residual gain 0.5) under the C4 names -- stem and res2..res4 under backbone.*, res5
    under roi_heads.res5.* -- with a StandardRPNHead on 1024 channels (15 anchors) and FastRCNNOutputLayers on 2048, scaled so that
    logits and deltas spread."""
    p = {}
    for k, v in O.make_r50_fpn_params(seed, res_gain).items():
        m = re.fullmatch(r"backbone\.bottom_up\.(stem|res[2-5])\.(.+)", k)
        if m:
            p[(f"{RES5}." if m.group(1) == "res5" else f"backbone.{m.group(1)}.") + m.group(2)] = v
    g = torch.Generator().manual_seed(seed + 4000)
    rpn = "proposal_generator.rpn_head."
    p[rpn + "conv.weight"] = torch.randn(1024, 1024, 3, 3, generator=g) * 0.01
    p[rpn + "conv.bias"] = torch.zeros(1024)
    p[rpn + "objectness_logits.weight"] = torch.randn(A, 1024, 1, 1, generator=g) * 0.25
    p[rpn + "objectness_logits.bias"] = torch.zeros(A)
    p[rpn + "anchor_deltas.weight"] = torch.randn(4 * A, 1024, 1, 1, generator=g) * 0.05
    p[rpn + "anchor_deltas.bias"] = torch.zeros(4 * A)
    p["roi_heads.box_predictor.cls_score.weight"] = torch.randn(num_classes + 1, 2048, generator=g) * 0.1
    p["roi_heads.box_predictor.cls_score.bias"] = torch.zeros(num_classes + 1)
    p["roi_heads.box_predictor.bbox_pred.weight"] = torch.randn(4 * num_classes, 2048, generator=g) * 0.02
    p["roi_heads.box_predictor.bbox_pred.bias"] = torch.zeros(4 * num_classes)
    return p


def load_folded(model, params):
    """BN-folded parameters into the model mirror: a folded bias becomes the FrozenBN's bias (its scale is exactly 1 at initialisation)."""
    sd = model.state_dict()
    for k, v in params.items():
        if k in sd:
            sd[k] = v
        else:
            assert k.endswith(".bias") and k[:-5] + ".norm.bias" in sd, k
            sd[k[:-5] + ".norm.bias"] = v
    model.load_state_dict(sd)


def images(seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in IMAGE_SIZES]


def stacked(imgs):
    """The engine's input: one float tensor, the smaller image padded bottom / right with the pixel mean (zero after normalisation)."""
    hm, wm = max(i.shape[1] for i in imgs), max(i.shape[2] for i in imgs)
    batch = torch.tensor(PIXEL_MEAN).view(1, 3, 1, 1).repeat(len(imgs), 1, hm, wm)
    for k, im in enumerate(imgs):
        batch[k, :, : im.shape[1], : im.shape[2]] = im.float()
    return batch


def _cv(t, p, name, stride=1, pad=0):
    return F.conv2d(t, p[name + ".weight"].to(t.dtype), p[name + ".bias"].to(t.dtype), stride=stride, padding=pad)


def bottleneck(t, p, pre, first, stride, s1x1, q):
    s1, s2 = (stride, 1) if s1x1 else (1, stride)
    sc = q(_cv(t, p, pre + ".shortcut", stride)) if first else t
    o = q(F.relu(_cv(t, p, pre + ".conv1", s1)))
    o = q(F.relu(_cv(o, p, pre + ".conv2", s2, 1)))
    return q(F.relu(_cv(o, p, pre + ".conv3") + sc))


def trunk(x, p, s1x1=True, q=lambda t: t):
    """[d2] build_resnet_backbone, OUT_FEATURES ["res4"], on the normalised padded batch."""
    t = q(F.relu(_cv(x, p, "backbone.stem.conv1", 2, 3)))
    t = F.max_pool2d(t, kernel_size=3, stride=2, padding=1)
    for stage, nb in ((2, 3), (3, 4), (4, 6)):
        for b in range(nb):
            t = bottleneck(t, p, f"backbone.res{stage}.{b}", b == 0, 2 if (b == 0 and stage > 2) else 1, s1x1, q)
    return t


def anchors(shape):
    """[d2] DefaultAnchorGenerator with five sizes on one level from O.anchor_grid (one size per call): size-major, then ratio."""
    hw = shape[0] * shape[1]
    return torch.cat([O.anchor_grid([shape], [STRIDE], [z], RATIOS)[0].view(hw, len(RATIOS), 4) for z in SIZES], dim=1).reshape(-1, 4)


def rpn_head(res4, p):
    """-> (logits (n, h*w*A), deltas (n, h*w*A, 4)) in [d2] RPN.forward's flattening."""
    d, l = O.standard_rpn_head(res4, p)
    ds, ls = O.flatten_head_outputs([d], [l])
    return ls[0], ds[0]


def proposals(logits, deltas, shape, image_sizes, pre, post, nms=0.7):
    n = logits.shape[0]
    a = anchors(shape)
    props = O.b2b_apply_deltas(deltas.reshape(-1, 4), a.unsqueeze(0).expand(n, -1, -1).reshape(-1, 4), (1.0, 1.0, 1.0, 1.0)).view(n, -1, 4)
    return O.standard_find_top_rpn_proposals([props], [logits], image_sizes, nms, pre, post)


def pooled_full(res4, boxes_per_image, out_size=14):
    """[d2] ROIPooler with one level: (M, 1024, P, P), the full grid."""
    rois = torch.cat([torch.cat((torch.full((len(b), 1), float(i)), b), dim=1) for i, b in enumerate(boxes_per_image)])
    return O.roi_align_torch(res4, rois, 1.0 / STRIDE, out_size)


def res5(x, p, s1x1=True, q=lambda t: t):
    """res5 on the FULL pooled grid (M, 1024, P, P) -> (M, 2048, ceil(P / 2), ceil(P / 2)); in x's dtype (float32 or float64)."""
    for b in range(3):
        x = bottleneck(x, p, f"{RES5}.{b}", b == 0, 2 if b == 0 else 1, s1x1, q)
    return x


def res5_on_even_bins(x, p, q=lambda t: t):
    """res5 with STRIDE_IN_1X1 on the even bins of the grid, (M, 1024, q, q): its first block's two stride-2 1x1 layers read nothing
    else, so they run at stride 1 here -- the same function of the full grid."""
    for b in range(3):
        x = bottleneck(x, p, f"{RES5}.{b}", b == 0, 1, True, q)
    return x


def predictor(box_feats, p):
    pre = "roi_heads.box_predictor."
    return F.linear(box_feats, p[pre + "cls_score.weight"], p[pre + "cls_score.bias"]), F.linear(box_feats, p[pre + "bbox_pred.weight"], p[pre + "bbox_pred.bias"])


def detect(imgs, p, s1x1=True, pre=6000, post=100, cfg=O.BASE_RCNN_CFG):
    """The whole model in fp32 on the CPU -> per image (boxes, scores, classes, (row, class))."""
    x = (stacked(imgs) - torch.tensor(PIXEL_MEAN).view(1, 3, 1, 1))
    sizes = [(int(i.shape[1]), int(i.shape[2])) for i in imgs]
    f = trunk(x, p, s1x1)
    lg, dl = rpn_head(f, p)
    props = proposals(lg, dl, tuple(f.shape[-2:]), sizes, pre, post)
    feats = res5(pooled_full(f, [pr[0] for pr in props]), p, s1x1).mean(dim=(2, 3))
    logits, deltas = predictor(feats, p)
    counts = [len(pr[0]) for pr in props]
    return [O.fast_rcnn_inference_from_outputs(l, d, pr[0], s, cfg) for l, d, pr, s in zip(logits.split(counts), deltas.split(counts), props, sizes)]


def storage_eps(dtype):
    """Half an ulp, relative: what one rounding to the storage dtype costs."""
    return {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}[dtype]
