"""References and inputs shared by the Panoptic FPN tests (no test lives here): torch-CPU code written from the contract in include/osr.h.

  gn_merge_reference        sum_t up_t(relu(group_norm_t(x_t))) in float64 on the stored inputs
  resample_reference        F.interpolate(x4) -> crop -> F.interpolate(size) in float64
  combine_reference         detectron2's combine_semantic_and_instance_outputs loop, with the branch each instance / label took
  combine_scene             the 40 x 56 scene of tests/test_panoptic_combine.py
  resample_logits           the seeded stride-4 logits of tests/test_semseg_resample.py"""
import torch
import torch.nn.functional as F

GROUPS, EPS = 32, 1e-5
RESAMPLE_C, RESAMPLE_PITCH, RESAMPLE_H4, RESAMPLE_W4 = 54, 56, 16, 24
RESAMPLE_CASES = [((61, 90), (97, 143)), ((64, 96), (64, 96)), ((50, 77), (33, 51))]  # (crop, output): upscale, identity, downscale
SCENE_THRESHOLDS = dict(overlap_thresh=0.5, stuff_area_limit=200, instances_confidence_thresh=0.5)


def gn_stats_reference(x):
    """x (n, h, w, c) as stored -> (mean, rstd) (n, 32) float64, biased variance."""
    n, h, w, c = x.shape
    g = x.double().reshape(n, h * w, GROUPS, c // GROUPS).permute(0, 2, 1, 3).reshape(n, GROUPS, -1)
    mean = g.mean(dim=2)
    var = ((g - mean[:, :, None]) ** 2).mean(dim=2)
    return mean, 1.0 / torch.sqrt(var + EPS)


def gn_merge_reference(terms):
    """terms: (x (n, h, w, c) as stored, gamma or None, beta or None, up2) -> the float64 sum (n, ho, wo, c), not yet rounded."""
    total = None
    for x, gamma, beta, up2 in terms:
        v = x.double().permute(0, 3, 1, 2)
        if gamma is not None:
            v = F.group_norm(v, GROUPS, gamma.double(), beta.double(), EPS)
        v = F.relu(v)
        if up2:
            v = F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)
        total = v if total is None else total + v
    return total.permute(0, 2, 3, 1).contiguous()


def resample_logits(seed=11):
    """Standard-normal logits (h4, w4, C) under torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    return torch.randn(RESAMPLE_H4, RESAMPLE_W4, RESAMPLE_C)


def resample_reference(logits, crop_hw, out_hw):
    """logits (h4, w4, C) -> (C, oh, ow) float64: detectron2's two interpolations."""
    x = logits.double().permute(2, 0, 1)[None]
    x = F.interpolate(x, scale_factor=4, mode="bilinear", align_corners=False)
    x = x[:, :, : crop_hw[0], : crop_hw[1]]
    return F.interpolate(x, size=tuple(out_hw), mode="bilinear", align_corners=False)[0]


def top_two_gap(values):
    """(C, h, w) -> (h, w): the gap between the largest and the second largest class."""
    top = torch.topk(values, 2, dim=0).values
    return top[0] - top[1]


def combine_reference(masks, scores, classes, labels, overlap_thresh, stuff_area_limit, instances_confidence_thresh):
    """[d2] combine_semantic_and_instance_outputs on CPU tensors: masks (k, H, W) bool, scores (k), classes (k), labels (H, W).
    -> (panoptic_seg (H, W) int32, table rows [isthing, category_id, instance_id or -1, area], scores per row, events).
    A thing's area is the number of pixels it painted. events: (kind, index) with kind in {"break", "empty", "overlap", "kept",
    "clipped", "stuff_kept", "stuff_small"}."""
    pan = torch.zeros(labels.shape, dtype=torch.int32)
    order = torch.sort(-scores.double(), stable=True).indices.tolist()
    table, seg_scores, events, cur = [], [], [], 0
    for i in order:
        score = float(scores[i])
        if score < instances_confidence_thresh:
            events.append(("break", i))
            break
        mask = masks[i].bool()
        area = int(mask.sum())
        if area == 0:
            events.append(("empty", i))
            continue
        inter = int((mask & (pan > 0)).sum())
        if inter * 1.0 / area > overlap_thresh:
            events.append(("overlap", i))
            continue
        if inter > 0:
            mask = mask & (pan == 0)
            events.append(("clipped", i))
        events.append(("kept", i))
        cur += 1
        pan[mask] = cur
        table.append([1, int(classes[i]), i, area - inter])
        seg_scores.append(score)
    for label in torch.unique(labels).tolist():
        if label == 0:
            continue
        mask = (labels == label) & (pan == 0)
        area = int(mask.sum())
        if area < stuff_area_limit:
            events.append(("stuff_small", label))
            continue
        events.append(("stuff_kept", label))
        cur += 1
        pan[mask] = cur
        table.append([0, int(label), -1, area])
        seg_scores.append(0.0)
    return pan, table, seg_scores, events


def segments_info_reference(table, seg_scores):
    out = []
    for r, (row, sc) in enumerate(zip(table, seg_scores)):
        if row[0]:
            out.append({"id": r + 1, "isthing": True, "score": sc, "category_id": row[1], "instance_id": row[2]})
        else:
            out.append({"id": r + 1, "isthing": False, "category_id": row[1], "area": row[3]})
    return out


def combine_scene():
    """-> (masks (6, 40, 56) bool, scores (6) fp32, classes (6) int64, labels (40, 56) int32)."""
    h, w = 40, 56
    labels = torch.zeros(h, w, dtype=torch.int32)
    labels[:, 0:20] = 3
    labels[:, 20:40] = 7
    labels[30:40, 40:56] = 5
    labels[0:2, 40:44] = 9
    boxes = [((5, 25), (5, 25)), ((6, 24), (6, 24)), ((5, 25), (20, 40)), None, ((0, 40), (22, 40)), ((0, 10), (44, 56))]
    masks = torch.zeros(len(boxes), h, w, dtype=torch.bool)
    for i, b in enumerate(boxes):
        if b is not None:
            masks[i, b[0][0]:b[0][1], b[1][0]:b[1][1]] = True
    scores = torch.tensor([0.95, 0.90, 0.85, 0.80, 0.70, 0.40], dtype=torch.float32)
    classes = torch.tensor([2, 2, 1, 4, 0, 3], dtype=torch.int64)
    return masks, scores, classes, labels
