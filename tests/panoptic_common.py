"""References and inputs shared by the Panoptic FPN tests (no test lives here): torch-CPU code written from the contract in include/osr.h.

  gn_merge_reference        sum_t up_t(relu(group_norm_t(x_t))) in float64 on the stored inputs
  resample_reference        F.interpolate(x4) -> crop -> F.interpolate(size) in float64
  combine_reference         detectron2's combine_semantic_and_instance_outputs loop, with the branch each instance / label took
  combine_scene             the 40 x 56 scene of tests/test_panoptic_combine.py
  combine_ragged_plane, combine_limits, combine_boundary_scene, combine_rounded_threshold_scene, combine_scene_with_ignored_labels
                            the inputs that take osr_panoptic_combine past word 1024, to k = 1024 and 255 labels, and onto its thresholds
  resample_logits           the seeded stride-4 logits of tests/test_semseg_resample.py
  RESAMPLE_WIDE_CASES       more classes than one LDS pass of osr_semseg_resample holds, and one-row / one-cell maps"""
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


def word_range(mask, width):
    """mask (H, W) bool with a set pixel -> (wlo, whi): the 64-pixel words [wlo, whi) of the rows from its first to its last set one,
    the range pc_walk_kernel walks for the instance (csrc/osr_panoptic.hip)."""
    rows = torch.nonzero(mask.any(dim=1)).flatten()
    y0, y1 = int(rows[0]), int(rows[-1]) + 1
    return y0 * width // 64, (y1 * width + 63) // 64


RAGGED_THRESHOLDS = dict(overlap_thresh=0.5, stuff_area_limit=256, instances_confidence_thresh=0.5)


def combine_ragged_plane(seed=4):
    """300 x 333 = 99 900 pixels = 1560 words and 60 pixels, k = 48 -> (masks bool, scores, classes, labels): instance 0 covers every
    row (a range of 1561 words), 1 starts at word 1092, 2 is the last row's tail in the partial last word, 3 overlaps 0 and 1; then
    44 seeded rectangles with sides 4 .. 120 and scores 0.4 .. 0.9; labels of 54 classes in 16 x 16 blocks."""
    g = torch.Generator().manual_seed(seed)
    h, w, k = 300, 333, 48
    masks = torch.zeros(k, h, w, dtype=torch.bool)
    masks[0, :, 100:140] = True
    masks[1, 210:290, 5:300] = True
    masks[2, 299:300, 300:333] = True
    masks[3, 205:215, 120:200] = True
    for i in range(4, k):
        y0, x0 = int(torch.randint(0, h - 4, (1,), generator=g)), int(torch.randint(0, w - 4, (1,), generator=g))
        y1, x1 = y0 + int(torch.randint(4, 121, (1,), generator=g)), x0 + int(torch.randint(4, 121, (1,), generator=g))
        masks[i, y0:min(y1, h), x0:min(x1, w)] = True
    scores = torch.rand(k, generator=g) * 0.5 + 0.4
    scores[:4] = torch.tensor([0.99, 0.98, 0.97, 0.96])
    classes = torch.randint(0, 80, (k,), generator=g)
    blocks = torch.randint(0, 54, (h // 16 + 1, w // 16 + 1), generator=g)
    labels = blocks.repeat_interleave(16, 0).repeat_interleave(16, 1)[:h, :w].to(torch.int32).contiguous()
    return masks, scores, classes, labels


LIMITS_THRESHOLDS = dict(overlap_thresh=0.5, stuff_area_limit=2, instances_confidence_thresh=0.5)


def combine_limits(seed=9):
    """32 x 48, k = 1024 single-pixel masks at distinct positions, scores from eight values in [0.5, 1.0] (long runs of equal scores);
    the other 512 pixels carry the labels 1 .. 255 twice each and 0 twice, the instance pixels random labels 0 .. 255: with
    stuff_area_limit = 2 every instance and every label takes a row, 1024 + 255 = the table's capacity."""
    g = torch.Generator().manual_seed(seed)
    h, w, k = 32, 48, 1024
    perm = torch.randperm(h * w, generator=g)
    masks = torch.zeros(k, h * w, dtype=torch.bool)
    masks[torch.arange(k), perm[:k]] = True
    scores = torch.linspace(0.5, 1.0, 8)[torch.randint(0, 8, (k,), generator=g)].contiguous()
    classes = torch.randint(0, 80, (k,), generator=g)
    labels = torch.zeros(h * w, dtype=torch.int32)
    labels[perm[:k]] = torch.randint(0, 256, (k,), generator=g).to(torch.int32)
    labels[perm[k:k + 510]] = torch.arange(1, 256, dtype=torch.int32).repeat(2)
    return masks.reshape(k, h, w), scores, classes, labels.reshape(h, w).contiguous()


def f32(v):
    """The double that a C `float` argument holds for the Python float v."""
    return float(torch.tensor(v, dtype=torch.float32))


def below(v):
    """The next fp32 value under v, as a double."""
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(0.0)))


def combine_boundary_scene(frac, conf):
    """8 x 40: A = columns 0 .. 7 (kept); B has `frac` of its 64 pixels on A: inter / area == frac exactly (kept where the threshold is
    frac: the test is `>`); C has one column more on A and B than that (overlap); D's score is `conf` exactly (kept); E's is the next
    fp32 value below (ends the walk); F would be kept but comes after E. frac in {0.5, 0.25}; frac and conf dyadic."""
    n = int(8 * frac)
    boxes = [(0, 8, 0, 8), (0, 8, 8 - n, 16 - n), (0, 8, 15 - 2 * n, 23 - 2 * n), (2, 6, 30, 36), (0, 2, 36, 40), (6, 8, 36, 40)]
    masks = torch.zeros(len(boxes), 8, 40, dtype=torch.bool)
    for i, (y0, y1, x0, x1) in enumerate(boxes):
        masks[i, y0:y1, x0:x1] = True
    scores = torch.tensor([0.9, 0.8, 0.75, conf, below(conf), 0.3], dtype=torch.float32)
    classes = torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int64)
    labels = torch.zeros(8, 40, dtype=torch.int32)
    labels[:, 20:30] = 4
    return masks, scores, classes, labels


def combine_rounded_threshold_scene():
    """4 x 32 for overlap_thresh = instances_confidence_thresh = 0.7, which a C float holds as 0.699999988: B has 7 of its 10 pixels
    on A, and 7 / 10 in double is above that float (overlap) though not above the double 0.7; C's score is float32(0.7), which is
    not below that float (kept) though below the double 0.7; D's is the next fp32 value below (ends the walk)."""
    boxes = [(0, 4, 0, 7), (0, 1, 0, 10), (2, 4, 20, 30), (0, 2, 12, 18)]
    masks = torch.zeros(len(boxes), 4, 32, dtype=torch.bool)
    for i, (y0, y1, x0, x1) in enumerate(boxes):
        masks[i, y0:y1, x0:x1] = True
    scores = torch.tensor([0.9, 0.8, 0.7, below(0.7)], dtype=torch.float32)
    classes = torch.tensor([1, 2, 3, 4], dtype=torch.int64)
    labels = torch.zeros(4, 32, dtype=torch.int32)
    labels[:, 16:32] = 2
    return masks, scores, classes, labels


IGNORED_LABELS = (256, 100000, -1)


def combine_scene_with_ignored_labels():
    """combine_scene() with the labels 256, 100000 and -1 painted over label-0 pixels that no kept instance covers (224, 224 and 24
    pixels). -> (masks, scores, classes, labels as given to the kernel, labels with those pixels set to 0 for the reference)."""
    masks, scores, classes, labels = combine_scene()
    dirty = labels.clone()
    dirty[2:16, 40:56], dirty[16:30, 40:56], dirty[0:2, 44:56] = IGNORED_LABELS
    assert bool((labels[dirty != labels] == 0).all())
    return masks, scores, classes, dirty, labels


# (name, C, pitch, (h4, w4), crop, output) for osr_semseg_resample beyond one 56-class pass through LDS, and on degenerate maps
RESAMPLE_WIDE_CASES = [
    ("a", 57, 60, (5, 9), (19, 34), (23, 70)),      # the second pass holds exactly one real class
    ("b", 133, 136, (5, 9), (19, 34), (23, 70)),    # three passes
    ("c", 150, 152, (5, 9), (20, 36), (20, 36)),    # three passes, identity scale
    ("d", 150, 152, (1, 7), (4, 27), (9, 65)),      # h4 == 1 (every second row tap clamps), a 65-pixel output row
    ("e", 19, 20, (1, 1), (3, 2), (7, 5)),          # a single stride-4 cell
]


def resample_wide_logits(case, seed=21):
    """Standard-normal logits (h4, w4, C) of a RESAMPLE_WIDE_CASES row under torch.manual_seed(seed)."""
    _, c, _, (h4, w4), _, _ = case
    torch.manual_seed(seed)
    return torch.randn(h4, w4, c)


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
