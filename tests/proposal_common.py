"""Shared by the box-proposal recall tests: a literal numpy version of the matching loop, seeded images (proposals near and far from
their ground truths, on a quarter-pixel grid, logits that repeat), and the specification's outputs laid out like osr_proposal_recall's
(hits, num_pos, per-ground-truth overlaps)."""
import numpy as np
import torch

AREAS = ("all", "small", "medium", "large")
LIMITS = (100, 1000)


def literal_overlaps(boxes, logits, gt_boxes, gt_area, lo, hi, limit):
    """The loop as the header describes it, on the full matrix, numpy fp32 -> overlaps (G) with -1 at the invalid ground truths, or
    None for an image that adds nothing."""
    boxes, logits = np.asarray(boxes, dtype=np.float32).reshape(-1, 4), np.asarray(logits, dtype=np.float32).reshape(-1)
    gt_boxes, gt_area = np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 4), np.asarray(gt_area, dtype=np.float32).reshape(-1)
    if len(boxes) == 0 or len(gt_boxes) == 0:
        return None
    order = np.argsort(-logits, kind="stable")
    out = -np.ones(len(gt_boxes), dtype=np.float32)
    valid = np.nonzero((gt_area >= np.float32(lo)) & (gt_area <= np.float32(hi)))[0]
    if len(valid) == 0:
        return out
    live = boxes[order][: len(boxes) if limit is None else min(len(boxes), limit)]
    m = np.zeros((len(live), len(valid)), dtype=np.float32)
    for p, b in enumerate(live):
        for c, j in enumerate(valid):
            g = gt_boxes[j]
            a1, a2 = (b[2] - b[0]) * (b[3] - b[1]), (g[2] - g[0]) * (g[3] - g[1])
            w, h = max(min(b[2], g[2]) - max(b[0], g[0]), np.float32(0)), max(min(b[3], g[3]) - max(b[1], g[1]), np.float32(0))
            inter = np.float32(w * h)
            m[p, c] = inter / np.float32(np.float32(a1 + a2) - inter) if inter > 0 else 0
    out[valid] = 0
    for _ in range(min(len(live), len(valid))):
        best_c, best_p, best = -1, -1, np.float32(-1)
        for c in range(len(valid)):          # ground truths in annotation order ...
            for p in range(len(live)):       # ... proposals in rank order: a strict > keeps the first of equals
                if m[p, c] > best:
                    best_c, best_p, best = c, p, m[p, c]
        out[valid[best_c]] = best
        m[best_p, :] = -2
        m[:, best_c] = -2
    return out


def seeded_image(rng, n_props, n_gt, extent=400.0):
    """-> (boxes (n_props, 4) fp32 xyxy, logits (n_props) fp32 multiples of 1/32, gt_boxes (n_gt, 4) fp32 xyxy, gt_area (n_gt) fp32).
    Ground truths straddle 32^2 and 96^2 (some exactly on them); about half of the proposals are jittered copies of ground truths, a
    few exact copies (IoU 1), the rest anywhere (many disjoint from everything)."""
    side = rng.choice([6.0, 14.0, 32.0, 34.0, 60.0, 96.0, 97.0, 130.0], size=(n_gt, 2))
    xy = rng.integers(0, int(extent * 4), size=(n_gt, 2)) / 4.0
    gt = np.concatenate([xy, xy + side], axis=1).astype(np.float32)
    area = (side[:, 0] * side[:, 1]).astype(np.float32)
    pside = rng.choice([8.0, 20.0, 40.0, 90.0, 140.0], size=(n_props, 2)) + rng.integers(0, 8, size=(n_props, 2)) / 4.0
    pxy = rng.integers(0, int(extent * 4), size=(n_props, 2)) / 4.0
    boxes = np.concatenate([pxy, pxy + pside], axis=1).astype(np.float32)
    if n_gt:
        src = rng.integers(0, n_gt, size=n_props)
        near = rng.random(n_props) < 0.5
        jit = gt[src] + rng.integers(-16, 17, size=(n_props, 4)).astype(np.float32) / 4.0
        jit[:, 2:] = np.maximum(jit[:, 2:], jit[:, :2] + 0.25)
        boxes[near] = jit[near]
        exact = rng.random(n_props) < 0.05
        boxes[exact] = gt[src][exact]
    logits = (rng.integers(-64, 65, size=n_props) / 32.0).astype(np.float32)
    return boxes, logits, gt, area


def pad_batch(images, cap, rng):
    """images: seeded_image tuples -> (boxes (n, cap, 4), logits (n, cap), counts (n) int32, gt_boxes (NG, 4), gt_area (NG), seg_off
    (n + 1) int32). The rows past an image's count hold plausible boxes and high logits, which must not count."""
    n = len(images)
    boxes = np.zeros((n, cap, 4), dtype=np.float32)
    logits = np.zeros((n, cap), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    for i, (b, s, g, _) in enumerate(images):
        k = len(b)
        counts[i] = k
        boxes[i, :k], logits[i, :k] = b, s
        if cap > k:
            fill = g[rng.integers(0, len(g), size=cap - k)] if len(g) else np.tile(np.float32([0, 0, 50, 50]), (cap - k, 1))
            boxes[i, k:], logits[i, k:] = fill, 5.0
    per = [len(g) for _, _, g, _ in images]
    seg_off = np.concatenate(([0], np.cumsum(per))).astype(np.int32)
    gt_boxes = np.concatenate([g for _, _, g, _ in images]).reshape(-1, 4).astype(np.float32)
    gt_area = np.concatenate([a for _, _, _, a in images]).astype(np.float32)
    return boxes, logits, counts, gt_boxes, gt_area, seg_off


def specification_outputs(images, areas=AREAS, limits=LIMITS, thresholds=None):
    """host/proposal_evaluation.match_image per (image, area range, limit) -> (hits (n, A, L, T) int32, num_pos (n, A) int32, overlaps
    (A, L, NG) fp32, -1 where the kernel writes -1)."""
    from openset_rcnn_amd.host import proposal_evaluation as PE
    thresholds = PE.default_thresholds() if thresholds is None else thresholds
    n, ng = len(images), sum(len(g) for _, _, g, _ in images)
    hits = np.zeros((n, len(areas), len(limits), len(thresholds)), dtype=np.int32)
    num_pos = np.zeros((n, len(areas)), dtype=np.int32)
    overlaps = -np.ones((len(areas), len(limits), ng), dtype=np.float32)
    g0 = 0
    for i, (b, s, g, ar) in enumerate(images):
        for a, area in enumerate(areas):
            for l, limit in enumerate(limits):
                ov = PE.match_image(torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(g), torch.from_numpy(ar), PE.AREA_RANGES[area], limit)
                if ov is None:
                    continue
                overlaps[a, l, g0:g0 + len(g)] = ov.numpy()
                num_pos[i, a] = int((ov >= 0).sum())
                hits[i, a, l] = ((ov[None, :] >= thresholds[:, None]) & (ov[None, :] >= 0)).sum(dim=1).numpy()
        g0 += len(g)
    return hits, num_pos, overlaps


def coco_gt(image_ids, gts):
    """gts: per image (gt_boxes xyxy, gt_area[, crowd flags]) -> a COCO JSON dict with one category; ids are assigned in order from 1."""
    anns = []
    for img, g in zip(image_ids, gts):
        boxes, area = g[0], g[1]
        crowd = g[2] if len(g) > 2 else [0] * len(boxes)
        for b, a, c in zip(np.asarray(boxes, dtype=np.float64), area, crowd):
            anns.append(dict(image_id=img, category_id=1, bbox=[float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])], area=float(a), iscrowd=int(c)))
    return dict(images=[dict(id=i, file_name=f"{i}.jpg", height=480, width=640) for i in image_ids], categories=[dict(id=1, name="thing")],
                annotations=[dict(a, id=k + 1) for k, a in enumerate(anns)])


def proposals(boxes, logits, device="cpu", size=(480, 640)):
    from openset_rcnn_amd.host.structures import Boxes, Instances
    return Instances(size, proposal_boxes=Boxes(torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4).to(device)),
                     objectness_logits=torch.as_tensor(logits, dtype=torch.float32).reshape(-1).to(device))
