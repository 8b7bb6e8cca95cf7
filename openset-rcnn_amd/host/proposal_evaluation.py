"""Class-agnostic box-proposal recall: AR@100 / AR@1000 over all, small, medium and large ground truths, as the reference's evaluator
reports it for the first stage (os_coco_evaluation.py `_eval_box_proposals`; detectron2's COCOEvaluator does the same).

  * `evaluate_box_proposals` is the specification: a plain torch-CPU loop over the full IoU matrix of every image. It scores CPU
    proposals and is what the tests hold the kernel against, bit for bit.
  * `ProposalRecall` is what the evaluators own. Device proposals go through ops.proposal_recall once per batch, every area range and
    both limits in one launch; only the integer sums `hits` and `num_pos` stay, on the device, until ONE copy in `state()`. CPU
    proposals are kept and scored by the specification. Both paths end in `finish`, so they return equal figures, and the sums of
    several ranks add.

Not built: re-reading stored proposals (MODEL.LOAD_PROPOSALS, --resume_test), LVIS proposal AR (host/lvis_evaluation.py scores LVIS
detections and refuses outputs that carry only proposals)."""
from __future__ import annotations

import os
import pickle
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .eval_buffers import upload_sections

# name -> [lo, hi] of the annotation's area, both ends inclusive; the first four are what the evaluators report
AREA_RANGES = {"all": (0 ** 2, 1e5 ** 2), "small": (0 ** 2, 32 ** 2), "medium": (32 ** 2, 96 ** 2), "large": (96 ** 2, 1e5 ** 2),
               "96-128": (96 ** 2, 128 ** 2), "128-256": (128 ** 2, 256 ** 2), "256-512": (256 ** 2, 512 ** 2), "512-inf": (512 ** 2, 1e5 ** 2)}
REPORTED_AREAS = {"all": "", "small": "s", "medium": "m", "large": "l"}  # the metric is "AR{suffix}@{limit}"
REPORTED_LIMITS = (100, 1000)
BBOX_MODE_XYXY_ABS = 0  # [d2] BoxMode.XYXY_ABS, what box_proposals.pkl declares
PROPOSALS_FILE = "box_proposals.pkl"


def default_thresholds() -> torch.Tensor:
    """The ten IoU thresholds 0.5 .. 0.95 as the fp32 values the reference compares with."""
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)


def area_range_tensor(names: Sequence[str]) -> torch.Tensor:
    return torch.tensor([AREA_RANGES[a] for a in names], dtype=torch.float32).reshape(-1, 2)


def image_ground_truth(tables, image_id) -> Tuple[np.ndarray, np.ndarray]:
    """An image's non-crowd annotations in the JSON's order -> (boxes (G, 4) fp32 xyxy, area (G) fp32). The corner x + w is formed in
    double and rounded once, as BoxMode.convert on the JSON's numbers followed by torch.as_tensor does."""
    pos = tables.img_pos.get(image_id)
    if pos is None:
        return np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.float32)
    r = np.arange(tables.start[pos], tables.start[pos + 1])
    r = r[tables.crowd[r] == 0]
    r = r[np.argsort(tables.json_pos[r], kind="mergesort")]
    b = tables.box[r]
    xyxy = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], axis=1).astype(np.float32).reshape(-1, 4)
    return xyxy, tables.area[r].astype(np.float32)


def pairwise_iou(boxes: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """[d2] pairwise_iou in fp32, every operation rounded on its own: (M, 4) x (G, 4) xyxy -> (M, G); inter / (a1 + a2 - inter) where
    inter > 0, else 0."""
    a1, a2 = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]), (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    w = (torch.min(boxes[:, None, 2], gt[None, :, 2]) - torch.max(boxes[:, None, 0], gt[None, :, 0])).clamp(min=0)
    h = (torch.min(boxes[:, None, 3], gt[None, :, 3]) - torch.max(boxes[:, None, 1], gt[None, :, 1])).clamp(min=0)
    inter = w * h
    union = a1[:, None] + a2[None, :] - inter
    return torch.where(inter > 0, inter / union, torch.zeros_like(inter))


def match_image(boxes: torch.Tensor, logits: torch.Tensor, gt_boxes: torch.Tensor, gt_area: torch.Tensor, area_range, limit: Optional[int]):
    """One image, one area range, one limit -> overlaps (G) fp32: the recorded IoU of each valid ground truth, -1 for the others; None
    when the image adds nothing (no proposal, or no non-crowd ground truth). See evaluate_box_proposals for the rules."""
    boxes, logits = boxes.detach().to(torch.float32).reshape(-1, 4), logits.detach().to(torch.float32).reshape(-1)
    gt_boxes, gt_area = gt_boxes.to(torch.float32).reshape(-1, 4), gt_area.to(torch.float32).reshape(-1)
    if len(boxes) == 0 or len(gt_boxes) == 0:
        return None
    order = torch.sort(logits, descending=True, stable=True)[1]
    boxes = boxes[order]
    lo, hi = torch.tensor(area_range[0], dtype=torch.float32), torch.tensor(area_range[1], dtype=torch.float32)
    valid = (gt_area >= lo) & (gt_area <= hi)
    out = torch.full((len(gt_boxes),), -1.0, dtype=torch.float32)
    cols = torch.nonzero(valid).reshape(-1)
    if len(cols) == 0:
        return out
    if limit is not None and len(boxes) > limit:
        boxes = boxes[:limit]
    overlaps = pairwise_iou(boxes, gt_boxes[cols])
    out[cols] = 0.0
    for _ in range(min(len(boxes), len(cols))):
        best, best_row = overlaps.max(dim=0)   # per ground truth: its best live proposal, the lowest rank among equals
        iou, g = best.max(dim=0)               # the best-covered ground truth, the lowest index among equals
        p = best_row[g]
        out[cols[g]] = iou
        overlaps[p, :] = -1
        overlaps[:, g] = -1
    return out


def finish(hits: torch.Tensor, num_pos: int, thresholds: torch.Tensor) -> dict:
    """Integer sums -> the figures: recalls = hits / num_pos and ar = their mean, both in fp32. hits (T) integers."""
    recalls = hits.to(torch.float32) / float(num_pos)
    return {"ar": recalls.mean(), "recalls": recalls, "thresholds": thresholds, "num_pos": int(num_pos)}


def evaluate_box_proposals(records: Sequence[dict], tables, area: str = "all", limit: Optional[int] = None,
                           thresholds: Optional[torch.Tensor] = None) -> dict:
    """The specification. records: one dict per image {"image_id", "boxes" (k, 4) xyxy, "objectness_logits" (k)}; tables: the
    evaluator's ground-truth tables (coco_evaluation._GroundTruthTables).
    -> {ar, recalls (T), thresholds (T), gt_overlaps (sorted ascending, the valid ground truths of the images that count), num_pos}.

      - An image with no proposal, or with no non-crowd ground truth, adds nothing. That includes num_pos, since the reference skips
        the image before it counts.
      - Otherwise rank the proposals by logit, descending. Equal logits keep row order, so the sort is stable.
      - The valid ground truths are those with lo <= area <= hi in fp32, both ends inclusive. An area of exactly 1024 is therefore
        both small and medium. num_pos grows by their number.
      - The live proposals are the first min(proposals, limit) ranks. The area filter comes before the limit, as in the reference.
      - Then run min(live proposals, valid ground truths) rounds. Among live pairs take the largest IoU (pairwise_iou, fp32). Ties go
        to the lowest ground-truth index in annotation order, then to the lowest rank. This is what `overlaps.max(dim=0)` followed
        by `max_overlaps.max(dim=0)` give on the CPU with current torch. Record that IoU at the chosen ground truth, then retire that
        ground truth and that proposal. A zero IoU is a legitimate choice. Ground truths never chosen keep 0.
      - hits[t] is the number of valid ground truths with gt_overlap >= thresholds[t], compared in fp32; recalls and ar: `finish`."""
    if area not in AREA_RANGES:
        raise ValueError(f"evaluate_box_proposals: unknown area range {area!r}, one of {tuple(AREA_RANGES)}")
    thresholds = default_thresholds() if thresholds is None else thresholds
    kept = []
    for rec in records:
        gb, ga = image_ground_truth(tables, rec["image_id"])
        ov = match_image(torch.as_tensor(rec["boxes"]), torch.as_tensor(rec["objectness_logits"]), torch.from_numpy(gb), torch.from_numpy(ga),
                         AREA_RANGES[area], limit)
        if ov is not None:
            kept.append(ov[ov >= 0])
    gt_overlaps = torch.sort(torch.cat(kept))[0] if kept else torch.zeros(0, dtype=torch.float32)
    hits = torch.stack([(gt_overlaps >= t).sum() for t in thresholds]) if len(thresholds) else torch.zeros(0, dtype=torch.int64)
    out = finish(hits, len(gt_overlaps), thresholds)
    out["gt_overlaps"] = gt_overlaps
    return out


def proposal_sums(records: Sequence[dict], tables, areas: Sequence[str], limits: Sequence[int], thresholds: torch.Tensor):
    """The specification's integer sums over `records` -> (hits (A, L, T) int64, num_pos (A) int64) numpy."""
    hits = np.zeros((len(areas), len(limits), len(thresholds)), dtype=np.int64)
    num_pos = np.zeros(len(areas), dtype=np.int64)
    for a, area in enumerate(areas):
        for l, limit in enumerate(limits):
            res = evaluate_box_proposals(records, tables, area, limit, thresholds)
            hits[a, l] = (res["gt_overlaps"][None, :] >= thresholds[:, None]).sum(dim=1).numpy()
            num_pos[a] = res["num_pos"]
    return hits, num_pos


class ProposalRecall:
    """The "proposals" half of an evaluator: process() per batch, state() once (this rank's sums, one device copy), results() on
    the gathered states."""

    def __init__(self, tables, areas: Sequence[str] = tuple(REPORTED_AREAS), limits: Sequence[int] = REPORTED_LIMITS):
        self.tables, self.areas, self.limits = tables, tuple(areas), tuple(int(v) for v in limits)
        self.thresholds = default_thresholds()
        self.area_ranges = area_range_tensor(self.areas)
        self.reset()

    def reset(self) -> None:
        self._cpu_records: List[dict] = []
        self._dev_sums = None        # (hits (A, L, T) int64, num_pos (A) int64) on the device
        self._dev_kept: List[tuple] = []  # per device batch (image ids, boxes, logits, counts): what the pickle needs
        self.seen = False

    def process(self, inputs: Sequence[dict], outputs: Sequence[dict], keep: bool = False) -> None:
        """outputs carry "proposals": Instances with proposal_boxes and objectness_logits. keep: also hold the proposals themselves
        (an evaluator with an output_dir writes them out)."""
        props = [o["proposals"] for o in outputs]
        if not props:
            return
        self.seen = True
        ids = [i["image_id"] for i in inputs]
        if props[0].proposal_boxes.tensor.is_cuda:
            self._process_device(ids, props, keep)
            return
        for img, p in zip(ids, props):
            self._cpu_records.append({"image_id": img, "boxes": p.proposal_boxes.tensor.detach().to(torch.float32).numpy(),
                                      "objectness_logits": p.objectness_logits.detach().to(torch.float32).numpy()})

    def _process_device(self, image_ids, props, keep: bool) -> None:
        from . import ops
        L = ops._lib
        dev = props[0].proposal_boxes.tensor.device
        n, lens = len(props), [len(p) for p in props]
        cap = max(max(lens), 1)
        if cap > L.PROPOSAL_MAX_CAP:
            raise ValueError(f"proposal recall: {cap} proposals in one image, osr_proposal_recall takes at most {L.PROPOSAL_MAX_CAP}")
        gts = [image_ground_truth(self.tables, img) for img in image_ids]
        per_image = [len(a) for _, a in gts]
        if max(per_image) > L.PROPOSAL_MAX_GT:
            raise ValueError(f"proposal recall: {max(per_image)} ground truths in one image, osr_proposal_recall takes at most {L.PROPOSAL_MAX_GT}")
        boxes = torch.zeros((n, cap, 4), dtype=torch.float32, device=dev)
        logits = torch.zeros((n, cap), dtype=torch.float32, device=dev)
        for i, p in enumerate(props):
            if lens[i]:
                boxes[i, :lens[i]], logits[i, :lens[i]] = p.proposal_boxes.tensor.to(torch.float32), p.objectness_logits.to(torch.float32)
        # the batch's tables, one buffer, one copy
        seg_off = np.concatenate(([0], np.cumsum(per_image))).astype(np.int32)
        gt_boxes, gt_area, d_seg, d_counts = upload_sections(
            [np.concatenate([b for b, _ in gts]).reshape(-1, 4), np.concatenate([a for _, a in gts]), seg_off, np.asarray(lens, dtype=np.int32)], dev)
        hits, num_pos, _ = ops.proposal_recall(boxes, logits, d_counts, gt_boxes, gt_area, d_seg, max(per_image), self.area_ranges, self.limits,
                                               self.thresholds)
        sums = (hits.sum(dim=0, dtype=torch.int64), num_pos.sum(dim=0, dtype=torch.int64))
        self._dev_sums = sums if self._dev_sums is None else (self._dev_sums[0] + sums[0], self._dev_sums[1] + sums[1])
        if keep:
            self._dev_kept.append((list(image_ids), boxes, logits, lens))

    def state(self, keep: bool = False) -> dict:
        """This rank's share as host data: the integer sums (device batches: ONE copy; CPU records: the specification) and, with
        keep, the proposals per image."""
        shape = (len(self.areas), len(self.limits), len(self.thresholds))
        hits, num_pos = np.zeros(shape, dtype=np.int64), np.zeros(shape[0], dtype=np.int64)
        if self._dev_sums is not None:
            host = torch.cat((self._dev_sums[0].reshape(-1), self._dev_sums[1])).cpu().numpy()  # the one copy
            hits += host[:hits.size].reshape(shape)
            num_pos += host[hits.size:]
        if self._cpu_records:
            h, p = proposal_sums(self._cpu_records, self.tables, self.areas, self.limits, self.thresholds)
            hits += h
            num_pos += p
        records = []
        if keep:
            for ids, boxes, logits, lens in self._dev_kept:
                b, s = boxes.cpu().numpy(), logits.cpu().numpy()
                records += [{"image_id": img, "boxes": b[i, :lens[i]].copy(), "objectness_logits": s[i, :lens[i]].copy()} for i, img in enumerate(ids)]
            records += self._cpu_records
        return {"seen": self.seen, "hits": hits, "num_pos": num_pos, "records": records}

    def results(self, states: Sequence[dict]) -> Optional[Dict[str, float]]:
        """The gathered ranks' states -> {"AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", ...} x 100; None when no rank saw a
        proposal."""
        if not any(s["seen"] for s in states):
            return None
        hits, num_pos = sum(s["hits"] for s in states), sum(s["num_pos"] for s in states)
        res = {}
        for l, limit in enumerate(self.limits):
            for a, area in enumerate(self.areas):
                stats = finish(torch.from_numpy(hits[a, l]), int(num_pos[a]), self.thresholds)
                res[f"AR{REPORTED_AREAS.get(area, area)}@{limit:d}"] = float(stats["ar"].item() * 100)
        return res

    @staticmethod
    def write(states: Sequence[dict], output_dir: str) -> None:
        """<output_dir>/box_proposals.pkl: {"boxes", "objectness_logits", "ids", "bbox_mode": 0}, numpy arrays per image."""
        recs = [r for s in states for r in s["records"]]
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, PROPOSALS_FILE), "wb") as f:
            pickle.dump({"boxes": [np.asarray(r["boxes"], dtype=np.float32).reshape(-1, 4) for r in recs],
                         "objectness_logits": [np.asarray(r["objectness_logits"], dtype=np.float32).reshape(-1) for r in recs],
                         "ids": [r["image_id"] for r in recs], "bbox_mode": BBOX_MODE_XYXY_ABS}, f)
