"""COCO box and keypoint AP: [d2] COCOEvaluator on pycocotools' COCOeval, with the per-image matching on the device.

Neither pycocotools nor detectron2 is at hand: both halves are written from memory of pycocotools 2.0 (cocoeval.py) and detectron2
v0.6 (coco_evaluation.py), and the rules are spelled out in include/osr.h (osr_coco_match) and in `COCOeval` below.

  * `COCOeval` is the specification in numpy: computeIoU / computeOks, evaluateImg as the literal sequential loop, accumulate and
    summarize. It scores CPU predictions, `evaluate(resume=True)` and is what the tests hold the kernel against.
  * `COCOEvaluator.process` on device `Instances` pads the batch into the engines' list form with torch ops, uploads the batch's
    ground-truth tables in ONE copy and calls ops.coco_match once per task; flags, ranks and the detections stay in device buffers
    and nothing is copied back. `evaluate` fetches them with ONE copy, gathers on rank 0 (host.parallel) and accumulates from the
    flags with vectorised numpy: per category one stable argsort of -score over the image-ordered detections with rank < maxDets,
    then cumulative sums over the thresholds. Both paths end in the same `precision_recall`, so they return equal figures.

Outputs that carry "proposals" (a ProposalNetwork's) are scored by host/proposal_evaluation.py: class-agnostic AR@100 / AR@1000 per
area range, matched on the device by ops.proposal_recall, reported as "box_proposals" ahead of the tasks.

LVIS names are scored by host/lvis_evaluation.py (federated box AP, matched on the device by ops.lvis_match).

Not built: `segm` (polygon rasterisation and RLE), a device accumulate."""
from __future__ import annotations

import json
import logging
import os
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import parallel
from .datasets import MetadataCatalog
from .os_coco_evaluation import box_iou_xywh
from .eval_buffers import fetch_chunks, upload_sections
from .proposal_evaluation import ProposalRecall

logger = logging.getLogger(__name__)

# pycocotools' Params.kpt_oks_sigmas for the 17 COCO person keypoints
COCO_KEYPOINT_OKS_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
RESULT_METRICS = {"bbox": ["AP", "AP50", "AP75", "APs", "APm", "APl"], "keypoints": ["AP", "AP50", "AP75", "APm", "APl"]}
SUPPORTED_TASKS = ("bbox", "keypoints")


class Params:
    """pycocotools' Params for iouType "bbox" / "keypoints"."""

    def __init__(self, iou_type: str = "bbox", max_dets: Optional[Sequence[int]] = None):
        if iou_type not in SUPPORTED_TASKS:
            raise NotImplementedError(f"COCOeval: iou_type {iou_type!r} is not built (bbox and keypoints are; segm needs polygon rasterisation and RLE)")
        self.iou_type = iou_type
        self.iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        if iou_type == "bbox":
            self.max_dets = [1, 10, 100]
            self.area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
            self.area_lbl = ["all", "small", "medium", "large"]
        else:
            self.max_dets = [20]
            self.area_rng = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
            self.area_lbl = ["all", "medium", "large"]
        if max_dets is not None:
            self.max_dets = [int(m) for m in max_dets]


def keypoint_oks(d_kpts: np.ndarray, g_kpts: np.ndarray, g_bbox: np.ndarray, g_area: np.ndarray, sigmas: np.ndarray) -> np.ndarray:
    """COCOeval.computeOks: detections (D, 3 Kp) x ground truths (G, 3 Kp) -> (D, G). A ground truth with visible points is compared
    at those; one without compares every point against its box doubled on each side."""
    d_kpts, g_kpts = np.asarray(d_kpts, dtype=np.float64).reshape(len(d_kpts), -1), np.asarray(g_kpts, dtype=np.float64).reshape(len(g_kpts), -1)
    out = np.zeros((len(d_kpts), len(g_kpts)))
    vars_ = (np.asarray(sigmas, dtype=np.float64) * 2) ** 2
    k = len(vars_)
    for j in range(len(g_kpts)):
        xg, yg, vg = g_kpts[j, 0::3], g_kpts[j, 1::3], g_kpts[j, 2::3]
        k1 = np.count_nonzero(vg > 0)
        bb = g_bbox[j]
        x0, x1, y0, y1 = bb[0] - bb[2], bb[0] + bb[2] * 2, bb[1] - bb[3], bb[1] + bb[3] * 2
        for i in range(len(d_kpts)):
            xd, yd = d_kpts[i, 0::3], d_kpts[i, 1::3]
            if k1 > 0:
                dx, dy = xd - xg, yd - yg
            else:
                z = np.zeros(k)
                dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
            e = (dx ** 2 + dy ** 2) / vars_ / (g_area[j] + np.spacing(1)) / 2
            if k1 > 0:
                e = e[vg > 0]
            out[i, j] = np.sum(np.exp(-e)) / e.shape[0]
    return out


def greedy_match(ious: np.ndarray, gt_ignore: Sequence[int], gt_crowd: Sequence[int], iou_thrs: Sequence[float]):
    """COCOeval.evaluateImg's loops, literally: detections in list order, ground truths sorted ignored-last by the caller.
    -> (dtm (T, D): the matched ground truth's column or -1, gtm (T, G): the matching detection's row or -1)."""
    T, D, G = len(iou_thrs), ious.shape[0], ious.shape[1]
    dtm, gtm = -np.ones((T, D), dtype=np.int64), -np.ones((T, G), dtype=np.int64)
    for tind, t in enumerate(iou_thrs):
        for dind in range(D):
            iou = min([t, 1 - 1e-10])  # the best similarity so far
            m = -1
            for gind in range(G):
                if gtm[tind, gind] >= 0 and not gt_crowd[gind]:  # taken, and not a crowd
                    continue
                if m > -1 and gt_ignore[m] == 0 and gt_ignore[gind] == 1:  # a regular match stands: stop at the first ignored one
                    break
                if ious[dind, gind] < iou:
                    continue
                iou = ious[dind, gind]
                m = gind
            if m == -1:
                continue
            dtm[tind, dind] = m
            gtm[tind, m] = dind
    return dtm, gtm


def precision_recall(scores_sorted: np.ndarray, tps: np.ndarray, fps: np.ndarray, npig: int, rec_thrs: np.ndarray):
    """COCOeval.accumulate's inner block for one (category, area range, maxDets): tps / fps (T, N) bool over the detections sorted by
    descending score -> (precision (T, R), recall (T), scores (T, R)). The precision envelope is the running maximum from the right;
    the recall thresholds are looked up with searchsorted(side="left") and stay 0 beyond the last detection."""
    T, R, nd = tps.shape[0], len(rec_thrs), tps.shape[1]
    tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(np.float64), np.cumsum(fps, axis=1).astype(np.float64)
    precision, recall, scores = np.zeros((T, R)), np.zeros(T), np.zeros((T, R))
    for t in range(T):
        tp, fp = tp_sum[t], fp_sum[t]
        rc = tp / npig
        pr = tp / (fp + tp + np.spacing(1))
        recall[t] = rc[-1] if nd else 0
        pr = np.maximum.accumulate(pr[::-1])[::-1]
        inds = np.searchsorted(rc, rec_thrs, side="left")
        ok = inds < nd
        precision[t, ok] = pr[inds[ok]]
        scores[t, ok] = scores_sorted[inds[ok]]
    return precision, recall, scores


def summarize_stats(precision: np.ndarray, recall: np.ndarray, p: Params) -> np.ndarray:
    """COCOeval.summarize: 12 figures for bbox, 10 for keypoints; the mean over the entries > -1, -1 when there is none."""
    def summ(ap, iou=None, area="all", max_det=100):
        s = precision if ap else recall
        if iou is not None:
            s = s[np.where(iou == p.iou_thrs)[0]]
        s = s[..., p.area_lbl.index(area), p.max_dets.index(max_det)]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    md = p.max_dets
    if p.iou_type == "bbox":
        last = md[2]
        return np.array([summ(1, max_det=last), summ(1, .5, max_det=last), summ(1, .75, max_det=last), summ(1, area="small", max_det=last),
                         summ(1, area="medium", max_det=last), summ(1, area="large", max_det=last), summ(0, max_det=md[0]), summ(0, max_det=md[1]),
                         summ(0, max_det=last), summ(0, area="small", max_det=last), summ(0, area="medium", max_det=last), summ(0, area="large", max_det=last)])
    last = md[-1]
    return np.array([summ(1, max_det=last), summ(1, .5, max_det=last), summ(1, .75, max_det=last), summ(1, area="medium", max_det=last),
                     summ(1, area="large", max_det=last), summ(0, max_det=last), summ(0, .5, max_det=last), summ(0, .75, max_det=last),
                     summ(0, area="medium", max_det=last), summ(0, area="large", max_det=last)])


def prepare_ground_truth(ann: dict, iou_type: str) -> dict:
    """COCOeval._prepare for one annotation: iscrowd defaults to 0, area to w * h; ignore = iscrowd, for keypoints also a ground
    truth without a labelled point."""
    g = dict(ann)
    g["iscrowd"] = int(g.get("iscrowd", 0))
    if "area" not in g:
        g["area"] = g["bbox"][2] * g["bbox"][3]
    g["ignore"] = g["iscrowd"]
    if iou_type == "keypoints":
        g["ignore"] = int(g["iscrowd"] or g.get("num_keypoints", 0) == 0)
    return g


class COCOeval:
    """pycocotools' COCOeval for iouType "bbox" and "keypoints" on plain dicts. gt_dataset: the COCO JSON; detections: the results
    records ({image_id, category_id, score, bbox xywh} or {.., keypoints}). Images and categories are ALL those of the JSON (an
    image without a detection still contributes its ground truths) unless img_ids narrows the images."""

    def __init__(self, gt_dataset: dict, detections: Sequence[dict], iou_type: str = "bbox", img_ids: Optional[Sequence] = None,
                 kpt_oks_sigmas: Optional[Sequence[float]] = None, max_dets: Optional[Sequence[int]] = None):
        self.params = p = Params(iou_type, max_dets)
        self.sigmas = np.asarray(kpt_oks_sigmas if kpt_oks_sigmas is not None and len(kpt_oks_sigmas) else COCO_KEYPOINT_OKS_SIGMAS, dtype=np.float64)
        self.img_ids = sorted(set(img_ids)) if img_ids is not None else sorted({im["id"] for im in gt_dataset["images"]})
        self.cat_ids = sorted(c["id"] for c in gt_dataset["categories"])
        imgs, cats = set(self.img_ids), set(self.cat_ids)
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for a in gt_dataset["annotations"]:
            if a["image_id"] in imgs and a["category_id"] in cats:
                self._gts[a["image_id"], a["category_id"]].append(prepare_ground_truth(a, iou_type))
        for i, d in enumerate(detections):  # COCO.loadRes: id = running index from 1, iscrowd = 0, the area from the box / the points' extent
            if iou_type == "keypoints" and "keypoints" not in d:
                continue
            d = dict(d)
            if iou_type == "bbox":
                d["area"] = d["bbox"][2] * d["bbox"][3]
            else:
                x, y = d["keypoints"][0::3], d["keypoints"][1::3]
                x0, x1, y0, y1 = np.min(x), np.max(x), np.min(y), np.max(y)
                d["area"] = float((x1 - x0) * (y1 - y0))
                d["bbox"] = [x0, y0, x1 - x0, y1 - y0]
            d["id"], d["iscrowd"] = i + 1, 0
            if d["image_id"] in imgs and d["category_id"] in cats:
                self._dts[d["image_id"], d["category_id"]].append(d)
        self.ious: dict = {}
        self.eval_imgs: List[Optional[dict]] = []
        self.eval: dict = {}
        self.stats: Optional[np.ndarray] = None

    # ---- per image ----------------------------------------------------------------------------------------
    def compute_similarity(self, img_id, cat_id) -> np.ndarray:
        """computeIoU / computeOks: (the detections by descending score, stable, at most maxDets[-1]) x (the ground truths in the
        JSON's order)."""
        gt, dt = self._gts[img_id, cat_id], self._dts[img_id, cat_id]
        if len(gt) == 0 or len(dt) == 0:
            return np.zeros((0, 0))
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in inds[: self.params.max_dets[-1]]]
        if self.params.iou_type == "bbox":
            return box_iou_xywh([d["bbox"] for d in dt], [g["bbox"] for g in gt], [g["iscrowd"] for g in gt])
        kp = len(self.sigmas) * 3
        return keypoint_oks(np.array([d["keypoints"] for d in dt]), np.array([g.get("keypoints", [0] * kp) for g in gt]), np.array([g["bbox"] for g in gt]),
                            np.array([g["area"] for g in gt]), self.sigmas)

    def evaluate_img(self, img_id, cat_id, a_rng, max_det) -> Optional[dict]:
        p = self.params
        gt, dt = self._gts[img_id, cat_id], self._dts[img_id, cat_id]
        if len(gt) == 0 and len(dt) == 0:
            return None
        g_ig = np.array([1 if (g["ignore"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt], dtype=np.int64)
        gtind = np.argsort(g_ig, kind="mergesort")  # ignored ground truths last, stably
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")[:max_det]
        dt = [dt[i] for i in dtind]
        g_ig = g_ig[gtind] if len(gt) else g_ig
        crowd = [gt[i]["iscrowd"] for i in gtind]
        ious = self.ious[img_id, cat_id]
        ious = ious[:, gtind] if ious.size else np.zeros((len(dt), len(gt)))
        T, D = len(p.iou_thrs), len(dt)
        dtm, gtm = greedy_match(ious[:D], g_ig, crowd, p.iou_thrs)
        matched = dtm >= 0
        dt_ig = np.zeros((T, D), dtype=bool)
        dt_ig[matched] = g_ig[dtm[matched]] == 1
        out_of_range = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt], dtype=bool).reshape(1, D)
        dt_ig = np.logical_or(dt_ig, np.logical_and(~matched, np.repeat(out_of_range, T, 0)))
        dt_gt = np.where(matched, gtind[np.maximum(dtm, 0)] if len(gt) else -1, -1)  # back to the JSON's order within the group
        return dict(image_id=img_id, category_id=cat_id, a_rng=a_rng, max_det=max_det, dt_ids=[d["id"] for d in dt], dt_matched=matched, dt_gt=dt_gt,
                    dt_scores=[d["score"] for d in dt], gt_ignore=g_ig, dt_ignore=dt_ig)

    def evaluate(self) -> None:
        p = self.params
        self.ious = {(i, c): self.compute_similarity(i, c) for i in self.img_ids for c in self.cat_ids}
        max_det = p.max_dets[-1]
        self.eval_imgs = [self.evaluate_img(i, c, a, max_det) for c in self.cat_ids for a in p.area_rng for i in self.img_ids]

    # ---- accumulation -------------------------------------------------------------------------------------
    def accumulate(self) -> None:
        p = self.params
        T, R, K, A, M = len(p.iou_thrs), len(p.rec_thrs), len(self.cat_ids), len(p.area_rng), len(p.max_dets)
        precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
        I = len(self.img_ids)
        for k in range(K):
            for a in range(A):
                E = [e for e in self.eval_imgs[(k * A + a) * I:(k * A + a + 1) * I] if e is not None]
                if len(E) == 0:
                    continue
                npig = int(np.count_nonzero(np.concatenate([e["gt_ignore"] for e in E]) == 0))
                if npig == 0:
                    continue
                for m, max_det in enumerate(p.max_dets):
                    sc = np.concatenate([np.asarray(e["dt_scores"][:max_det], dtype=np.float64) for e in E])
                    inds = np.argsort(-sc, kind="mergesort")
                    dtm = np.concatenate([e["dt_matched"][:, :max_det] for e in E], axis=1)[:, inds]
                    dtig = np.concatenate([e["dt_ignore"][:, :max_det] for e in E], axis=1)[:, inds]
                    tps, fps = np.logical_and(dtm, np.logical_not(dtig)), np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                    precision[:, :, k, a, m], recall[:, k, a, m], scores[:, :, k, a, m] = precision_recall(sc[inds], tps, fps, npig, p.rec_thrs)
        self.eval = dict(precision=precision, recall=recall, scores=scores)

    def summarize(self) -> np.ndarray:
        self.stats = summarize_stats(self.eval["precision"], self.eval["recall"], self.params)
        return self.stats


def derive_coco_results(stats: Optional[np.ndarray], precision: Optional[np.ndarray], iou_type: str, class_names: Sequence[str]) -> Dict[str, float]:
    """[d2] COCOEvaluator._derive_coco_results: the first figures x100 with NaN for -1; for bbox with more than one class also
    "AP-<name>", the mean of precision[:, :, k, all, last maxDets] over its entries > -1."""
    metrics = RESULT_METRICS[iou_type]
    if stats is None:
        return {m: float("nan") for m in metrics}
    res = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(metrics)}
    if iou_type != "bbox" or class_names is None or len(class_names) <= 1:
        return res
    for k, name in enumerate(class_names):
        pr = precision[:, :, k, 0, -1]
        pr = pr[pr > -1]
        res["AP-" + name] = float(np.mean(pr) * 100) if pr.size else float("nan")
    return res


def detection_records(image_id, boxes: np.ndarray, scores: np.ndarray, classes: np.ndarray, keypoints: Optional[np.ndarray], reverse_id_map: Dict[int, int]) -> List[dict]:
    """[d2] instances_to_coco_json: fp32 xyxy -> xywh with the differences taken in fp32, contiguous class -> dataset id, keypoints
    with x and y shifted by -0.5 in fp32 (COCO's keypoint coordinates are pixel indices)."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    xywh = np.stack([boxes[:, 0], boxes[:, 1], boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]], axis=1).astype(np.float64).tolist()
    kp = None
    if keypoints is not None:
        k = np.array(keypoints, dtype=np.float32)
        k = k.reshape(len(boxes), max(k.size // max(3 * len(boxes), 1), 1), 3)
        k[:, :, :2] -= np.float32(0.5)
        kp = k.astype(np.float64).reshape(len(boxes), 3 * k.shape[1]).tolist()
    classes, scores = np.asarray(classes).tolist(), np.asarray(scores, dtype=np.float32).astype(np.float64).tolist()
    out = []
    for r in range(len(boxes)):
        c = int(classes[r])
        if c not in reverse_id_map:
            raise ValueError(f"COCOEvaluator: a prediction has class {c}, the dataset has contiguous ids 0 .. {len(reverse_id_map) - 1}")
        rec = dict(image_id=image_id, category_id=reverse_id_map[c], bbox=xywh[r], score=scores[r])
        if kp is not None:
            rec["keypoints"] = kp[r]
        out.append(rec)
    return out


def tasks_from_config(cfg) -> tuple:
    """[d2] COCOEvaluator._tasks_from_config."""
    tasks = ("bbox",)
    if cfg.MODEL.MASK_ON:
        tasks += ("segm",)
    if cfg.MODEL.KEYPOINT_ON:
        tasks += ("keypoints",)
    return tasks


class _GroundTruthTables:
    """The JSON's annotations as flat arrays sorted by (image, category) in annotation order: what osr_coco_match reads."""

    def __init__(self, gt: dict):
        self.img_ids = sorted({im["id"] for im in gt["images"]})
        self.cat_ids = sorted(c["id"] for c in gt["categories"])
        self.img_pos = {v: i for i, v in enumerate(self.img_ids)}
        cat_pos = {v: i for i, v in enumerate(self.cat_ids)}
        anns = [a for a in gt["annotations"] if a["image_id"] in self.img_pos and a["category_id"] in cat_pos]
        K = len(self.cat_ids)
        key = np.array([self.img_pos[a["image_id"]] * K + cat_pos[a["category_id"]] for a in anns], dtype=np.int64)
        order = np.argsort(key, kind="mergesort")
        anns = [anns[i] for i in order]
        self.key = key[order]
        self.json_pos = order  # where the annotation stands in the JSON: an image's annotation order (proposal recall reads it)
        self.box = np.array([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
        self.area = np.array([a["area"] if "area" in a else a["bbox"][2] * a["bbox"][3] for a in anns], dtype=np.float64)
        crowd = np.array([int(a.get("iscrowd", 0)) for a in anns], dtype=np.uint8)
        self.crowd = crowd
        nokp = np.array([a.get("num_keypoints", 0) == 0 for a in anns], dtype=bool)
        self.flags = {"bbox": (crowd | (crowd << 1)).astype(np.uint8), "keypoints": (crowd | ((crowd.astype(bool) | nokp).astype(np.uint8) << 1)).astype(np.uint8)}
        self.ann_ids = [a.get("id") for a in anns]
        self.num_kpts = max([len(a["keypoints"]) // 3 for a in anns if "keypoints" in a], default=0)
        kp = self.num_kpts
        self.kpts = np.array([a["keypoints"] if "keypoints" in a else [0] * (3 * kp) for a in anns], dtype=np.float64).reshape(-1, kp, 3) if kp else None
        self.start = np.searchsorted(self.key, np.arange(len(self.img_ids) + 1) * K, side="left")  # an image's annotations: start[i] .. start[i + 1]

    def batch(self, image_ids: Sequence):
        """-> (rows: indices into the flat arrays, image by image; seg_off (n * K + 1) int32; the largest group)."""
        K = len(self.cat_ids)
        rows, keys = [], []
        for i, img in enumerate(image_ids):
            pos = self.img_pos.get(img)
            if pos is None:
                continue
            r = np.arange(self.start[pos], self.start[pos + 1])
            rows.append(r)
            keys.append(self.key[r] - pos * K + i * K)
        rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        per_group = np.bincount(np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64), minlength=len(image_ids) * K)
        seg_off = np.concatenate(([0], np.cumsum(per_group))).astype(np.int32)
        return rows, seg_off, int(per_group.max()) if per_group.size else 0

    def npig(self, task: str, area_rng, img_ids: Optional[Sequence] = None) -> np.ndarray:
        """(K, A): the ground truths that are not ignored, over the images that count."""
        K = len(self.cat_ids)
        keep = np.ones(len(self.key), dtype=bool)
        if img_ids is not None:
            chosen = np.zeros(len(self.img_ids), dtype=bool)
            chosen[[self.img_pos[i] for i in img_ids if i in self.img_pos]] = True
            keep = chosen[self.key // K]
        ign = (self.flags[task] & 2) != 0
        out = np.zeros((K, len(area_rng)), dtype=np.int64)
        for a, (lo, hi) in enumerate(area_rng):
            ok = keep & ~(ign | (self.area < lo) | (self.area > hi))
            out[:, a] = np.bincount(self.key[ok] % K, minlength=K)
        return out


class COCOEvaluator:
    """[d2] COCOEvaluator for the tasks "bbox" and "keypoints". `tasks`: a tuple of task names, None (taken from what the first
    predictions carry: bbox, and keypoints when they have pred_keypoints) or a config node (bbox, keypoints with MODEL.KEYPOINT_ON;
    with MODEL.MASK_ON one warning that `segm` is not built, and the rest is scored). Asking for "segm" by name raises.

    Outputs with "proposals" (with or without "instances") add "box_proposals": {AR@100, ARs@100, ARm@100, ARl@100, AR@1000, ...}, first
    in the result, and <output_dir>/box_proposals.pkl.

    evaluate() returns {"bbox": {AP, AP50, AP75, APs, APm, APl, "AP-<name>" per class when there are several}, "keypoints": {AP, AP50,
    AP75, APm, APl}}, x100, NaN where COCOeval says -1, and writes detectron2's coco_instances_results.json into output_dir."""

    RESULTS_FILE = "coco_instances_results.json"

    def __init__(self, dataset_name: str, tasks=None, output_dir: Optional[str] = None, max_dets_per_image: Optional[int] = None,
                 kpt_oks_sigmas: Sequence[float] = ()):
        meta = MetadataCatalog.get(dataset_name)
        self.dataset_name, self.output_dir = dataset_name, output_dir
        sigmas = kpt_oks_sigmas
        if tasks is not None and hasattr(tasks, "MODEL"):  # a config node, as detectron2 still accepts
            cfg = tasks
            tasks = tasks_from_config(cfg)
            if "segm" in tasks:
                logger.warning("COCOEvaluator(%s): MODEL.MASK_ON is set but the task 'segm' is not built (no polygon rasterisation / RLE); scoring %s",
                               dataset_name, ", ".join(t for t in tasks if t != "segm"))
                tasks = tuple(t for t in tasks if t != "segm")
            if not len(sigmas):
                sigmas = cfg.TEST.KEYPOINT_OKS_SIGMAS
        if tasks is not None:
            for t in tasks:
                if t not in SUPPORTED_TASKS:
                    raise NotImplementedError(f"COCOEvaluator: the task '{t}' is not built (bbox and keypoints are; segm needs polygon rasterisation and RLE)")
        self.tasks = tuple(tasks) if tasks is not None else None
        self.kpt_oks_sigmas = [float(s) for s in sigmas]
        self.max_dets = {"bbox": [1, 10, 100] if max_dets_per_image is None else [1, 10, int(max_dets_per_image)], "keypoints": [20]}
        with open(meta.json_file) as f:
            self.gt = json.load(f)
        self.tables = _GroundTruthTables(self.gt)
        cats = sorted(self.gt["categories"], key=lambda c: c["id"])
        self.class_names = [c["name"] for c in cats]
        id_map = getattr(meta, "thing_dataset_id_to_contiguous_id", None) or {c["id"]: i for i, c in enumerate(cats)}
        self.reverse_id_map = {v: k for k, v in id_map.items()}
        self.proposals = ProposalRecall(self.tables)
        self.reset()

    def reset(self) -> None:
        self.proposals.reset()
        self._saw_instances = False
        self._cpu_records: List[dict] = []
        self._chunks: List[dict] = []      # per device batch: tensors that stay on the device
        self._image_ids: List = []         # of the device batches, in order

    # ---- process ------------------------------------------------------------------------------------------
    def _tasks_for(self, has_keypoints: bool) -> tuple:
        if self.tasks is None:
            self.tasks = ("bbox", "keypoints") if has_keypoints else ("bbox",)
        return self.tasks

    def sigmas_for(self, num_keypoints: int) -> np.ndarray:
        if len(self.kpt_oks_sigmas):
            if len(self.kpt_oks_sigmas) != num_keypoints:
                raise ValueError(f"COCOEvaluator: TEST.KEYPOINT_OKS_SIGMAS has {len(self.kpt_oks_sigmas)} entries, the predictions {num_keypoints} keypoints")
            return np.asarray(self.kpt_oks_sigmas, dtype=np.float64)
        if num_keypoints == 17:
            return COCO_KEYPOINT_OKS_SIGMAS
        raise ValueError(f"COCOEvaluator: {num_keypoints} keypoints and no TEST.KEYPOINT_OKS_SIGMAS (only the 17 COCO keypoints have built-in sigmas)")

    def process(self, inputs: Sequence[dict], outputs: Sequence[dict]) -> None:
        if outputs and "proposals" in outputs[0]:
            self.proposals.process(inputs, outputs, keep=self.output_dir is not None)
            if "instances" not in outputs[0]:
                return
        insts = [o["instances"] for o in outputs]
        if not insts:
            return
        self._saw_instances = True
        has_kp = insts[0].has("pred_keypoints")
        tasks = self._tasks_for(has_kp)
        if "keypoints" in tasks:
            if not has_kp:
                raise ValueError("COCOEvaluator: the task 'keypoints' needs predictions with pred_keypoints")
            self.sigmas_for(int(insts[0].pred_keypoints.shape[1]))
        if insts[0].pred_boxes.tensor.is_cuda:
            self._process_device([i["image_id"] for i in inputs], insts, tasks)
            return
        for inp, inst in zip(inputs, insts):
            kp = inst.pred_keypoints.detach().float().numpy() if "keypoints" in tasks else None
            self._cpu_records += detection_records(inp["image_id"], inst.pred_boxes.tensor.detach().float().numpy(), inst.scores.detach().float().numpy(),
                                                   inst.pred_classes.detach().numpy(), kp, self.reverse_id_map)

    def _process_device(self, image_ids, insts, tasks) -> None:
        from . import ops
        dev = insts[0].pred_boxes.tensor.device
        n, K = len(insts), len(self.tables.cat_ids)
        lens = [len(i) for i in insts]
        cap = max(max(lens), 1)
        if cap > ops._lib.COCO_MAX_CAP:
            raise ValueError(f"COCOEvaluator: {cap} detections in one image, osr_coco_match takes at most {ops._lib.COCO_MAX_CAP}")
        kp_task = "keypoints" in tasks
        kpn = int(insts[0].pred_keypoints.shape[1]) if kp_task else 0
        boxes = torch.zeros((n, cap, 4), dtype=torch.float32, device=dev)
        scores = torch.zeros((n, cap), dtype=torch.float32, device=dev)
        classes = torch.full((n, cap), -1, dtype=torch.int64, device=dev)
        kpts = torch.zeros((n, cap, kpn, 3), dtype=torch.float32, device=dev) if kp_task else None
        for i, inst in enumerate(insts):
            m = lens[i]
            if m:
                boxes[i, :m], scores[i, :m], classes[i, :m] = inst.pred_boxes.tensor.to(torch.float32), inst.scores.to(torch.float32), inst.pred_classes.to(torch.int64)
                if kp_task:
                    kpts[i, :m] = inst.pred_keypoints.to(torch.float32)
        # the batch's tables, one buffer, one copy
        tb = self.tables
        rows, seg_off, max_group = tb.batch(image_ids)
        if max_group > ops._lib.COCO_MAX_GROUP:
            raise ValueError(f"COCOEvaluator: {max_group} ground truths of one category in one image, osr_coco_match takes at most {ops._lib.COCO_MAX_GROUP}")
        ng = len(rows)
        if kp_task and ng and tb.num_kpts != kpn:
            raise ValueError(f"COCOEvaluator: the predictions have {kpn} keypoints, the ground truth of {self.dataset_name} {tb.num_kpts}")
        sections = [tb.box[rows], tb.area[rows], np.asarray(seg_off, dtype=np.int32), np.asarray(lens, dtype=np.int32)]  # (the tables are float64 / uint8)
        if kp_task:
            sections += [tb.kpts[rows] if ng else np.zeros((0, kpn, 3)), self.sigmas_for(kpn)]
        views = upload_sections(sections + [tb.flags[t][rows] for t in tasks], dev)
        gt_box, gt_area, d_seg, d_counts = views[:4]
        gt_kpts, sig = views[4:6] if kp_task else (None, None)
        gt_flags = views[len(sections):]
        chunk = dict(n=n, cap=cap, kpn=kpn, boxes=boxes, scores=scores, classes=classes, counts=d_counts, kpts=kpts)
        for ti, task in enumerate(tasks):
            p = Params(task, self.max_dets[task])
            flags, rank, _, _ = ops.coco_match(boxes, scores, classes, d_counts, K, d_seg, gt_box, gt_area, gt_flags[ti], max_group, p.iou_thrs,
                                               p.area_rng, p.max_dets[-1], keypoints=kpts if task == "keypoints" else None,
                                               gt_kpts=gt_kpts if task == "keypoints" else None, sigmas=sig if task == "keypoints" else None)
            chunk["flags_" + task], chunk["rank_" + task] = flags, rank
        self._chunks.append(chunk)
        self._image_ids += list(image_ids)

    # ---- evaluate -----------------------------------------------------------------------------------------
    def _fetch(self) -> Optional[dict]:
        """Every device buffer in ONE copy -> flat host arrays over the rows that exist, in processing order."""
        if not self._chunks:
            return None
        fields = [("boxes", np.float32), ("scores", np.float32), ("classes", np.int64), ("counts", np.int32)] + \
                 ([("kpts", np.float32)] if self._chunks[0]["kpts"] is not None else []) + \
                 [(f + t, dt) for t in self.tasks for f, dt in (("flags_", np.uint32), ("rank_", np.int32))]
        out, img0 = defaultdict(list), 0
        for c, got in zip(self._chunks, fetch_chunks(self._chunks, fields)):
            n, cap = c["n"], c["cap"]
            exists = (np.arange(cap)[None, :] < got["counts"][:, None]).reshape(-1)
            out["image"].append(np.repeat(np.arange(img0, img0 + n), cap)[exists])
            out["boxes"].append(got["boxes"].reshape(-1, 4)[exists])
            out["scores"].append(got["scores"][exists])
            out["classes"].append(got["classes"][exists])
            if "kpts" in got:
                out["kpts"].append(got["kpts"].reshape(n * cap, c["kpn"], 3)[exists])
            for t in self.tasks:
                out["rank_" + t].append(got["rank_" + t][exists])
                out["flags_" + t].append(got["flags_" + t].reshape(n * cap, -1)[exists])
            img0 += n
        res = {k: np.concatenate(v) for k, v in out.items()}
        res["image_ids"] = list(self._image_ids)
        return res

    def _records_from(self, part: dict) -> List[dict]:
        ids = part["image_ids"]
        recs = detection_records(None, part["boxes"], part["scores"], part["classes"], part.get("kpts"), self.reverse_id_map)
        for r, i in zip(recs, part["image"]):
            r["image_id"] = ids[i]
        return recs

    def _accumulate_from_flags(self, parts: Sequence[dict], task: str, img_ids: Optional[Sequence]):
        """COCOeval.accumulate from the kernel's flags: -> (precision (T, R, K, A, M), recall (T, K, A, M))."""
        p = Params(task, self.max_dets[task])
        tb = self.tables
        T, R, K, A, M = len(p.iou_thrs), len(p.rec_thrs), len(tb.cat_ids), len(p.area_rng), len(p.max_dets)
        precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
        chosen = set(img_ids) if img_ids is not None else None
        pos = np.concatenate([np.array([tb.img_pos.get(i, -1) if chosen is None or i in chosen else -1 for i in q["image_ids"]], dtype=np.int64)[q["image"]]
                              for q in parts])
        cls, rank = np.concatenate([q["classes"] for q in parts]), np.concatenate([q["rank_" + task] for q in parts])
        score, flags = np.concatenate([q["scores"] for q in parts]).astype(np.float64), np.concatenate([q["flags_" + task] for q in parts])
        npig = tb.npig(task, p.area_rng, img_ids)
        listed = (rank >= 0) & (pos >= 0)
        shifts = np.arange(T, dtype=np.uint32)[:, None]
        for k in range(K):
            sel = np.nonzero(listed & (cls == k))[0]
            sel = sel[np.lexsort((rank[sel], pos[sel]))]  # image order, each image's list in rank order: what COCOeval concatenates
            for m, max_det in enumerate(p.max_dets):
                sub = sel[rank[sel] < max_det]
                inds = np.argsort(-score[sub], kind="mergesort")
                sub = sub[inds]
                for a in range(A):
                    if npig[k, a] == 0:
                        continue
                    w = flags[sub, a][None, :]
                    matched, ignored = ((w >> shifts) & 1).astype(bool), ((w >> (shifts + 16)) & 1).astype(bool)
                    precision[:, :, k, a, m], recall[:, k, a, m], _ = precision_recall(score[sub], matched & ~ignored, ~matched & ~ignored, int(npig[k, a]), p.rec_thrs)
        return precision, recall, p

    def _score_records(self, records: Sequence[dict], img_ids) -> dict:
        out = {}
        for task in self.tasks:
            dets = [r for r in records if task != "keypoints" or "keypoints" in r]
            if not dets:
                out[task] = derive_coco_results(None, None, task, self.class_names)
                continue
            sig = self.sigmas_for(len(dets[0]["keypoints"]) // 3) if task == "keypoints" else None
            ev = COCOeval(self.gt, dets, task, img_ids, sig, self.max_dets[task])
            ev.evaluate()
            ev.accumulate()
            out[task] = derive_coco_results(ev.summarize(), ev.eval["precision"], task, self.class_names)
        return out

    def evaluate(self, img_ids=None, resume: bool = False) -> Optional[dict]:
        """Rank 0 gathers every rank's detections and flags, writes the detections to <output_dir>/coco_instances_results.json and
        scores them; `resume=True` scores that file through the numpy COCOeval instead and returns the same figures."""
        if resume:
            if self.output_dir is None:
                raise ValueError("resume=True needs output_dir (where a previous run wrote its detections)")
            if parallel.world_info()[0] != 0:
                return None
            with open(os.path.join(self.output_dir, self.RESULTS_FILE)) as f:
                records = json.load(f)
            if self.tasks is None:
                self.tasks = ("bbox", "keypoints") if records and "keypoints" in records[0] else ("bbox",)
            return self._score_records(records, img_ids)
        gathered = parallel.gather_to_rank0({"device": self._fetch(), "cpu": self._cpu_records, "instances": self._saw_instances,
                                             "proposals": self.proposals.state(keep=self.output_dir is not None)})
        if gathered is None:
            return None
        states = [g["proposals"] for g in gathered]
        box_proposals = self.proposals.results(states)
        if box_proposals is None:
            return self._evaluate_instances(gathered, img_ids)
        if self.output_dir:
            self.proposals.write(states, self.output_dir)
        out = {"box_proposals": box_proposals}  # (first, as in the reference)
        if any(g["instances"] for g in gathered):
            out.update(self._evaluate_instances(gathered, img_ids))
        return out

    def _evaluate_instances(self, gathered, img_ids) -> dict:
        parts = [g["device"] for g in gathered if g["device"] is not None]
        records = [r for q in parts for r in self._records_from(q)] + [r for g in gathered for r in g["cpu"]]
        if self.output_dir:
            os.makedirs(self.output_dir, exist_ok=True)
            with open(os.path.join(self.output_dir, self.RESULTS_FILE), "w") as f:
                json.dump(records, f)
        if self.tasks is None or not records:
            return {t: derive_coco_results(None, None, t, self.class_names) for t in (self.tasks or ("bbox",))}
        if any(g["cpu"] for g in gathered):  # CPU predictions: everything through the numpy specification
            return self._score_records(records, img_ids)
        out = {}
        for task in self.tasks:
            precision, recall, p = self._accumulate_from_flags(parts, task, img_ids)
            out[task] = derive_coco_results(summarize_stats(precision, recall, p), precision, task, self.class_names)
        return out
