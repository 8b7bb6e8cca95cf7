"""LVIS federated box AP: [d2] LVISEvaluator on lvis-api's LVISResults / LVISEval, with the per-image matching on the device.

Neither lvis-api nor detectron2 is at hand: both halves are written from memory of lvis-api 0.5.x (results.py, eval.py) and detectron2
v0.6 (lvis_evaluation.py), and the rules are spelled out in include/osr.h (osr_lvis_match) and in `LVISEval` below.

  * `LVISEval` is the specification in numpy: the per-image cut across categories, the category filter, evaluate_img as the literal
    sequential loop (coco_evaluation.greedy_match with no crowd), accumulate and the nine figures. It scores CPU predictions,
    `evaluate(resume=True)` and is what the tests hold the kernel against.
  * `LVISEvaluator.process` on device `Instances` pads the batch into the engines' list form, uploads the batch's sparse tables (the
    evaluated (image, category) entries and their ground truths) in ONE copy and calls ops.lvis_match once; flags, ranks and the
    detections stay in device buffers. `evaluate` fetches them with ONE copy and accumulates from the flags: per category one stable
    argsort of -score over the image-ordered listed detections, then cumulative sums over the thresholds. Both paths end in
    coco_evaluation.precision_recall and `lvis_figures`, so they return equal dicts.

Not built: `segm`, LVIS proposal AR (outputs that carry only "proposals"), a device accumulate."""
from __future__ import annotations

import json
import logging
import os
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import parallel
from .coco_evaluation import detection_records, greedy_match, precision_recall
from .datasets import MetadataCatalog
from .eval_buffers import fetch_chunks, upload_sections
from .os_coco_evaluation import box_iou_xywh

logger = logging.getLogger(__name__)

LVIS_METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"]
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]  # all, small, medium, large
MAX_DETS = 300


def lvis_figures(precision: Optional[np.ndarray], frequency: Sequence[str]) -> Dict[str, float]:
    """LVISEval.summarize + [d2] _derive_lvis_results: precision (T, R, K, A) with -1 where a category has no ground truth -> the nine
    figures x100; the mean over the entries > -1, NaN where there is none (a frequency group without a category as well)."""
    if precision is None:
        return {m: float("nan") for m in LVIS_METRICS}

    def summ(iou=None, area=0, freq=None):
        s = precision
        if iou is not None:
            s = s[np.where(iou == IOU_THRS)[0]]
        if freq is not None:
            s = s[:, :, [k for k, f in enumerate(frequency) if f == freq]]
        s = s[:, :, :, area]
        return float(np.mean(s[s > -1]) * 100) if len(s[s > -1]) else float("nan")

    return dict(AP=summ(), AP50=summ(.5), AP75=summ(.75), APs=summ(area=1), APm=summ(area=2), APl=summ(area=3), APr=summ(freq="r"), APc=summ(freq="c"),
                APf=summ(freq="f"))


class LVISEval:
    """lvis-api's LVISResults + LVISEval for iou_type "bbox" on plain dicts. gt_dataset: the LVIS JSON (images with neg_category_ids and
    not_exhaustive_category_ids, categories with frequency, annotations with bbox xywh and area); detections: the results records
    {image_id, category_id, score, bbox xywh}. Images are ALL those of the JSON (an image without a detection still contributes its
    ground truths) unless img_ids narrows them."""

    def __init__(self, gt_dataset: dict, detections: Sequence[dict], img_ids: Optional[Sequence] = None, max_dets: int = MAX_DETS):
        self.max_dets = int(max_dets)
        self.iou_thrs, self.rec_thrs, self.area_rng = IOU_THRS, REC_THRS, AREA_RNG
        self.img_ids = sorted(set(img_ids)) if img_ids is not None else sorted({im["id"] for im in gt_dataset["images"]})
        cats = sorted(gt_dataset["categories"], key=lambda c: c["id"])
        self.cat_ids = [c["id"] for c in cats]
        self.frequency = [c.get("frequency") for c in cats]
        imgs, cat_set = set(self.img_ids), set(self.cat_ids)
        # LVISResults: ids from 1, area = w * h, then each image keeps its max_dets best over ALL categories (stable: the earlier row)
        by_img = defaultdict(list)
        for i, d in enumerate(detections):
            d = dict(d)
            d["area"], d["id"] = d["bbox"][2] * d["bbox"][3], i + 1
            by_img[d["image_id"]].append(d)
        if self.max_dets >= 0:
            by_img = {k: sorted(v, key=lambda d: d["score"], reverse=True)[: self.max_dets] for k, v in by_img.items()}
        # _prepare
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        self.img_nl = {im["id"]: set(im.get("neg_category_ids", [])) for im in gt_dataset["images"]}
        self.img_nel = {im["id"]: set(im.get("not_exhaustive_category_ids", [])) for im in gt_dataset["images"]}
        img_pl = defaultdict(set)
        for a in gt_dataset["annotations"]:
            if a["image_id"] in imgs and a["category_id"] in cat_set:
                g = dict(a)
                g["ignore"] = int(g.get("ignore", 0))
                self._gts[a["image_id"], a["category_id"]].append(g)
                img_pl[a["image_id"]].add(a["category_id"])
        for img, kept in by_img.items():
            for d in kept:
                c = d["category_id"]
                if img in imgs and c in cat_set and (c in img_pl[img] or c in self.img_nl.get(img, ())):
                    self._dts[img, c].append(d)
        self.ious: dict = {}
        self.eval_imgs: Dict[tuple, dict] = {}  # (image id, category id, area range index) -> the per-image result
        self.eval: dict = {}

    # ---- per image ----------------------------------------------------------------------------------------
    def evaluate_img(self, img_id, cat_id, a_rng) -> Optional[dict]:
        gt, dt = self._gts[img_id, cat_id], self._dts[img_id, cat_id]
        if len(gt) == 0 and len(dt) == 0:
            return None
        g_ig = np.array([1 if (g["ignore"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt], dtype=np.int64)
        gtind = np.argsort(g_ig, kind="mergesort")  # ignored ground truths last, stably
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")  # (already the order of the cut)
        dt = [dt[i] for i in dtind]
        g_ig = g_ig[gtind] if len(gt) else g_ig
        ious = self.ious[img_id, cat_id]
        ious = ious[:, gtind] if ious.size else np.zeros((len(dt), len(gt)))
        T, D = len(self.iou_thrs), len(dt)
        dtm, _ = greedy_match(ious, g_ig, [0] * len(gt), self.iou_thrs)  # no crowds: a matched ground truth is never available again
        matched = dtm >= 0
        dt_ig = np.zeros((T, D), dtype=bool)
        dt_ig[matched] = g_ig[dtm[matched]] == 1
        not_exhaustive = cat_id in self.img_nel.get(img_id, ())
        mask = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] or not_exhaustive for d in dt], dtype=bool).reshape(1, D)
        dt_ig = np.logical_or(dt_ig, np.logical_and(~matched, np.repeat(mask, T, 0)))
        dt_gt = np.where(matched, gtind[np.maximum(dtm, 0)] if len(gt) else -1, -1)  # back to the JSON's order within the group
        return dict(image_id=img_id, category_id=cat_id, dt_ids=[d["id"] for d in dt], dt_matched=matched, dt_gt=dt_gt,
                    dt_scores=[d["score"] for d in dt], gt_ignore=g_ig, dt_ignore=dt_ig)

    def evaluate(self) -> None:
        for (img, cat) in set(self._gts) | set(self._dts):
            gt, dt = self._gts[img, cat], self._dts[img, cat]
            self.ious[img, cat] = box_iou_xywh([d["bbox"] for d in dt], [g["bbox"] for g in gt], [0] * len(gt)) if gt and dt else np.zeros((0, 0))
            for a, rng in enumerate(self.area_rng):
                e = self.evaluate_img(img, cat, rng)
                if e is not None:
                    self.eval_imgs[img, cat, a] = e

    # ---- accumulation -------------------------------------------------------------------------------------
    def accumulate(self) -> None:
        T, R, K, A = len(self.iou_thrs), len(self.rec_thrs), len(self.cat_ids), len(self.area_rng)
        precision, recall = -np.ones((T, R, K, A)), -np.ones((T, K, A))
        by_cat = defaultdict(list)
        for (img, cat, a) in self.eval_imgs:
            by_cat[cat, a].append(img)
        for k, cat in enumerate(self.cat_ids):
            for a in range(A):
                E = [self.eval_imgs[img, cat, a] for img in sorted(by_cat.get((cat, a), []))]  # ascending image id
                if len(E) == 0:
                    continue
                num_gt = int(np.count_nonzero(np.concatenate([e["gt_ignore"] for e in E]) == 0))
                if num_gt == 0:
                    continue
                sc = np.concatenate([np.asarray(e["dt_scores"], dtype=np.float64) for e in E])
                inds = np.argsort(-sc, kind="mergesort")
                dtm = np.concatenate([e["dt_matched"] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e["dt_ignore"] for e in E], axis=1)[:, inds]
                tps, fps = np.logical_and(dtm, np.logical_not(dtig)), np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                precision[:, :, k, a], recall[:, k, a], _ = precision_recall(sc[inds], tps, fps, num_gt, self.rec_thrs)
        self.eval = dict(precision=precision, recall=recall)

    def results(self) -> Dict[str, float]:
        return lvis_figures(self.eval["precision"], self.frequency)


class _LVISTables:
    """The JSON as flat arrays: the annotations sorted by (image, category) in annotation order, and per image its evaluated
    (image, category) entries in ascending category: what osr_lvis_match reads."""

    def __init__(self, gt: dict):
        self.img_ids = sorted({im["id"] for im in gt["images"]})
        cats = sorted(gt["categories"], key=lambda c: c["id"])
        self.cat_ids = [c["id"] for c in cats]
        self.frequency = [c.get("frequency") for c in cats]
        self.img_pos = {v: i for i, v in enumerate(self.img_ids)}
        cat_pos = {v: i for i, v in enumerate(self.cat_ids)}
        K, I = len(self.cat_ids), len(self.img_ids)
        anns = [a for a in gt["annotations"] if a["image_id"] in self.img_pos and a["category_id"] in cat_pos]
        key = np.array([self.img_pos[a["image_id"]] * K + cat_pos[a["category_id"]] for a in anns], dtype=np.int64)
        order = np.argsort(key, kind="mergesort")
        anns = [anns[i] for i in order]
        self.key = key[order]
        self.box = np.array([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
        self.area = np.array([a["area"] for a in anns], dtype=np.float64)
        self.flags = np.array([2 if a.get("ignore", 0) else 0 for a in anns], dtype=np.uint8)  # bit 1 = ignore
        self.gt_start = np.searchsorted(self.key, np.arange(I + 1) * K, side="left")  # an image's annotations
        neg = [self.img_pos[im["id"]] * K + cat_pos[c] for im in gt["images"] for c in im.get("neg_category_ids", []) if c in cat_pos]
        nex = [self.img_pos[im["id"]] * K + cat_pos[c] for im in gt["images"] for c in im.get("not_exhaustive_category_ids", []) if c in cat_pos]
        ent = np.unique(np.concatenate([self.key, np.array(neg, dtype=np.int64)]))  # positive or negative, ascending (image, category)
        self.ent_cat = (ent % K).astype(np.int32)
        self.ent_count = (np.searchsorted(self.key, ent, side="right") - np.searchsorted(self.key, ent, side="left")).astype(np.int64)
        self.ent_flags = np.isin(ent, np.array(nex, dtype=np.int64)).astype(np.uint8)  # bit 0 = not exhaustive
        self.ent_start = np.searchsorted(ent, np.arange(I + 1) * K, side="left")  # an image's entries

    def batch(self, image_ids: Sequence):
        """-> (gt rows: indices into box / area / flags; entries: indices into ent_*; img_off (n + 1); ev_gt_off (NE + 1); the largest
        group). An image the JSON does not hold owns no entry."""
        rows, ents, img_off = [], [], [0]
        for img in image_ids:
            pos = self.img_pos.get(img)
            if pos is not None:
                rows.append(np.arange(self.gt_start[pos], self.gt_start[pos + 1]))
                ents.append(np.arange(self.ent_start[pos], self.ent_start[pos + 1]))
            img_off.append(img_off[-1] + (len(ents[-1]) if pos is not None else 0))
        rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        ents = np.concatenate(ents) if ents else np.zeros(0, dtype=np.int64)
        per = self.ent_count[ents]
        return rows, ents, np.asarray(img_off, dtype=np.int32), np.concatenate(([0], np.cumsum(per))).astype(np.int32), int(per.max()) if per.size else 0

    def num_gt(self, img_ids: Optional[Sequence] = None) -> np.ndarray:
        """(K, A): the ground truths that are not ignored, over the images that count."""
        K = len(self.cat_ids)
        keep = np.ones(len(self.key), dtype=bool)
        if img_ids is not None:
            chosen = np.zeros(len(self.img_ids), dtype=bool)
            chosen[[self.img_pos[i] for i in img_ids if i in self.img_pos]] = True
            keep = chosen[self.key // K]
        out = np.zeros((K, len(AREA_RNG)), dtype=np.int64)
        for a, (lo, hi) in enumerate(AREA_RNG):
            ok = keep & ~((self.flags != 0) | (self.area < lo) | (self.area > hi))
            out[:, a] = np.bincount(self.key[ok] % K, minlength=K)
        return out


class LVISEvaluator:
    """[d2] LVISEvaluator for the task "bbox". `tasks`: a tuple of task names, None (bbox) or a config node (bbox; with MODEL.MASK_ON
    one warning that `segm` is not built). Asking for "segm" by name raises, and so do outputs that carry only "proposals".

    evaluate() returns {"bbox": {AP, AP50, AP75, APs, APm, APl, APr, APc, APf}}, x100, NaN where LVISEval says -1, and writes
    detectron2's lvis_instances_results.json into output_dir: every detection, dataset category ids."""

    RESULTS_FILE = "lvis_instances_results.json"

    def __init__(self, dataset_name: str, tasks=None, output_dir: Optional[str] = None, max_dets_per_image: Optional[int] = None):
        meta = MetadataCatalog.get(dataset_name)
        self.dataset_name, self.output_dir = dataset_name, output_dir
        if tasks is not None and hasattr(tasks, "MODEL"):  # a config node
            if tasks.MODEL.MASK_ON:
                logger.warning("LVISEvaluator(%s): MODEL.MASK_ON is set but the task 'segm' is not built (no polygon rasterisation / RLE); scoring bbox",
                               dataset_name)
            tasks = ("bbox",)
        for t in tasks or ():
            if t != "bbox":
                raise NotImplementedError(f"LVISEvaluator: the task '{t}' is not built (bbox is; segm needs polygon rasterisation and RLE)")
        self.tasks = ("bbox",)
        self.max_dets = MAX_DETS if max_dets_per_image is None else int(max_dets_per_image)
        with open(meta.json_file) as f:
            self.gt = json.load(f)
        self.tables = _LVISTables(self.gt)
        id_map = getattr(meta, "thing_dataset_id_to_contiguous_id", None) or {c: i for i, c in enumerate(self.tables.cat_ids)}
        self.reverse_id_map = {v: k for k, v in id_map.items()}
        self.reset()

    def reset(self) -> None:
        self._cpu_records: List[dict] = []
        self._chunks: List[dict] = []   # per device batch: tensors that stay on the device
        self._image_ids: List = []      # of the device batches, in order

    # ---- process ------------------------------------------------------------------------------------------
    def process(self, inputs: Sequence[dict], outputs: Sequence[dict]) -> None:
        if outputs and "instances" not in outputs[0]:
            raise NotImplementedError("LVISEvaluator: outputs without 'instances' (LVIS proposal AR) are not built")
        insts = [o["instances"] for o in outputs]
        if not insts:
            return
        if insts[0].pred_boxes.tensor.is_cuda:
            self._process_device([i["image_id"] for i in inputs], insts)
            return
        for inp, inst in zip(inputs, insts):
            self._cpu_records += detection_records(inp["image_id"], inst.pred_boxes.tensor.detach().float().numpy(), inst.scores.detach().float().numpy(),
                                                   inst.pred_classes.detach().numpy(), None, self.reverse_id_map)

    def _process_device(self, image_ids, insts) -> None:
        from . import ops
        L = ops._lib
        dev = insts[0].pred_boxes.tensor.device
        n, lens = len(insts), [len(i) for i in insts]
        cap = max(max(lens), 1)
        if cap > L.LVIS_MAX_CAP:
            raise ValueError(f"LVISEvaluator: {cap} detections in one image, osr_lvis_match takes at most {L.LVIS_MAX_CAP}")
        if not 1 <= self.max_dets <= L.LVIS_MAX_DET:
            raise ValueError(f"LVISEvaluator: max_dets_per_image {self.max_dets}, osr_lvis_match takes 1 .. {L.LVIS_MAX_DET}")
        boxes = torch.zeros((n, cap, 4), dtype=torch.float32, device=dev)
        scores = torch.zeros((n, cap), dtype=torch.float32, device=dev)
        classes = torch.full((n, cap), -1, dtype=torch.int64, device=dev)
        for i, inst in enumerate(insts):
            m = lens[i]
            if m:
                boxes[i, :m], scores[i, :m], classes[i, :m] = inst.pred_boxes.tensor.to(torch.float32), inst.scores.to(torch.float32), inst.pred_classes.to(torch.int64)
        tb = self.tables
        rows, ents, img_off, ev_gt_off, max_group = tb.batch(image_ids)
        if max_group > L.LVIS_MAX_GROUP:
            raise ValueError(f"LVISEvaluator: {max_group} ground truths of one category in one image, osr_lvis_match takes at most {L.LVIS_MAX_GROUP}")
        gt_box, gt_area, d_img_off, d_cat, d_gt_off, d_counts, gt_flags, d_ev_flags = upload_sections(  # one buffer, one copy
            [tb.box[rows], tb.area[rows], img_off, tb.ent_cat[ents], ev_gt_off, np.asarray(lens, dtype=np.int32), tb.flags[rows], tb.ent_flags[ents]], dev)
        flags, rank, _, _ = ops.lvis_match(boxes, scores, classes, d_counts, len(tb.cat_ids), d_img_off, d_cat, d_gt_off, d_ev_flags, gt_box, gt_area, gt_flags,
                                           max_group, IOU_THRS, AREA_RNG, self.max_dets)
        self._chunks.append(dict(n=n, cap=cap, boxes=boxes, scores=scores, classes=classes, counts=d_counts, flags=flags, rank=rank))
        self._image_ids += list(image_ids)

    # ---- evaluate -----------------------------------------------------------------------------------------
    def _fetch(self) -> Optional[dict]:
        """Every device buffer in ONE copy -> flat host arrays over the rows that exist, in processing order."""
        if not self._chunks:
            return None
        fields = [("boxes", np.float32), ("scores", np.float32), ("classes", np.int64), ("counts", np.int32), ("flags", np.uint32), ("rank", np.int32)]
        out, img0 = defaultdict(list), 0
        for c, got in zip(self._chunks, fetch_chunks(self._chunks, fields)):
            n, cap = c["n"], c["cap"]
            exists = (np.arange(cap)[None, :] < got["counts"][:, None]).reshape(-1)
            out["image"].append(np.repeat(np.arange(img0, img0 + n), cap)[exists])
            out["boxes"].append(got["boxes"].reshape(-1, 4)[exists])
            out["flags"].append(got["flags"].reshape(n * cap, -1)[exists])
            for f in ("scores", "classes", "rank"):
                out[f].append(got[f][exists])
            img0 += n
        res = {k: np.concatenate(v) for k, v in out.items()}
        res["image_ids"] = list(self._image_ids)
        return res

    def _records_from(self, part: dict) -> List[dict]:
        ids = part["image_ids"]
        recs = detection_records(None, part["boxes"], part["scores"], part["classes"], None, self.reverse_id_map)
        for r, i in zip(recs, part["image"]):
            r["image_id"] = ids[i]
        return recs

    def _accumulate_from_flags(self, parts: Sequence[dict], img_ids: Optional[Sequence]) -> np.ndarray:
        """LVISEval.accumulate from the kernel's flags: -> precision (T, R, K, A)."""
        tb = self.tables
        T, R, K, A = len(IOU_THRS), len(REC_THRS), len(tb.cat_ids), len(AREA_RNG)
        precision = -np.ones((T, R, K, A))
        chosen = set(img_ids) if img_ids is not None else None
        pos = np.concatenate([np.array([tb.img_pos.get(i, -1) if chosen is None or i in chosen else -1 for i in q["image_ids"]], dtype=np.int64)[q["image"]]
                              for q in parts])
        cls, rank = np.concatenate([q["classes"] for q in parts]), np.concatenate([q["rank"] for q in parts])
        score, flags = np.concatenate([q["scores"] for q in parts]).astype(np.float64), np.concatenate([q["flags"] for q in parts])
        num_gt = tb.num_gt(img_ids)
        sel = np.nonzero((rank >= 0) & (pos >= 0))[0]
        sel = sel[np.lexsort((rank[sel], pos[sel], cls[sel]))]  # by category; image order, each group in list order: what LVISEval concatenates
        bounds = np.searchsorted(cls[sel], np.arange(K + 1), side="left")
        shifts = np.arange(T, dtype=np.uint32)[:, None]
        for k in np.nonzero(num_gt.any(axis=1))[0]:
            sub = sel[bounds[k]:bounds[k + 1]]
            sub = sub[np.argsort(-score[sub], kind="mergesort")]
            for a in range(A):
                if num_gt[k, a] == 0:
                    continue
                w = flags[sub, a][None, :]
                matched, ignored = ((w >> shifts) & 1).astype(bool), ((w >> (shifts + 16)) & 1).astype(bool)
                precision[:, :, k, a], _, _ = precision_recall(score[sub], matched & ~ignored, ~matched & ~ignored, int(num_gt[k, a]), REC_THRS)
        return precision

    def _score_records(self, records: Sequence[dict], img_ids) -> dict:
        if not records:
            return {"bbox": lvis_figures(None, self.tables.frequency)}
        ev = LVISEval(self.gt, records, img_ids, self.max_dets)
        ev.evaluate()
        ev.accumulate()
        return {"bbox": ev.results()}

    def evaluate(self, img_ids=None, resume: bool = False) -> Optional[dict]:
        """Rank 0 gathers every rank's detections and flags, writes the detections to <output_dir>/lvis_instances_results.json and
        scores them; `resume=True` scores that file through the numpy LVISEval instead and returns the same figures."""
        if resume:
            if self.output_dir is None:
                raise ValueError("resume=True needs output_dir (where a previous run wrote its detections)")
            if parallel.world_info()[0] != 0:
                return None
            with open(os.path.join(self.output_dir, self.RESULTS_FILE)) as f:
                return self._score_records(json.load(f), img_ids)
        gathered = parallel.gather_to_rank0({"device": self._fetch(), "cpu": self._cpu_records})
        if gathered is None:
            return None
        parts = [g["device"] for g in gathered if g["device"] is not None]
        records = [r for q in parts for r in self._records_from(q)] + [r for g in gathered for r in g["cpu"]]
        if self.output_dir:
            os.makedirs(self.output_dir, exist_ok=True)
            with open(os.path.join(self.output_dir, self.RESULTS_FILE), "w") as f:
                json.dump(records, f)
        if not parts or any(g["cpu"] for g in gathered):  # CPU predictions: everything through the numpy specification
            return self._score_records(records, img_ids)
        return {"bbox": lvis_figures(self._accumulate_from_flags(parts, img_ids), self.tables.frequency)}
