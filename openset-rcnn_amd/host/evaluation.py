"""Open-set PASCAL-VOC evaluator -- the `mAP_k` half of the headline metric.

Own numpy implementation of the protocol in /root/reference/openset_rcnn/evaluation/pascal_voc_evaluation.py:
  * process (:53-70): per detection one text record "image score xmin ymin xmax ymax" with xmin/ymin + 1 (the inverse of
    the VOC loader's -1), score rounded to 3 decimals and coordinates to 1 decimal BEFORE scoring -- kept, because the
    rounding changes ranks and overlaps;
  * per class (:130-163, voc_eval :264-379): GT of the class from the XML annotations with every category outside the
    known set renamed "unknown"; detections sorted by descending confidence; greedy matching at IoU > 0.5 with the
    inclusive "+1" pixel box convention (:247-261); "difficult" GT neither counts nor penalises; a second match of the same
    GT is a false positive; precision/recall curves; VOC-2012 style AP (area under the monotone precision envelope,
    `_is_2007 = False` :41);
  * open-set extras: A-OSE = known-class detections that overlap an unknown GT at IoU > 0.5 (:350-377), WI = wilderness
    impact at recall 0.8 (:72-100): mean over known classes of open-set false positives / mean of closed-set TP+FP, each
    taken at the detection whose recall is closest to 0.8;
  * summary keys (:165-215): mAP (over ALL class names, empty classes count as 0), WI (x100), AOSE, AP@K / P@K / R@K over the
    known classes, AP@U / P@U / R@U for the last class ("unknown"), rounded to 2 decimals.
Multi-process runs gather the per-rank records on rank 0 ([d2] comm.gather :106) through host.parallel.

Tie order: like the reference, detections are ordered with np.argsort(-confidence) (not a stable sort); with scores rounded
to 3 decimals ties exist, and their order may differ between numpy builds. AP@K moves by < 0.01 in practice.

Device path. Device predictions (fp32 boxes and scores) are matched on the device by osr_voc_match (include/osr.h, which restates
the rules above without the text; csrc/osr_voc_eval.hip): `process` pads the batch into the engines' list form, launches the kernel
once and keeps everything in device buffers: no copy to the host and no synchronisation. `evaluate` fetches all of it in ONE copy
and builds the per-class curves from the flag bytes (`accumulate_from_flags`); the text records (`_predictions`, the <class>.txt
files) are rebuilt from the fetched fp32 arrays with the same format string. `voc_match_reference` is the kernel's specification as
a numpy loop. The device path's tie order is DEFINED: descending rounded score, then arrival order (chunk, image row, detection
row; ranks in rank order), i.e. `voc_eval(..., kind="stable")`. numpy's default argsort may order ties differently, which moves
AP@K by < 0.01 as said above. The whole evaluation falls back to the numpy path on the rebuilt records, with one warning that
names the reason, when CPU and device input were mixed, boxes or scores are not fp32, an image_id is missing from the annotations
or was processed twice, a list is longer than 1024, an image has more than 4096 ground truths, the last class name is not
"unknown" (or a name occurs twice), or the kernel reports a non-finite score or coordinate."""
from __future__ import annotations

import logging
import os
import xml.etree.ElementTree as ET
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import parallel

logger = logging.getLogger(__name__)

UNKNOWN_NAME = "unknown"
VOC_VALID, VOC_TP, VOC_FP, VOC_UNK, VOC_NONFINITE = 1, 2, 4, 8, 16  # osr_voc_match's flag bits (include/osr.h)


def voc_ap(rec: np.ndarray, prec: np.ndarray, use_07_metric: bool = False) -> float:
    """[d2] detectron2.evaluation.pascal_voc_evaluation.voc_ap: 11-point average (VOC07) or the exact area under the
    precision envelope (VOC10+)."""
    rec, prec = np.asarray(rec, dtype=np.float64), np.asarray(prec, dtype=np.float64)
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            p = float(np.max(prec[rec >= t])) if np.sum(rec >= t) > 0 else 0.0
            ap += p / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]  # envelope: running max from the right
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def parse_voc_xml(path: str, known_classes: Sequence[str]) -> List[dict]:
    """Objects of one annotation file; categories outside `known_classes` become "unknown" (:230-232)."""
    known = set(known_classes)
    out = []
    for obj in ET.parse(path).findall("object"):
        name = obj.find("name").text
        bb = obj.find("bndbox")
        out.append(dict(name=name if name in known else UNKNOWN_NAME, difficult=int(obj.find("difficult").text),
                        bbox=[int(bb.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")]))
    return out


def _overlaps(gt: np.ndarray, bb: np.ndarray) -> np.ndarray:
    """IoU of one detection against (G,4) GT boxes with the inclusive-pixel (+1) convention (:247-261)."""
    iw = np.maximum(np.minimum(gt[:, 2], bb[2]) - np.maximum(gt[:, 0], bb[0]) + 1.0, 0.0)
    ih = np.maximum(np.minimum(gt[:, 3], bb[3]) - np.maximum(gt[:, 1], bb[1]) + 1.0, 0.0)
    inter = iw * ih
    union = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (gt[:, 2] - gt[:, 0] + 1.0) * (gt[:, 3] - gt[:, 1] + 1.0) - inter
    return inter / union


def _class_gt(annos: Dict[str, List[dict]], image_ids: Sequence[str], name: str):
    per_image, npos = {}, 0
    for im in image_ids:
        objs = [o for o in annos[im] if o["name"] == name]
        bbox = np.array([o["bbox"] for o in objs], dtype=np.float64).reshape(-1, 4)
        difficult = np.array([o["difficult"] for o in objs], dtype=bool)
        npos += int(np.sum(~difficult))
        per_image[im] = (bbox, difficult, np.zeros(len(objs), dtype=bool))
    return per_image, npos


def _curves(tp: np.ndarray, fp: np.ndarray, is_unk: Optional[np.ndarray], npos: int, n_unk: int, classname: str, use_07_metric: bool):
    """voc_eval's second half: the per-detection 0/1 sequences in list order -> its return value."""
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    with np.errstate(divide="ignore", invalid="ignore"):
        rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    ap = voc_ap(rec, prec, use_07_metric)
    if classname == UNKNOWN_NAME:
        return rec, prec, ap, 0, n_unk, None, None
    return rec, prec, ap, float(np.sum(is_unk)), n_unk, tp + fp, np.cumsum(is_unk)


def voc_eval(records: Sequence[str], annos: Dict[str, List[dict]], image_ids: Sequence[str], classname: str, ovthresh: float = 0.5,
             use_07_metric: bool = False, kind: Optional[str] = None):
    """One class (:264-379). records: "image score xmin ymin xmax ymax" strings. Returns (rec, prec, ap, unknown dets taken
    as this class, number of unknown GT, closed-set TP+FP curve, open-set FP curve); the last two are None for "unknown".
    kind: np.argsort's; None is the reference's order, "stable" the one the device path defines (ties in arrival order)."""
    gt, npos = _class_gt(annos, image_ids, classname)
    rows = [r.strip().split(" ") for r in records if r.strip()]
    det_images = [r[0] for r in rows]
    conf = np.array([float(r[1]) for r in rows], dtype=np.float64)
    bb = np.array([[float(z) for z in r[2:]] for r in rows], dtype=np.float64).reshape(-1, 4)
    order = np.argsort(-conf, kind=kind)
    bb = bb[order]
    det_images = [det_images[i] for i in order]
    nd = len(det_images)
    tp, fp = np.zeros(nd), np.zeros(nd)
    for d in range(nd):
        boxes, difficult, taken = gt[det_images[d]]
        ovmax, jmax = -np.inf, -1
        if boxes.size:
            ov = _overlaps(boxes, bb[d])
            jmax = int(np.argmax(ov))
            ovmax = ov[jmax]
        if ovmax > ovthresh:
            if not difficult[jmax]:
                if not taken[jmax]:
                    tp[d] = 1.0
                    taken[jmax] = True
                else:
                    fp[d] = 1.0
        else:
            fp[d] = 1.0
    unk, n_unk = _class_gt(annos, image_ids, UNKNOWN_NAME)
    is_unk = None
    if classname != UNKNOWN_NAME:
        is_unk = np.zeros(nd)
        for d in range(nd):
            boxes = unk[det_images[d]][0]
            if boxes.size and np.max(_overlaps(boxes, bb[d])) > ovthresh:
                is_unk[d] = 1.0
    return _curves(tp, fp, is_unk, npos, n_unk, classname, use_07_metric)


def voc_record_numbers(boxes: np.ndarray, scores: np.ndarray):
    """The numbers a text record holds, without the text (include/osr.h osr_voc_match, "record geometry"): boxes (N, 4) fp32 xyxy,
    scores (N) fp32 -> (t (N, 4) float64 = rint(v * 10) of (x0 + 1, y0 + 1, x1, y1) with the + 1 in fp32, k (N) float64 = rint(s * 1000),
    finite (N) bool). t / 10 == float(f"{v:.1f}") and k / 1000 == float(f"{s:.3f}") exactly: the products are exact in float64, rint
    rounds half to even as the formatting does, and the division is correctly rounded as float("...") is."""
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        b[:, :2] = b[:, :2] + np.float32(1.0)
        t = np.rint(b.astype(np.float64) * 10.0)
        k = np.rint(s.astype(np.float64) * 1000.0)
        finite = np.isfinite(b).all(axis=1) & np.isfinite(s) & (np.abs(k) < 2.0 ** 31) & (np.abs(t) < 2.0 ** 63).all(axis=1)
    return t, k, finite


def voc_match_reference(boxes: np.ndarray, scores: np.ndarray, classes: np.ndarray, counts: np.ndarray, image_index: np.ndarray, num_classes: int,
                        gt_img_off: np.ndarray, gt_box: np.ndarray, gt_cls: np.ndarray, gt_difficult: np.ndarray, ovthresh: float = 0.5):
    """osr_voc_match's CPU specification (include/osr.h states the rules): one batch of padded lists against the dataset's ground-truth
    table, as a plain loop. -> (flags (n, cap) uint8, milli (n, cap) int32, match (n, cap) int32, deci (n, cap, 4) int64, status (1)
    int32), the kernel's outputs."""
    boxes = np.asarray(boxes, dtype=np.float32)
    n, cap = boxes.shape[0], boxes.shape[1]
    scores, classes = np.asarray(scores, dtype=np.float32).reshape(n, cap), np.asarray(classes, dtype=np.int64).reshape(n, cap)
    gt_box, gt_cls, gt_difficult = np.asarray(gt_box, dtype=np.float64).reshape(-1, 4), np.asarray(gt_cls), np.asarray(gt_difficult)
    flags, milli = np.zeros((n, cap), dtype=np.uint8), np.zeros((n, cap), dtype=np.int32)
    match, deci, status = np.full((n, cap), -1, dtype=np.int32), np.zeros((n, cap, 4), dtype=np.int64), np.zeros(1, dtype=np.int32)
    C, num_images = int(num_classes), len(gt_img_off) - 1
    t, k, finite = voc_record_numbers(boxes.reshape(-1, 4), scores.reshape(-1))
    t, k, finite = t.reshape(n, cap, 4), k.reshape(n, cap), finite.reshape(n, cap)
    for i in range(n):
        img = int(image_index[i])
        if not 0 <= img < num_images:
            continue
        g0, g1 = int(gt_img_off[img]), int(gt_img_off[img + 1])
        lists: Dict[int, List[int]] = defaultdict(list)
        for r in range(min(max(int(counts[i]), 0), cap)):
            c = int(classes[i, r])
            if not 0 <= c < C:
                continue
            if not finite[i, r]:
                flags[i, r] = VOC_VALID | VOC_NONFINITE
                status[0] = 1
                continue
            flags[i, r], milli[i, r], deci[i, r] = VOC_VALID, int(k[i, r]), t[i, r].astype(np.int64)
            lists[c].append(r)
        unk = np.array([j for j in range(g0, g1) if gt_cls[j] == C - 1], dtype=np.int64)
        for c, rows in lists.items():
            own = np.array([j for j in range(g0, g1) if gt_cls[j] == c], dtype=np.int64)
            taken = set()
            for r in sorted(rows, key=lambda r: (-int(milli[i, r]), r)):  # descending rounded score, equal ones the lower row first
                bb = t[i, r] / 10.0
                ovmax, jmax = -np.inf, -1
                if own.size:
                    ov = _overlaps(gt_box[own], bb)
                    jmax = int(np.argmax(ov))
                    ovmax = ov[jmax]
                if ovmax > ovthresh:
                    match[i, r] = own[jmax]
                    if not gt_difficult[own[jmax]]:
                        if jmax not in taken:
                            flags[i, r] |= VOC_TP
                            taken.add(jmax)
                        else:
                            flags[i, r] |= VOC_FP
                else:
                    flags[i, r] |= VOC_FP
                if c != C - 1 and unk.size and np.max(_overlaps(gt_box[unk], bb)) > ovthresh:
                    flags[i, r] |= VOC_UNK
    return flags, milli, match, deci, status


class VocGroundTruthTable:
    """The annotations as the flat arrays osr_voc_match reads (include/osr.h): per image of `image_ids`, in annotation order, the box,
    the class index (the position of the object's name in class_names, -1 for a name that is not there) and the difficult mark."""

    def __init__(self, annos: Dict[str, List[dict]], image_ids: Sequence[str], class_names: Sequence[str]):
        cls_of = {name: i for i, name in enumerate(class_names)}
        self.index = {im: m for m, im in reversed(list(enumerate(image_ids)))}  # (a repeated id means its first position)
        off, box, cls, difficult = [0], [], [], []
        for im in image_ids:
            for o in annos[im]:
                box.append(o["bbox"])
                cls.append(cls_of.get(o["name"], -1))
                difficult.append(1 if o["difficult"] else 0)
            off.append(len(cls))
        self.img_off = np.array(off, dtype=np.int32)
        self.box = np.array(box, dtype=np.float64).reshape(-1, 4)
        self.cls = np.array(cls, dtype=np.int32)
        self.difficult = np.array(difficult, dtype=np.uint8)
        self.max_per_image = int(np.max(np.diff(self.img_off))) if len(image_ids) else 0


def wilderness_impact(recalls: List[np.ndarray], tp_plus_fp: List[Optional[np.ndarray]], fp_open: List[Optional[np.ndarray]],
                      num_known: int, recall_level: float = 0.8) -> float:
    """compute_WI_at_a_recall_level (:84-100) at one IoU threshold."""
    tpfp, fps = [], []
    for cls_id, rec in enumerate(recalls):
        if cls_id < num_known and len(rec) > 0:
            idx = int(np.argmin(np.abs(np.asarray(rec) - recall_level)))  # first closest, as min(range, key=...)
            tpfp.append(tp_plus_fp[cls_id][idx])
            fps.append(fp_open[cls_id][idx])
    return float(np.mean(fps) / np.mean(tpfp)) if tpfp else 0.0


class PascalVOCDetectionEvaluator:
    """DatasetEvaluator-shaped (reset / process / evaluate) open-set VOC evaluator (pascal_voc_evaluation.py:21-215).

    dirname holds Annotations/<id>.xml and ImageSets/Main/<split>.txt; class_names are the dataset's thing classes with
    "unknown" last (openset_rcnn/data/voc_coco.py:5-29); predicted class ids index into class_names (unknown id =
    len(class_names) - 1 = 80 under --opendet-benchmark).

    Device predictions (fp32 boxes and scores) are matched on the device: `process` pads the batch into the engines' list form and
    calls ops.voc_match once, against the dataset's ground-truth table that went up with the first device batch; detections, flags
    and rounded scores stay in device buffers. `evaluate` fetches them in ONE copy, gathers on rank 0 and accumulates from the flags
    (accumulate_from_flags, which shares its arithmetic with voc_eval); ties are in arrival order. CPU predictions go through voc_eval
    on the text records, as does everything when the device path cannot be taken (the module docstring lists when). sort_kind is
    voc_eval's `kind` for that numpy path: None, the reference's order, or "stable", the device path's."""

    def __init__(self, dirname: str, split: str, class_names: Sequence[str], num_known_classes: int, output_dir: Optional[str] = None,
                 annotations: Optional[Dict[str, List[dict]]] = None, image_ids: Optional[Sequence[str]] = None, sort_kind: Optional[str] = None):
        self._class_names = list(class_names)
        self._sort_kind = sort_kind
        self._gt_table = None   # (VocGroundTruthTable or None, why not), built with the first device batch
        self._dev_table = None  # (device, gt_box, gt_img_off, gt_cls, gt_difficult): its device copy
        self.num_known_classes = int(num_known_classes)
        self.known_classes = self._class_names[: self.num_known_classes]
        self.total_num_class = len(self._class_names)
        self.unknown_class_index = self.total_num_class - 1
        self.output_dir = output_dir
        self._is_2007 = False
        if annotations is None:
            with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt")) as f:
                image_ids = [x.strip() for x in f.readlines()]
            annotations = {im: parse_voc_xml(os.path.join(dirname, "Annotations", im + ".xml"), self.known_classes) for im in image_ids}
        self._annos = annotations
        self._image_ids = list(image_ids if image_ids is not None else annotations.keys())
        self.reset()

    def reset(self) -> None:
        self._segments: List[tuple] = []  # processing order: ("host", {class: records}) / ("device", chunk)
        self._merged: Optional[Dict[int, List[str]]] = None
        self._seen = set()                # the image ids of the device chunks
        self._host_reason: Optional[str] = None

    @property
    def _predictions(self) -> Dict[int, List[str]]:
        """{class id: text records} of this process, in processing order. Device chunks are fetched (one copy) and their records
        rebuilt on first access."""
        if self._merged is None:
            self._merged = self._records(self._host_segments())
        return self._merged

    def process(self, inputs: Sequence[dict], outputs: Sequence[dict]) -> None:
        self._merged = None
        insts = [out["instances"] for out in outputs]
        if not insts:
            return
        if insts[0].pred_boxes.tensor.is_cuda and self._host_reason is None:
            reason = self._process_device([inp["image_id"] for inp in inputs], insts)
            if reason is None:
                return
            logger.warning("PascalVOCDetectionEvaluator: device predictions take the host path and numpy scores everything (%s)", reason)
            self._host_reason = reason
        records: Dict[int, List[str]] = defaultdict(list)
        for inp, inst in zip(inputs, insts):
            boxes = inst.pred_boxes.tensor.detach().cpu().numpy()
            scores = inst.scores.detach().cpu().tolist()
            classes = inst.pred_classes.detach().cpu().tolist()
            for box, score, cls in zip(boxes, scores, classes):
                xmin, ymin, xmax, ymax = box
                records[int(cls)].append(f"{inp['image_id']} {score:.3f} {xmin + 1:.1f} {ymin + 1:.1f} {xmax:.1f} {ymax:.1f}")
        self._segments.append(("host", dict(records)))

    def _table(self):
        """(ground-truth table, None) or (None, why the device path cannot score this dataset); built with the first device batch."""
        if self._gt_table is None:
            names = self._class_names
            if not names or names[-1] != UNKNOWN_NAME or len(set(names)) != len(names):
                self._gt_table = (None, 'class names that do not end in "unknown" or repeat a name')
            else:
                tb = VocGroundTruthTable(self._annos, self._image_ids, names)
                from ._lib import VOC_MAX_GT
                self._gt_table = (tb, None) if tb.max_per_image <= VOC_MAX_GT else \
                    (None, f"{tb.max_per_image} ground truths in one image: osr_voc_match takes at most {VOC_MAX_GT}")
        return self._gt_table

    def _process_device(self, image_ids, insts) -> Optional[str]:
        """The batch through ops.voc_match; -> None, or why it has to take the host path instead. Reads pred_boxes.tensor, scores and
        pred_classes only; copies nothing to the host and does not synchronise."""
        import torch
        from . import ops
        from .eval_buffers import upload_sections
        L = ops._lib
        tb, reason = self._table()
        if tb is None:
            return reason
        parts = [(i.pred_boxes.tensor.detach(), i.scores.detach(), i.pred_classes.detach()) for i in insts]
        dev = parts[0][0].device
        if any(t.device != dev for p in parts for t in p):
            return "CPU and device input were mixed"
        if any(b.dtype != torch.float32 or s.dtype != torch.float32 for b, s, _ in parts):
            return "boxes or scores that are not float32"
        lens = [int(s.shape[0]) for _, s, _ in parts]
        if max(lens) > L.VOC_MAX_CAP:
            return f"{max(lens)} detections in one image: osr_voc_match takes at most {L.VOC_MAX_CAP}"
        index, batch_ids = [], set()
        for im in image_ids:
            if im not in tb.index:
                return f"image_id {im!r} is not in the annotations"
            if im in self._seen or im in batch_ids:
                return f"image_id {im!r} was processed twice"
            batch_ids.add(im)
            index.append(tb.index[im])
        if self._dev_table is None or self._dev_table[0] != dev:  # the dataset's table, one buffer, one copy
            self._dev_table = (dev, *upload_sections([tb.box, tb.img_off, tb.cls, tb.difficult], dev))
        _, gt_box, gt_off, gt_cls, gt_difficult = self._dev_table
        n, total = len(parts), sum(lens)
        cap = max((max(lens) + 7) // 8 * 8, 8)
        dest = np.concatenate([i * cap + np.arange(m, dtype=np.int64) for i, m in enumerate(lens)])  # where each detection goes in the padded lists
        d_dest, d_counts, d_index = upload_sections([dest, np.asarray(lens, dtype=np.int32), np.asarray(index, dtype=np.int32)], dev)
        boxes = torch.zeros((n, cap, 4), dtype=torch.float32, device=dev)
        scores = torch.zeros((n, cap), dtype=torch.float32, device=dev)
        classes = torch.full((n, cap), -1, dtype=torch.int64, device=dev)
        if total:
            boxes.view(-1, 4).index_copy_(0, d_dest, torch.cat([b.reshape(-1, 4) for b, _, _ in parts]))
            scores.view(-1).index_copy_(0, d_dest, torch.cat([s.reshape(-1) for _, s, _ in parts]))
            classes.view(-1).index_copy_(0, d_dest, torch.cat([c.reshape(-1) for _, _, c in parts]).to(torch.int64))
        flags, milli, _, _, status = ops.voc_match(boxes, scores, classes, d_counts, d_index, self.total_num_class, gt_off, gt_box, gt_cls, gt_difficult,
                                                   tb.max_per_image, 0.5)
        self._seen |= batch_ids
        self._segments.append(("device", dict(n=n, cap=cap, image_ids=list(image_ids), lens=lens, boxes=boxes, scores=scores, classes=classes, flags=flags,
                                              milli=milli, status=status)))
        return None

    _FIELDS = (("boxes", np.float32), ("scores", np.float32), ("classes", np.int64), ("flags", np.uint8), ("milli", np.int32), ("status", np.int32))

    def _host_segments(self) -> List[tuple]:
        """The segments with every device chunk replaced by flat host arrays over the rows that exist, in arrival order (image row, then
        detection row). All chunks not fetched before come over in ONE copy."""
        from .eval_buffers import fetch_chunks
        todo = [c for kind, c in self._segments if kind == "device" and "host" not in c]
        for c, got in zip(todo, fetch_chunks(todo, self._FIELDS)):
            exists = (np.arange(c["cap"])[None, :] < np.asarray(c["lens"])[:, None]).reshape(-1)
            c["host"] = dict(image_ids=c["image_ids"], image=np.repeat(np.arange(c["n"]), c["cap"])[exists], boxes=got["boxes"].reshape(-1, 4)[exists],
                             scores=got["scores"][exists], classes=got["classes"][exists], flags=got["flags"][exists], milli=got["milli"][exists],
                             status=int(got["status"][0]))
        return [(kind, c["host"] if kind == "device" else c) for kind, c in self._segments]

    @staticmethod
    def _records(segments: Sequence[tuple]) -> Dict[int, List[str]]:
        """{class id: text records} in arrival order; a device chunk's records are rebuilt from its fetched fp32 arrays with process()'s
        format string."""
        predictions: Dict[int, List[str]] = defaultdict(list)
        for kind, seg in segments:
            if kind == "host":
                for cls_id, lines in seg.items():
                    predictions[cls_id].extend(lines)
                continue
            ids = [seg["image_ids"][i] for i in seg["image"].tolist()]
            for im, box, score, cls in zip(ids, seg["boxes"], seg["scores"].tolist(), seg["classes"].tolist()):
                xmin, ymin, xmax, ymax = box
                predictions[int(cls)].append(f"{im} {score:.3f} {xmin + 1:.1f} {ymin + 1:.1f} {xmax:.1f} {ymax:.1f}")
        return predictions

    def accumulate_from_flags(self, chunks: Sequence[dict], detail: Optional[dict] = None) -> Dict[str, float]:
        """The results from osr_voc_match's outputs instead of voc_eval's matching. chunks: per fetched batch the flat arrays `classes`,
        `flags` and `milli` over its detections in arrival order (image row, then detection row); the chunks in arrival order (with
        several ranks: in rank order, as the text records are concatenated). Per class the valid rows, sorted stably by descending
        milli / 1000, give the tp / fp / is_unk sequences voc_eval builds; the rest is voc_eval's arithmetic. npos and the number of
        unknown ground truths come from the annotations over all image ids. detail, if given, receives per class id voc_eval's
        return value."""
        cat = lambda key, dt: np.concatenate([np.asarray(c[key]).reshape(-1) for c in chunks]) if chunks else np.zeros(0, dtype=dt)  # noqa: E731
        classes, flags, milli = cat("classes", np.int64), cat("flags", np.uint8), cat("milli", np.int32)
        keep = (flags & VOC_VALID) != 0
        classes, flags, milli = classes[keep], flags[keep], milli[keep]
        by_class = np.argsort(classes, kind="stable")  # (arrival order inside a class)
        lo = np.searchsorted(classes[by_class], np.arange(self.total_num_class), side="left")
        hi = np.searchsorted(classes[by_class], np.arange(self.total_num_class), side="right")
        npos: Dict[str, int] = defaultdict(int)
        for im in self._image_ids:
            for o in self._annos[im]:
                if not o["difficult"]:
                    npos[o["name"]] += 1
        per_class = []
        for cls_id, name in enumerate(self._class_names):
            rows = by_class[lo[cls_id]:hi[cls_id]]
            conf = milli[rows].astype(np.float64) / 1000.0
            f = flags[rows[np.argsort(-conf, kind="stable")]]
            bit = lambda b: ((f & b) != 0).astype(np.float64)  # noqa: E731
            per_class.append(_curves(bit(VOC_TP), bit(VOC_FP), bit(VOC_UNK), npos[name], npos[UNKNOWN_NAME], name, self._is_2007))
            if detail is not None:
                detail[cls_id] = per_class[-1]
        return self._summarize(per_class)

    def _summarize(self, per_class: Sequence[tuple]) -> Dict[str, float]:
        """voc_eval's return value per class -> the nine results (:165-215)."""
        aps, recs, precs, all_recs, aose, tpfp, fpo = [], [], [], [], [], [], []
        for rec, prec, ap, unk_as_known, _, tp_plus_fp, fp_open in per_class:
            aps.append(ap * 100)
            aose.append(unk_as_known)
            all_recs.append(rec)
            tpfp.append(tp_plus_fp)
            fpo.append(fp_open)
            recs.append(rec[-1] * 100 if len(rec) else 0)
            precs.append(prec[-1] * 100 if len(prec) else 0)
        k = self.num_known_classes
        res = {"mAP": np.mean(aps), "WI": wilderness_impact(all_recs, tpfp, fpo, k, 0.8) * 100, "AOSE": np.sum(aose),
               "AP@K": np.mean(aps[:k]), "P@K": np.mean(precs[:k]), "R@K": np.mean(recs[:k]),
               "AP@U": aps[-1], "P@U": precs[-1], "R@U": recs[-1]}
        return {key: round(float(v), 2) for key, v in res.items()}

    def evaluate(self, detail: Optional[dict] = None) -> Optional[Dict[str, float]]:
        """Rank 0 gathers every rank's segments and scores them: from the kernel's flags when everything was matched on the device,
        else with voc_eval on the (rebuilt) text records. detail, if given, receives per class id voc_eval's return value."""
        gathered = parallel.gather_to_rank0({"segments": self._host_segments(), "reason": self._host_reason})
        if gathered is None:
            return None
        segments = [s for part in gathered for s in part["segments"]]
        reason = next((part["reason"] for part in gathered if part["reason"]), None)
        chunks = [seg for kind, seg in segments if kind == "device"]
        if chunks and reason is None:
            ids = [im for c in chunks for im in c["image_ids"]]
            if len(chunks) != len(segments):
                reason = "CPU and device input were mixed"
            elif any(c["status"] for c in chunks):
                reason = "a non-finite score or coordinate"
            elif len(set(ids)) != len(ids):
                reason = "an image was processed twice"
            if reason is not None:
                logger.warning("PascalVOCDetectionEvaluator: the whole evaluation goes through the numpy path (%s)", reason)
        from_flags = bool(chunks) and reason is None
        predictions = None
        if not from_flags or self.output_dir is not None:
            predictions = self._records(segments)
            if len(gathered) == 1:
                self._merged = predictions
        if self.output_dir is not None:  # the reference leaves one <class>.txt per class behind (:121-136)
            d = os.path.join(self.output_dir, "pascal_voc_eval")
            os.makedirs(d, exist_ok=True)
            for cls_id, name in enumerate(self._class_names):
                with open(os.path.join(d, name + ".txt"), "w") as f:
                    f.write("\n".join(predictions.get(cls_id, [""])))
        if from_flags:
            return self.accumulate_from_flags(chunks, detail)
        per_class = [voc_eval(predictions.get(cls_id, []), self._annos, self._image_ids, name, 0.5, self._is_2007, kind=self._sort_kind)
                     for cls_id, name in enumerate(self._class_names)]
        if detail is not None:
            detail.update(enumerate(per_class))
        return self._summarize(per_class)


class DatasetEvaluators:
    """[d2] DatasetEvaluators: several evaluators fed with the same inputs and outputs; evaluate() merges their result dicts (rank 0;
    None on the other ranks, where every member returns None)."""

    def __init__(self, evaluators: Sequence):
        self._evaluators = list(evaluators)

    def reset(self) -> None:
        for e in self._evaluators:
            e.reset()

    def process(self, inputs, outputs) -> None:
        for e in self._evaluators:
            e.process(inputs, outputs)

    def evaluate(self) -> Optional[dict]:
        results = None
        for e in self._evaluators:
            res = e.evaluate()
            if res is None:
                continue
            results = {} if results is None else results
            for k, v in res.items():
                assert k not in results, f"two evaluators report '{k}'"
                results[k] = v
        return results


def inference_on_dataset(model, batches, evaluator, rank: Optional[int] = None, world: Optional[int] = None):
    """[d2] inference_on_dataset as train.py:96 drives it: every rank runs the model over its share of the batches and feeds
    the evaluator; evaluate() gathers on rank 0 (None elsewhere). `batches` is a sequence of list[dict] inputs (each dict with
    "image", "image_id", optionally "height"/"width"); batch i goes to rank i % world -- images are independent, there is no
    data-path collective."""
    if rank is None or world is None:
        rank, world = parallel.world_info()
    evaluator.reset()
    for i, batch in enumerate(batches):
        if i % world != rank:
            continue
        evaluator.process(batch, model(batch))
    parallel.barrier()
    return evaluator.evaluate()
