"""Evaluators for what PanopticFPN and SemanticSegmentor produce: [d2] SemSegEvaluator (mIoU, fwIoU, mACC, pACC) and
[d2] COCOPanopticEvaluator (PQ, SQ, RQ; panopticapi's pq_compute). Neither detectron2, panopticapi nor pycocotools is at hand:
both are written from memory of detectron2 v0.6 and panopticapi, and the rules are spelled out in include/osr.h and below.

The per-pixel work runs on the device, where the models' outputs already are (csrc/osr_seg_eval.hip through host/ops.py):
`process` decodes the image's ground-truth PNG on the host, uploads its bytes and a few small tables, and launches; it copies nothing
back and does not synchronise. The statistics stay on the device for the whole dataset, and `evaluate` fetches them with ONE
device-to-host copy, gathers them on rank 0 (host.parallel) and does the final arithmetic in float64 numpy. There is no CPU
fallback: a prediction that is not on the GPU is refused by the ops, like everywhere else.

Not built: mask AP, box AP under the panoptic dataset names (host/coco_evaluation.py scores plain COCO instances datasets) and
TEST.AUG for the two meta-architectures."""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops, parallel
from .datasets import MetadataCatalog

PQ_FLAG_NAMES = ("predicted ids outside 0 .. the number of listed segments (flags[0])", "listed predicted segments without a pixel (flags[1])",
                 "segments whose category is unknown to the dataset (flags[2])")


def sem_seg_results(conf: np.ndarray, class_names: Sequence[str]) -> Dict[str, float]:
    """The figures of [d2] SemSegEvaluator.evaluate from the (C + 1, C + 1) matrix [pred][gt] (last column: ignored pixels), x100.
    On M = conf[:-1, :-1]: tp = diag, pos_gt = column sums, pos_pred = row sums; acc = tp / pos_gt where pos_gt > 0 (the valid
    classes, NaN elsewhere), iou = tp / (pos_gt + pos_pred - tp) where valid and the union is > 0; mACC / mIoU are the means over the
    valid classes, fwIoU = sum(iou * pos_gt / pos_gt.sum()), pACC = tp.sum() / pos_gt.sum()."""
    m = np.asarray(conf, dtype=np.int64)[:-1, :-1]
    c = m.shape[0]
    tp, pos_gt, pos_pred = np.diag(m).astype(np.float64), m.sum(axis=0).astype(np.float64), m.sum(axis=1).astype(np.float64)
    acc, iou = np.full(c, np.nan), np.full(c, np.nan)
    acc_valid = pos_gt > 0
    acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
    union = pos_gt + pos_pred - tp
    iou_valid = acc_valid & (union > 0)
    iou[iou_valid] = tp[iou_valid] / union[iou_valid]
    total = pos_gt.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        res = {"mIoU": 100 * np.sum(iou[iou_valid]) / np.sum(iou_valid), "fwIoU": 100 * np.sum(iou[iou_valid] * (pos_gt[iou_valid] / total)),
               "mACC": 100 * np.sum(acc[acc_valid]) / np.sum(acc_valid), "pACC": 100 * np.sum(tp) / total}
    for i, name in enumerate(class_names):
        res[f"IoU-{name}"] = 100 * iou[i]
    for i, name in enumerate(class_names):
        res[f"ACC-{name}"] = 100 * acc[i]
    return {k: float(v) for k, v in res.items()}


def pq_results(counts: np.ndarray, iou: np.ndarray, isthing: Sequence[bool]) -> Dict[str, float]:
    """panopticapi's PQStat.pq_average for all / thing / stuff categories, x100. counts (ncat, 3) {tp, fp, fn}, iou (ncat). Per
    category with tp + fp + fn > 0: pq = iou / (tp + fp / 2 + fn / 2), sq = iou / tp (0 when tp is 0), rq = tp / (tp + fp / 2 +
    fn / 2); a group's figure is the plain mean over its counted categories, 0 when it has none."""
    counts, iou = np.asarray(counts, dtype=np.float64), np.asarray(iou, dtype=np.float64)
    isthing = np.asarray(isthing, dtype=bool)
    res = {}
    for suffix, sel in (("", np.ones_like(isthing)), ("_th", isthing), ("_st", ~isthing)):
        pq = sq = rq = 0.0
        n = 0
        for i in np.nonzero(sel)[0]:
            tp, fp, fn = counts[i]
            if tp + fp + fn == 0:
                continue
            n += 1
            den = tp + 0.5 * fp + 0.5 * fn
            pq += iou[i] / den
            sq += iou[i] / tp if tp != 0 else 0.0
            rq += tp / den
        for key, v in (("PQ", pq), ("SQ", sq), ("RQ", rq)):
            res[key + suffix] = 100 * v / n if n else 0.0
    return res


def merge_sem_seg_partials(partials: Sequence[dict]) -> dict:
    """Per-rank {conf, invalid} -> their sum (integers: the order does not matter)."""
    return {"conf": sum(np.asarray(p["conf"], dtype=np.int64) for p in partials), "invalid": int(sum(int(p["invalid"]) for p in partials))}


def merge_pq_partials(partials: Sequence[dict]) -> dict:
    """Per-rank {counts, iou, flags} -> their sum, the ranks in order. The sum of per-rank partial iou sums is not bit-equal to the
    sum one process would have formed over all images: float64 addition is not associative."""
    return {"counts": sum(np.asarray(p["counts"], dtype=np.int64) for p in partials), "iou": sum(np.asarray(p["iou"], dtype=np.float64) for p in partials),
            "flags": sum(np.asarray(p["flags"], dtype=np.int64) for p in partials)}


class SemSegEvaluator:
    """[d2] SemSegEvaluator on a device confusion matrix. `process` takes output["sem_seg"] as the models return it, (C, H, W) float
    (the argmax is fused into the kernel), or an (H, W) integer label map, and the ground truth named by the input's
    "sem_seg_file_name" (a single-channel PNG of class ids, `ignore_label` for pixels that do not count)."""

    def __init__(self, dataset_name: str, num_classes: int, ignore_label: int, class_names: Sequence[str], output_dir: Optional[str] = None):
        self.dataset_name, self.num_classes, self.ignore_label = dataset_name, int(num_classes), int(ignore_label)
        self.class_names = list(class_names)
        if len(self.class_names) != self.num_classes:
            raise ValueError(f"SemSegEvaluator: {len(self.class_names)} class names for {self.num_classes} classes")
        self.output_dir = output_dir
        self._buf: Optional[torch.Tensor] = None  # (C + 1)^2 + 1 int64 on the device: the matrix, then the invalid counter

    def reset(self) -> None:
        if self._buf is not None:
            self._buf.zero_()

    def _views(self, device):
        n = self.num_classes + 1
        if self._buf is None or self._buf.device != device:
            self._buf = torch.zeros((n * n + 1,), dtype=torch.int64, device=device)
        return self._buf[: n * n].view(n, n), self._buf[n * n:]

    def process(self, inputs: Sequence[dict], outputs: Sequence[dict]) -> None:
        from PIL import Image
        for inp, out in zip(inputs, outputs):
            pred = out["sem_seg"]
            if pred.dim() == 3 and pred.is_floating_point():
                pred = pred.to(torch.float32).contiguous()
            elif pred.dim() == 2 and not pred.is_floating_point():
                pred = pred.to(torch.int32).contiguous()
            else:
                raise ValueError(f"SemSegEvaluator: sem_seg must be (C, H, W) float or (H, W) integer, got {tuple(pred.shape)} {pred.dtype}")
            gt = np.array(Image.open(inp["sem_seg_file_name"]))
            if gt.ndim != 2 or gt.dtype != np.uint8:
                raise ValueError(f"SemSegEvaluator: {inp['sem_seg_file_name']} must be a single-channel 8-bit image, got {gt.shape} {gt.dtype}")
            conf, invalid = self._views(pred.device)
            gt_dev = torch.from_numpy(np.ascontiguousarray(gt)).to(pred.device, non_blocking=True)
            ops.semseg_confusion(pred, gt_dev, self.num_classes, self.ignore_label, conf, invalid)

    def evaluate(self) -> Optional[dict]:
        n = self.num_classes + 1
        host = self._buf.cpu().numpy() if self._buf is not None else np.zeros(n * n + 1, dtype=np.int64)  # the one copy
        gathered = parallel.gather_to_rank0({"conf": host[:-1].reshape(n, n), "invalid": int(host[-1])})
        if gathered is None:
            return None
        total = merge_sem_seg_partials(gathered)
        if total["invalid"]:
            raise ValueError(f"SemSegEvaluator({self.dataset_name}): {total['invalid']} pixels carry a predicted label outside [0, {self.num_classes}) or a "
                             f"ground-truth value in [{self.num_classes}, 255] other than the ignore label {self.ignore_label}")
        res = sem_seg_results(total["conf"], self.class_names)
        if self.output_dir is not None:
            os.makedirs(self.output_dir, exist_ok=True)
            with open(os.path.join(self.output_dir, "sem_seg_evaluation.json"), "w") as f:
                json.dump({"results": res, "confusion": total["conf"].tolist()}, f)
        return {"sem_seg": res}


class COCOPanopticEvaluator:
    """[d2] COCOPanopticEvaluator / panopticapi pq_compute on device statistics. The dataset's metadata names its panoptic JSON and
    PNG directory (datasets.register_coco_panoptic_separated). A category slot is the position of a category in the JSON's
    `categories` sorted by id. `process` takes output["panoptic_seg"] = ((H, W) integer map, segments_info) with the segments' ids
    1 .. n (what PanopticFPN gives) and contiguous category ids, which go back to slots through the metadata's thing / stuff tables
    (an unknown id becomes slot -1 and is reported by evaluate()).

    evaluate() sums the ranks' statistics: the sum of per-rank partial IoU sums is not bit-equal to one process's sum over all
    images (float64 addition is not associative); the integer counts are."""

    def __init__(self, dataset_name: str, output_dir: Optional[str] = None):
        meta = MetadataCatalog.get(dataset_name)
        self.dataset_name, self.output_dir = dataset_name, output_dir
        self.panoptic_root = meta.panoptic_root
        with open(meta.panoptic_json) as f:
            data = json.load(f)
        cats = sorted(data["categories"], key=lambda c: c["id"])
        self.category_names = [c["name"] for c in cats]
        self.isthing = [bool(c["isthing"]) for c in cats]
        self._slot_of = {c["id"]: i for i, c in enumerate(cats)}
        self._thing_slot = {v: self._slot_of[k] for k, v in meta.thing_dataset_id_to_contiguous_id.items() if k in self._slot_of}
        self._stuff_slot = {v: self._slot_of[k] for k, v in meta.stuff_dataset_id_to_contiguous_id.items() if k in self._slot_of}
        self._annotations = {a["image_id"]: a for a in data["annotations"]}
        self._buf: Optional[torch.Tensor] = None  # int64 on the device: (ncat, 3) counts, 3 flags, then ncat float64 IoU sums

    @property
    def num_categories(self) -> int:
        return len(self.isthing)

    def reset(self) -> None:
        if self._buf is not None:
            self._buf.zero_()

    def _views(self, device):
        n = self.num_categories
        if self._buf is None or self._buf.device != device:
            self._buf = torch.zeros((4 * n + 3,), dtype=torch.int64, device=device)
        return self._buf[: 3 * n].view(n, 3), self._buf[3 * n: 3 * n + 3], self._buf[3 * n + 3:].view(torch.float64)

    def ground_truth_tables(self, image_id):
        """-> (PNG path, gt_ids (G) ascending, gt_meta (G, 4) {slot, iscrowd, area, crowd_pick}) of one image, int32 numpy."""
        ann = self._annotations[image_id]
        segs = ann["segments_info"]
        crowd_last = {}
        for s in segs:  # the JSON's order: a later crowd segment of a category replaces the earlier one
            if s.get("iscrowd", 0):
                crowd_last[s["category_id"]] = s["id"]
        segs = sorted(segs, key=lambda s: s["id"])
        ids = np.array([s["id"] for s in segs], dtype=np.int32)
        meta = np.array([[self._slot_of[s["category_id"]], int(bool(s.get("iscrowd", 0))), int(s["area"]),
                          int(crowd_last.get(s["category_id"]) == s["id"])] for s in segs], dtype=np.int32).reshape(-1, 4)
        return os.path.join(self.panoptic_root, ann["file_name"]), ids, meta

    def process(self, inputs: Sequence[dict], outputs: Sequence[dict]) -> None:
        from PIL import Image
        for inp, out in zip(inputs, outputs):
            pan, segments_info = out["panoptic_seg"]
            if segments_info is None:
                raise ValueError("COCOPanopticEvaluator: segments_info is None; the evaluator needs the list of segments (id, isthing, category_id) "
                                 "that PanopticFPN returns beside the map")
            n = len(segments_info)
            slots = np.full(n, -1, dtype=np.int32)
            seen = set()
            for s in segments_info:
                sid = int(s["id"])
                if not 1 <= sid <= n or sid in seen:
                    raise ValueError(f"COCOPanopticEvaluator: segment ids must be 1 .. {n}, each once; got {sid}")
                seen.add(sid)
                slots[sid - 1] = (self._thing_slot if s["isthing"] else self._stuff_slot).get(int(s["category_id"]), -1)
            path, ids, meta = self.ground_truth_tables(inp["image_id"])
            rgb = np.array(Image.open(path).convert("RGB"))
            if tuple(rgb.shape[:2]) != tuple(pan.shape):
                raise ValueError(f"COCOPanopticEvaluator: {path} is {rgb.shape[:2]}, the predicted map {tuple(pan.shape)}")
            dev = pan.device
            g = len(ids)
            tables = torch.from_numpy(np.concatenate((ids, meta.reshape(-1), slots))).to(dev, non_blocking=True)  # one upload for the three
            rgb_dev = torch.from_numpy(np.ascontiguousarray(rgb)).to(dev, non_blocking=True)
            counts_acc, flags, iou = self._views(dev)
            counts = ops.panoptic_pair_counts(rgb_dev, tables[:g], pan.to(torch.int32).contiguous(), n, flags)
            ops.pq_accumulate(counts, tables[g: 5 * g].view(g, 4), tables[5 * g:], counts_acc, iou, flags)

    def evaluate(self) -> Optional[dict]:
        n = self.num_categories
        host = self._buf.cpu() if self._buf is not None else torch.zeros(4 * n + 3, dtype=torch.int64)  # the one copy
        part = {"counts": host[: 3 * n].view(n, 3).numpy(), "flags": host[3 * n: 3 * n + 3].numpy(), "iou": host[3 * n + 3:].view(torch.float64).numpy()}
        gathered = parallel.gather_to_rank0(part)
        if gathered is None:
            return None
        total = merge_pq_partials(gathered)
        for i, name in enumerate(PQ_FLAG_NAMES):
            if total["flags"][i]:
                raise ValueError(f"COCOPanopticEvaluator({self.dataset_name}): {int(total['flags'][i])} {name}")
        res = pq_results(total["counts"], total["iou"], self.isthing)
        if self.output_dir is not None:
            os.makedirs(self.output_dir, exist_ok=True)
            with open(os.path.join(self.output_dir, "panoptic_evaluation.json"), "w") as f:
                json.dump({"results": res, "categories": self.category_names, "tp_fp_fn": total["counts"].tolist(), "iou": total["iou"].tolist()}, f)
        return {"panoptic_seg": res}
