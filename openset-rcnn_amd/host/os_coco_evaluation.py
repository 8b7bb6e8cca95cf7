"""Open-set COCO-style evaluator of the GraspNet benchmark, bounding boxes only.

Own numpy implementation of the protocol in /root/reference/openset_rcnn/evaluation/os_cocoeval.py (OpensetCOCOEval, a subclass
of pycocotools' COCOeval -- not installed here, so the inherited parts are restated too) and of the result derivation in
os_coco_evaluation.py:336-440:

  * ground truth: every annotation whose category is not one of the known ids becomes category 1000 ("unknown",
    os_coco_evaluation.py:603-605); detections carry dataset category ids, 1000 for the unknown class;
  * per image and known category c, detections of c (score-descending, stable, at most maxDets[-1]) are matched greedily,
    COCO style (a detection takes the best still-free GT with IoU >= t; ignored GT sorted last; crowd GT can be matched
    repeatedly), three times: against the GT of c (true positives), against the GT of the OTHER known categories and against the
    unknown GT (os_cocoeval.py:242-424). Unknown detections are matched against all known GT and against the unknown GT
    (:426-555). IoU as pycocotools' maskUtils.iou on xywh boxes (intersection / union, or / detection area for crowd GT);
  * accumulation (:557-787): per IoU threshold, category, area range and maxDets the precision envelope sampled at 101 recall
    thresholds, recall, and the open-set counters: known detections matched to unknown GT (A-OSE), to other-known GT, unknown
    detections matched to known GT, and closed-set TP+FP / open-set FP at each recall threshold (wilderness impact);
  * summary (:789-972): 30 numbers -- known AP / AP50 / AP75 / APs / APm / APl, AR@10/20/30/50/100, ARs / ARm / ARl, WI at
    recall 0.8 and IoU 0.5, A-OSE at IoU 0.5, then the same 14 AP/AR numbers for the unknown class.

`OpensetCOCOEval` is the specification. For device `Instances` the per-image half runs on the device instead (include/osr.h
osr_os_coco_match, which restates the matching rules; csrc/osr_os_coco_eval.hip): `OpensetCOCOEvaluator.process` launches it once per
batch and keeps detections, ranks and flags there; `evaluate` fetches them in one copy and `accumulate_from_flags` fills eval_kdt /
eval_unkdt through the same `_fill_known` / `_fill_unknown` / `_pr` as `accumulate()`, so both paths return equal figures.
"""
from __future__ import annotations

import copy
import json
import logging
import os
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import parallel

logger = logging.getLogger(__name__)

UNKNOWN_CAT = 1000


def box_iou_xywh(d: np.ndarray, g: np.ndarray, iscrowd: Sequence[int]) -> np.ndarray:
    """pycocotools maskUtils.iou for boxes: (D,4) x (G,4) xywh -> (D,G); crowd columns use the detection's area as denominator."""
    d, g = np.asarray(d, dtype=np.float64).reshape(-1, 4), np.asarray(g, dtype=np.float64).reshape(-1, 4)
    if len(d) == 0 or len(g) == 0:
        return np.zeros((len(d), len(g)))
    dx2, dy2, gx2, gy2 = d[:, 0] + d[:, 2], d[:, 1] + d[:, 3], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]
    w = np.clip(np.minimum(dx2[:, None], gx2[None]) - np.maximum(d[:, 0][:, None], g[:, 0][None]), 0, None)
    h = np.clip(np.minimum(dy2[:, None], gy2[None]) - np.maximum(d[:, 1][:, None], g[:, 1][None]), 0, None)
    inter = w * h
    da, ga = (d[:, 2] * d[:, 3])[:, None], (g[:, 2] * g[:, 3])[None]
    crowd = np.asarray(iscrowd, dtype=bool)[None]
    union = np.where(crowd, da, da + ga - inter)
    return np.where(union > 0, inter / np.maximum(union, 1e-300), 0.0)


def _greedy_match(ious: np.ndarray, dt_ids, gt_ids, gt_ignore: np.ndarray, gt_crowd, iou_thrs) -> tuple:
    """COCOeval.evaluateImg inner loops: returns (dtm (T,D) matched gt id or 0, gtm (T,G), dtIg (T,D))."""
    T, D, G = len(iou_thrs), len(dt_ids), len(gt_ids)
    dtm, gtm, dtig = np.zeros((T, D)), np.zeros((T, G)), np.zeros((T, D))
    if ious.size == 0:
        return dtm, gtm, dtig
    for ti, t in enumerate(iou_thrs):
        for di in range(D):
            iou, m = min(t, 1 - 1e-10), -1
            for gi in range(G):
                if gtm[ti, gi] > 0 and not gt_crowd[gi]:
                    continue
                if m > -1 and gt_ignore[m] == 0 and gt_ignore[gi] == 1:
                    break
                if ious[di, gi] < iou:
                    continue
                iou, m = ious[di, gi], gi
            if m == -1:
                continue
            dtig[ti, di] = gt_ignore[m]
            dtm[ti, di] = gt_ids[m]
            gtm[ti, m] = dt_ids[di]
    return dtm, gtm, dtig


class OpensetCOCOEval:
    def __init__(self, gt_dataset: dict, detections: List[dict], known_cat_ids: Sequence[int], max_dets: Sequence[int] = (10, 20, 30, 50, 100),
                 img_ids: Optional[Sequence] = None):
        self.cat_ids = sorted(int(c) for c in known_cat_ids)
        known = set(self.cat_ids)
        self.max_dets = sorted(max_dets)
        self.iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.area_lbl = ["all", "small", "medium", "large"]
        self.img_ids = sorted(set(img_ids)) if img_ids is not None else sorted({im["id"] for im in gt_dataset["images"]})
        self._k_gts, self._ok_gts, self._unk_gts = defaultdict(list), defaultdict(list), defaultdict(list)
        self._k_dts, self._unk_dts = defaultdict(list), defaultdict(list)
        imgs = set(self.img_ids)
        k_gts = []
        for a in gt_dataset["annotations"]:
            if a["image_id"] not in imgs:
                continue
            a = dict(a)
            a["category_id"] = a["category_id"] if a["category_id"] in known else UNKNOWN_CAT
            a["iscrowd"] = int(a.get("iscrowd", 0))
            a["ignore"] = a["iscrowd"]
            a.setdefault("area", a["bbox"][2] * a["bbox"][3])
            if a["category_id"] == UNKNOWN_CAT:
                self._unk_gts[a["image_id"]].append(a)
            else:
                self._k_gts[a["image_id"], a["category_id"]].append(a)
                k_gts.append(a)
        for c in self.cat_ids:
            for a in k_gts:
                if a["category_id"] != c:
                    self._ok_gts[a["image_id"], c].append(a)
        for i, d in enumerate(detections):  # COCO.loadRes for box results: area = w*h, id = running index, iscrowd = 0
            if d["image_id"] not in imgs:
                continue
            d = dict(d)
            d["area"] = d["bbox"][2] * d["bbox"][3]
            d["id"] = i + 1
            d["iscrowd"] = 0
            if d["category_id"] == UNKNOWN_CAT:
                self._unk_dts[d["image_id"]].append(d)
            elif d["category_id"] in known:
                self._k_dts[d["image_id"], d["category_id"]].append(d)
        self.eval_kdt: dict = {}
        self.eval_unkdt: dict = {}
        self.stats = None

    # ---- per image ----------------------------------------------------------------------------------------
    @staticmethod
    def _sorted_dets(dt, max_det):
        order = np.argsort([-d["score"] for d in dt], kind="mergesort")
        return [dt[i] for i in order[:max_det]]

    def _ious(self, dt, gt):
        if len(gt) == 0 and len(dt) == 0:
            return np.zeros((0, 0))
        dt = self._sorted_dets(dt, self.max_dets[-1])
        return box_iou_xywh([d["bbox"] for d in dt], [g["bbox"] for g in gt], [g["iscrowd"] for g in gt])

    def _one(self, dt_sorted, gt, ious_full, a_rng):
        """Match one detection list against one GT list for an area range: (dtm, dtIg incl. the out-of-range rule, gtIg)."""
        ig = np.array([1 if (g["ignore"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt], dtype=np.int64)
        order = np.argsort(ig, kind="mergesort")
        gt = [gt[i] for i in order]
        ig = ig[order] if len(ig) else ig
        ious = ious_full[:, order] if ious_full.size else ious_full
        dtm, gtm, dtig = _greedy_match(ious[: len(dt_sorted)] if ious.size else ious, [d["id"] for d in dt_sorted], [g["id"] for g in gt], ig,
                                       [g["iscrowd"] for g in gt], self.iou_thrs)
        out = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt_sorted]).reshape(1, len(dt_sorted))
        dtig = np.logical_or(dtig, np.logical_and(dtm == 0, np.repeat(out, len(self.iou_thrs), 0)))
        return dtm, dtig, ig

    def evaluate(self):
        max_det = self.max_dets[-1]
        self.eval_imgs_kdt, self.eval_imgs_unkdt = [], []
        for c in self.cat_ids:
            for a_rng in self.area_rng:
                for im in self.img_ids:
                    k_gt, ok_gt, u_gt, k_dt = self._k_gts[im, c], self._ok_gts[im, c], self._unk_gts[im], self._k_dts[im, c]
                    dts = self._sorted_dets(k_dt, max_det)
                    m_k, ig_k, gig_k = self._one(dts, k_gt, self._ious(k_dt, k_gt), a_rng)
                    m_ok, ig_ok, _ = self._one(dts, ok_gt, self._ious(k_dt, ok_gt), a_rng)
                    m_u, ig_u, _ = self._one(dts, u_gt, self._ious(k_dt, u_gt), a_rng)
                    self.eval_imgs_kdt.append(dict(scores=[d["score"] for d in dts], m_k=m_k, m_ok=m_ok, m_u=m_u, ig_k=ig_k, ig_ok=ig_ok, ig_u=ig_u,
                                                   gt_ig=gig_k))
        for a_rng in self.area_rng:
            for im in self.img_ids:
                k_gt = [g for c in self.cat_ids for g in self._k_gts[im, c]]
                u_gt, u_dt = self._unk_gts[im], self._unk_dts[im]
                if len(u_gt) == 0 and len(u_dt) == 0:
                    self.eval_imgs_unkdt.append(None)
                    continue
                dts = self._sorted_dets(u_dt, max_det)
                m_k, ig_k, _ = self._one(dts, k_gt, self._ious(u_dt, k_gt), a_rng)
                m_u, ig_u, gig_u = self._one(dts, u_gt, self._ious(u_dt, u_gt), a_rng)
                self.eval_imgs_unkdt.append(dict(scores=[d["score"] for d in dts], m_k=m_k, m_u=m_u, ig_k=ig_k, ig_u=ig_u, gt_ig=gig_u))

    # ---- accumulation -------------------------------------------------------------------------------------
    def _pr(self, tp, fp, npig, scores_sorted):
        """Precision envelope sampled at the recall thresholds (COCOeval.accumulate inner block)."""
        R = len(self.rec_thrs)
        nd = len(tp)
        rc = tp / npig
        pr = tp / (fp + tp + np.spacing(1))
        pr = np.maximum.accumulate(pr[::-1])[::-1]  # the envelope: the running maximum from the right
        q, ss = np.zeros(R), np.zeros(R)
        inds = np.searchsorted(rc, self.rec_thrs, side="left")
        ok = inds < nd  # (rc does not decrease, so neither does inds: nothing is filled past the first miss)
        q[ok], ss[ok] = pr[inds[ok]], np.asarray(scores_sorted, dtype=np.float64)[inds[ok]]
        return rc, q, ss, inds

    def _empty_known(self) -> dict:
        T, R, K, A, M = len(self.iou_thrs), len(self.rec_thrs), len(self.cat_ids), len(self.area_rng), len(self.max_dets)
        return dict(precision=-np.ones((T, R, K, A, M)), recall=-np.ones((T, K, A, M)), scores=-np.ones((T, R, K, A, M)), ok_det_as_known=np.zeros((T, K, A, M)),
                    unk_det_as_known=np.zeros((T, K, A, M)), tp_plus_fp_cs=np.zeros((T, R, K, A, M)), fp_os=np.zeros((T, R, K, A, M)))

    def _empty_unknown(self) -> dict:
        T, R, A, M = len(self.iou_thrs), len(self.rec_thrs), len(self.area_rng), len(self.max_dets)
        return dict(precision=-np.ones((T, R, A, M)), recall=-np.ones((T, A, M)), scores=-np.ones((T, R, A, M)), k_det_as_unk=np.zeros((T, A, M)))

    def _fill_known(self, out, k, a, m, scs, m_k, ig_k, m_ok, ig_ok, m_u, ig_u, npig):
        """One (category, area range, maxDets) of eval_kdt from the (T, N) matched / ignored arrays of its three matchings, the
        detections already in descending-score order. Shared by accumulate() and accumulate_from_flags()."""
        tps = np.logical_and(m_k, np.logical_not(ig_k))
        fps = np.logical_and(np.logical_not(m_k), np.logical_not(ig_k))
        okfps = np.logical_and(m_ok, np.logical_not(ig_ok))
        ufps = np.logical_and(m_u, np.logical_not(ig_u))
        tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(float), np.cumsum(fps, axis=1).astype(float)
        ufp_sum = np.cumsum(ufps, axis=1).astype(float)
        for t in range(len(self.iou_thrs)):
            tp, fp, ufp = tp_sum[t], fp_sum[t], ufp_sum[t]
            if len(ufp):
                out["unk_det_as_known"][t, k, a, m] = ufp[-1]
            out["ok_det_as_known"][t, k, a, m] = float(np.sum(okfps[t]))
            rc, q, ss, pinds = self._pr(tp, fp, npig, scs)
            out["recall"][t, k, a, m] = rc[-1] if len(tp) else 0
            out["precision"][t, :, k, a, m], out["scores"][t, :, k, a, m] = q, ss
            n = len(tp)
            if n:
                pi = np.where(pinds == n, pinds - 1, pinds)
                out["tp_plus_fp_cs"][t, :, k, a, m] = (tp + fp)[pi]
                out["fp_os"][t, :, k, a, m] = ufp[pi]

    def _fill_unknown(self, out, a, m, scs, m_k, ig_k, m_u, ig_u, npig):
        """One (area range, maxDets) of eval_unkdt, as _fill_known."""
        tps = np.logical_and(m_u, np.logical_not(ig_u))
        fps = np.logical_and(np.logical_not(m_u), np.logical_not(ig_u))
        kfps = np.logical_and(m_k, np.logical_not(ig_k))
        tp_sum, fp_sum, kfp_sum = np.cumsum(tps, axis=1).astype(float), np.cumsum(fps, axis=1).astype(float), np.cumsum(kfps, axis=1).astype(float)
        for t in range(len(self.iou_thrs)):
            if kfp_sum.shape[1]:
                out["k_det_as_unk"][t, a, m] = kfp_sum[t][-1]
            rc, q, ss, _ = self._pr(tp_sum[t], fp_sum[t], npig, scs)
            out["recall"][t, a, m] = rc[-1] if len(tp_sum[t]) else 0
            out["precision"][t, :, a, m], out["scores"][t, :, a, m] = q, ss

    def accumulate(self):
        K, A = len(self.cat_ids), len(self.area_rng)
        known, unknown = self._empty_known(), self._empty_unknown()
        I = len(self.img_ids)
        for k in range(K):
            for a in range(A):
                E = self.eval_imgs_kdt[(k * A + a) * I:(k * A + a + 1) * I]
                for m, max_det in enumerate(self.max_dets):
                    sc = np.concatenate([np.asarray(e["scores"][:max_det], dtype=np.float64) for e in E]) if E else np.zeros(0)
                    inds = np.argsort(-sc, kind="mergesort")
                    scs = sc[inds]
                    cat = lambda key: np.concatenate([e[key][:, :max_det] for e in E], axis=1)[:, inds]  # noqa: E731
                    m_k, m_ok, m_u, ig_k, ig_ok, ig_u = cat("m_k"), cat("m_ok"), cat("m_u"), cat("ig_k"), cat("ig_ok"), cat("ig_u")
                    npig = int(np.count_nonzero(np.concatenate([e["gt_ig"] for e in E]) == 0))
                    if npig == 0:
                        continue
                    self._fill_known(known, k, a, m, scs, m_k, ig_k, m_ok, ig_ok, m_u, ig_u, npig)
        self.eval_kdt = known
        for a in range(A):
            E = [e for e in self.eval_imgs_unkdt[a * I:(a + 1) * I] if e is not None]
            if not E:
                continue
            for m, max_det in enumerate(self.max_dets):
                sc = np.concatenate([np.asarray(e["scores"][:max_det], dtype=np.float64) for e in E])
                inds = np.argsort(-sc, kind="mergesort")
                scs = sc[inds]
                cat = lambda key: np.concatenate([e[key][:, :max_det] for e in E], axis=1)[:, inds]  # noqa: E731
                m_k, m_u, ig_k, ig_u = cat("m_k"), cat("m_u"), cat("ig_k"), cat("ig_u")
                npig = int(np.count_nonzero(np.concatenate([e["gt_ig"] for e in E]) == 0))
                if npig == 0:
                    continue
                self._fill_unknown(unknown, a, m, scs, m_k, ig_k, m_u, ig_u, npig)
        self.eval_unkdt = unknown

    def accumulate_from_flags(self, image: np.ndarray, slot: np.ndarray, rank: np.ndarray, score: np.ndarray, flags: np.ndarray, npig: np.ndarray):
        """accumulate() from osr_os_coco_match's outputs instead of evaluate()'s per-image results. One entry per detection row:
        image = the row's image as an index into self.img_ids (-1: not among them), slot = 0 .. K - 1 known / K unknown / -1, rank
        and flags (N, A, 3) uint32 as the kernel writes them, score fp32 or fp64; npig (K + 1, A) = the ground truths that are not
        ignored, per slot and area range, over ALL of self.img_ids (processed or not). The lists are put together as accumulate()
        does: images in sorted id order, each image's list in rank order, then a mergesort by descending score."""
        T, K, A = len(self.iou_thrs), len(self.cat_ids), len(self.area_rng)
        score = np.asarray(score).astype(np.float64)
        flags = np.asarray(flags).view(np.uint32).reshape(len(score), A, 3)
        listed = (rank >= 0) & (image >= 0)
        shifts = np.arange(T, dtype=np.uint32)[:, None]

        def bits(sub, a, s):
            w = flags[sub, a, s][None, :]
            return ((w >> shifts) & 1).astype(bool), ((w >> (shifts + 16)) & 1).astype(bool)

        known, unknown = self._empty_known(), self._empty_unknown()
        for k in range(K + 1):
            sel = np.nonzero(listed & (slot == k))[0]
            sel = sel[np.lexsort((rank[sel], image[sel]))]
            for m, max_det in enumerate(self.max_dets):
                sub = sel[rank[sel] < max_det]
                sub = sub[np.argsort(-score[sub], kind="mergesort")]
                for a in range(A):
                    if npig[k, a] == 0:
                        continue
                    (m0, i0), (m1, i1) = bits(sub, a, 0), bits(sub, a, 1)
                    if k < K:
                        m2, i2 = bits(sub, a, 2)
                        self._fill_known(known, k, a, m, score[sub], m0, i0, m1, i1, m2, i2, int(npig[k, a]))
                    else:
                        self._fill_unknown(unknown, a, m, score[sub], m1, i1, m0, i0, int(npig[k, a]))
        self.eval_kdt, self.eval_unkdt = known, unknown

    # ---- summary ------------------------------------------------------------------------------------------
    def summarize(self) -> np.ndarray:
        ai = {lbl: i for i, lbl in enumerate(self.area_lbl)}
        mi = {m: i for i, m in enumerate(self.max_dets)}

        def mean_valid(s):
            return -1 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

        def summ(ev, unknown, ap, iou=None, area="all", max_dets=100):
            s = ev["precision"] if ap else ev["recall"]
            if iou is not None:
                s = s[np.where(np.isclose(self.iou_thrs, iou))[0]]
            s = s[..., ai[area], mi[max_dets]]
            return mean_valid(s)

        last = self.max_dets[-1]
        st = np.zeros(30)
        for base, ev, unk in ((0, self.eval_kdt, False), (16, self.eval_unkdt, True)):
            st[base + 0] = summ(ev, unk, 1, max_dets=100 if 100 in mi else last)
            st[base + 1] = summ(ev, unk, 1, iou=.5, max_dets=last)
            st[base + 2] = summ(ev, unk, 1, iou=.75, max_dets=last)
            for j, area in enumerate(("small", "medium", "large")):
                st[base + 3 + j] = summ(ev, unk, 1, area=area, max_dets=last)
                st[base + 11 + j] = summ(ev, unk, 0, area=area, max_dets=last)
            for j in range(5):
                st[base + 6 + j] = summ(ev, unk, 0, max_dets=self.max_dets[j]) if j < len(self.max_dets) else -1
        t5, r8 = int(np.where(np.isclose(self.iou_thrs, .5))[0][0]), int(np.where(np.isclose(self.rec_thrs, .8))[0][0])
        a_all, m100 = ai["all"], mi.get(100, len(self.max_dets) - 1)
        tpfp, fpo = self.eval_kdt["tp_plus_fp_cs"][t5, r8, :, a_all, m100], self.eval_kdt["fp_os"][t5, r8, :, a_all, m100]
        with np.errstate(divide="ignore", invalid="ignore"):
            st[14] = np.mean(fpo) / np.mean(tpfp)
        st[15] = float(np.sum(self.eval_kdt["unk_det_as_known"][t5, :, a_all, m100]))
        self.stats = st
        self.k_det_as_unk = float(self.eval_unkdt["k_det_as_unk"][t5, a_all, m100])
        return st


METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR10", "AR20", "AR30", "AR50", "AR100", "ARs", "ARm", "ARl"]


def derive_results(stats: np.ndarray) -> Dict[str, Dict[str, float]]:
    """os_coco_evaluation.py:336-440 for eval_type "openset": percentages for known and unknown, WI and A-OSE as raw numbers.
    (The reference tests stats[idx] >= 0 -- the KNOWN entry -- when it formats the unknown entry idx + 16; kept.)"""
    known = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(METRICS)}
    known["WI"], known["AOSE"] = float(stats[14]), float(stats[15])
    unknown = {m: float(stats[i + 16] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(METRICS)}
    return {"bbox": known, "bbox_unknown": unknown}


def instances_to_coco_json(instances, img_id, reverse_id_map: Optional[Dict[int, int]] = None) -> List[dict]:
    """[d2] instances_to_coco_json for boxes: XYXY -> XYWH, contiguous class id -> dataset id (1000 stays 1000)."""
    boxes = instances.pred_boxes.tensor.detach().cpu().numpy().astype(np.float64)
    scores = instances.scores.detach().cpu().tolist()
    classes = instances.pred_classes.detach().cpu().tolist()
    out = []
    for b, s, c in zip(boxes, scores, classes):
        c = int(c)
        if reverse_id_map is not None and c != UNKNOWN_CAT:
            c = reverse_id_map[c]
        out.append(dict(image_id=img_id, category_id=c, bbox=[float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])], score=float(s)))
    return out


def records_from_arrays(image_ids: Sequence, boxes: np.ndarray, scores: np.ndarray, classes: np.ndarray, reverse_id_map: Optional[Dict[int, int]]) -> List[dict]:
    """instances_to_coco_json on rows fetched from the device: boxes (N, 4) fp32 xyxy widened to fp64 before the differences, the
    records equal to what the host path builds from the same Instances."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4).astype(np.float64)
    xywh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1).tolist()
    scores, classes = np.asarray(scores, dtype=np.float32).tolist(), np.asarray(classes).tolist()
    out = []
    for img, bb, s, c in zip(image_ids, xywh, scores, classes):
        c = int(c)
        if reverse_id_map is not None and c != UNKNOWN_CAT:
            c = reverse_id_map[c]
        out.append(dict(image_id=img, category_id=c, bbox=bb, score=float(s)))
    return out


class OpensetGroundTruthTables:
    """The JSON's annotations as flat arrays sorted by (image, slot, annotation order): what osr_os_coco_match reads (include/osr.h).
    slot: the category's position among the sorted known ids, K for every other category (the unknown class); pos: the
    annotation's position in the JSON's order within its image."""

    def __init__(self, gt: dict, known_ids: Sequence[int]):
        self.known_ids = sorted(int(c) for c in known_ids)
        K = self.num_known = len(self.known_ids)
        slot_of = {c: k for k, c in enumerate(self.known_ids)}
        anns = gt["annotations"]
        self.img_ids = sorted({im["id"] for im in gt["images"]} | {a["image_id"] for a in anns})
        self.img_pos = {v: i for i, v in enumerate(self.img_ids)}
        I, N = len(self.img_ids), len(anns)
        img = np.array([self.img_pos[a["image_id"]] for a in anns], dtype=np.int64)
        slot = np.array([slot_of.get(a["category_id"], K) for a in anns], dtype=np.int64)
        by_img = np.argsort(img, kind="mergesort")
        first = np.searchsorted(img[by_img], np.arange(I + 1), side="left")
        pos = np.zeros(N, dtype=np.int64)
        pos[by_img] = np.arange(N) - first[img[by_img]]
        order = np.lexsort((pos, slot, img))
        self.img, self.slot, self.pos = img[order], slot[order].astype(np.int32), pos[order].astype(np.int32)
        self.box = np.array([anns[i]["bbox"] for i in order], dtype=np.float64).reshape(-1, 4)
        self.area = np.array([anns[i]["area"] if "area" in anns[i] else anns[i]["bbox"][2] * anns[i]["bbox"][3] for i in order], dtype=np.float64)
        self.crowd = np.array([int(anns[i].get("iscrowd", 0)) for i in order], dtype=np.uint8)
        self.start = first  # an image's annotations: start[i] .. start[i + 1]
        self.ids_nonzero = all(a.get("id", 0) != 0 for a in anns)  # the numpy class reads "matched" as "matched id != 0"

    def batch(self, image_ids: Sequence):
        """-> (rows: indices into the flat arrays, image by image; img_off (n + 1) int32; the largest image)."""
        rows, per_image = [], []
        for img in image_ids:
            p = self.img_pos.get(img)
            r = np.arange(self.start[p], self.start[p + 1]) if p is not None else np.zeros(0, dtype=np.int64)
            rows.append(r)
            per_image.append(len(r))
        rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        return rows, np.concatenate(([0], np.cumsum(per_image))).astype(np.int32), max(per_image, default=0)

    def npig(self, area_rng, img_ids: Sequence) -> np.ndarray:
        """(K + 1, A): the ground truths that are not ignored, per slot, over the given images."""
        chosen = np.zeros(len(self.img_ids), dtype=bool)
        chosen[[self.img_pos[i] for i in img_ids if i in self.img_pos]] = True
        keep = chosen[self.img] & (self.crowd == 0)
        out = np.zeros((self.num_known + 1, len(area_rng)), dtype=np.int64)
        for a, (lo, hi) in enumerate(area_rng):
            out[:, a] = np.bincount(self.slot[keep & ~((self.area < lo) | (self.area > hi))], minlength=self.num_known + 1)
        return out

    def class_slots(self, reverse_id_map: Optional[Dict[int, int]]) -> Optional[np.ndarray]:
        """class value -> slot (include/osr.h: class_slot), or None when the values do not fit a table."""
        K = self.num_known
        slot_of = {c: k for k, c in enumerate(self.known_ids)}
        values = {int(c): slot_of[d] for c, d in reverse_id_map.items() if d in slot_of} if reverse_id_map is not None else dict(slot_of)
        if any(v < 0 for v in values) or max(values, default=0) >= 1 << 20:
            return None
        table = -np.ones(max(max(values, default=0), UNKNOWN_CAT) + 1, dtype=np.int32)
        for v, k in values.items():
            table[v] = k
        table[UNKNOWN_CAT] = K  # (1000 is the unknown class before anything else, as in instances_to_coco_json)
        return table


class _Detections:
    """Every rank's detections in processing order: ("host", records) and ("device", the arrays of one fetched chunk)."""

    def __init__(self, segments: List[tuple], host_reason: Optional[str]):
        self.segments, self.host_reason = segments, host_reason

    def __len__(self) -> int:
        return sum(len(seg) if kind == "host" else len(seg["scores"]) for kind, seg in self.segments)

    def has_device(self) -> bool:
        return any(kind == "device" for kind, _ in self.segments)

    def device_only(self) -> bool:
        """Whether the kernel's flags cover everything: device chunks only, each image in one of them, once."""
        ids = [i for kind, seg in self.segments if kind == "device" for i in seg["image_ids"]]
        return self.has_device() and self.host_reason is None and all(kind == "device" for kind, _ in self.segments) and len(set(ids)) == len(ids)

    def records(self, reverse_id_map) -> List[dict]:
        out: List[dict] = []
        for kind, seg in self.segments:
            out += seg if kind == "host" else records_from_arrays([seg["image_ids"][i] for i in seg["image"]], seg["boxes"], seg["scores"], seg["classes"],
                                                                  reverse_id_map)
        return out


class OpensetCOCOEvaluator:
    """DatasetEvaluator-shaped wrapper (os_coco_evaluation.py:31-300): reset / process / evaluate on a COCO-format ground-truth
    json; known_names select the known categories, everything else is "unknown".

    Device `Instances` (fp32 boxes and scores) are matched on the device: `process` pads the batch into the engines' list form,
    uploads the batch's ground-truth table in ONE buffer and calls ops.os_coco_match once; detections, ranks and flags stay in device
    buffers. `evaluate` fetches them in ONE copy, gathers on rank 0 and accumulates from the flags (OpensetCOCOEval.
    accumulate_from_flags, which shares its arithmetic with accumulate()). CPU `Instances`, `resume=True`, a batch beyond a kernel
    limit and a JSON with a zero or missing annotation id go through the numpy OpensetCOCOEval on the (rebuilt) records, as does a
    run that mixes the two kinds of input."""

    def __init__(self, gt_json, known_names: Sequence[str], contiguous_to_dataset_id: Optional[Dict[int, int]] = None,
                 max_dets_per_image: Sequence[int] = (10, 20, 30, 50, 100), output_dir: Optional[str] = None):
        if isinstance(gt_json, str):
            with open(gt_json) as f:
                gt_json = json.load(f)
        self.gt = gt_json
        names = set(known_names)
        self.known_ids = sorted(c["id"] for c in gt_json["categories"] if c["name"] in names)
        self.reverse_id_map = contiguous_to_dataset_id
        self.max_dets = list(max_dets_per_image)
        self.output_dir = output_dir
        from .coco_evaluation import _GroundTruthTables  # (that module imports this one)
        from .proposal_evaluation import ProposalRecall
        self.proposals = ProposalRecall(_GroundTruthTables(gt_json))
        self._tables: Optional[OpensetGroundTruthTables] = None  # built with the first device batch
        self._class_slot = None                                   # (host table or None, its device copy or None)
        self.reset()

    def reset(self):
        self._predictions: List[dict] = []   # the host path's records
        self._chunks: List[dict] = []        # per device batch: tensors that stay on the device
        self._segments: List[tuple] = []     # processing order: ("host", first record, last + 1) / ("device", chunk index)
        self._host_reason: Optional[str] = None
        self._saw_instances = False
        self.proposals.reset()

    def process(self, inputs, outputs):
        """outputs carry "instances", "proposals" (a ProposalNetwork's: class-agnostic AR, host/proposal_evaluation.py) or both."""
        if outputs and "proposals" in outputs[0]:
            self.proposals.process(inputs, outputs, keep=self.output_dir is not None)
            if "instances" not in outputs[0]:
                return
        self._saw_instances = self._saw_instances or len(outputs) > 0
        insts = [out["instances"] for out in outputs]
        if insts and insts[0].pred_boxes.tensor.is_cuda:
            reason = self._process_device([inp["image_id"] for inp in inputs], insts)
            if reason is None:
                return
            if self._host_reason is None:  # one line, not one per batch
                logger.warning("OpensetCOCOEvaluator: device predictions take the host path and the numpy OpensetCOCOEval scores everything (%s)", reason)
                self._host_reason = reason
        first = len(self._predictions)
        for inp, inst in zip(inputs, insts):
            self._predictions += instances_to_coco_json(inst, inp["image_id"], self.reverse_id_map)
        self._segments.append(("host", first, len(self._predictions)))

    def _process_device(self, image_ids, insts) -> Optional[str]:
        """The batch through ops.os_coco_match; -> None, or why this batch has to take the host path instead."""
        import torch
        from . import ops
        from .eval_buffers import upload_sections
        L = ops._lib
        if self._tables is None:
            self._tables = OpensetGroundTruthTables(self.gt, self.known_ids)
            table = self._tables.class_slots(self.reverse_id_map)
            self._class_slot = (table, None)
        tb = self._tables
        if not tb.ids_nonzero:
            return "an annotation without a non-zero id (the numpy class reads a match as a non-zero ground-truth id)"
        if self._class_slot[0] is None:
            return "class values that fit no slot table"
        max_det = sorted(self.max_dets)[-1]
        lens = [len(i) for i in insts]
        cap = max(max(lens), 1)
        if cap > L.OS_COCO_MAX_CAP or max_det > L.OS_COCO_MAX_DET:
            return f"{cap} detections in one image / maxDets {max_det}: osr_os_coco_match takes at most {L.OS_COCO_MAX_CAP} / {L.OS_COCO_MAX_DET}"
        if any(i.pred_boxes.tensor.dtype != torch.float32 or i.scores.dtype != torch.float32 for i in insts):
            return "boxes or scores that are not float32"
        rows, img_off, max_img = tb.batch(image_ids)
        if max_img > L.OS_COCO_MAX_GT:
            return f"{max_img} ground truths in one image: osr_os_coco_match takes at most {L.OS_COCO_MAX_GT}"
        dev = insts[0].pred_boxes.tensor.device
        if self._class_slot[1] is None or self._class_slot[1].device != dev:
            self._class_slot = (self._class_slot[0], torch.from_numpy(self._class_slot[0]).to(dev))
        n = len(insts)
        boxes = torch.zeros((n, cap, 4), dtype=torch.float32, device=dev)
        scores = torch.zeros((n, cap), dtype=torch.float32, device=dev)
        classes = torch.full((n, cap), -1, dtype=torch.int64, device=dev)
        for i, inst in enumerate(insts):
            m = lens[i]
            if m:
                boxes[i, :m], scores[i, :m], classes[i, :m] = inst.pred_boxes.tensor.detach(), inst.scores.detach(), inst.pred_classes.detach().to(torch.int64)
        # the batch's table, one buffer, one copy
        i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
        gt_box, gt_area, d_off, d_counts, gt_slot, gt_pos, gt_crowd = upload_sections(
            [tb.box[rows], tb.area[rows], i32(img_off), i32(lens), tb.slot[rows], tb.pos[rows], tb.crowd[rows]], dev)
        area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]  # OpensetCOCOEval's, like its thresholds
        iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        flags, rank, _ = ops.os_coco_match(boxes, scores, classes, d_counts, self._class_slot[1], tb.num_known, d_off, gt_box, gt_area, gt_slot, gt_pos, gt_crowd,
                                           max_img, iou_thrs, area_rng, max_det)
        self._chunks.append(dict(n=n, cap=cap, image_ids=list(image_ids), boxes=boxes, scores=scores, classes=classes, counts=d_counts, flags=flags, rank=rank))
        self._segments.append(("device", len(self._chunks) - 1))
        return None

    def _fetch(self) -> List[dict]:
        """Every device buffer in ONE copy -> per chunk the flat host arrays over the rows that exist."""
        from .eval_buffers import fetch_chunks
        fields = (("boxes", np.float32), ("scores", np.float32), ("classes", np.int64), ("counts", np.int32), ("flags", np.uint32), ("rank", np.int32))
        out = []
        for c, got in zip(self._chunks, fetch_chunks(self._chunks, fields)):
            n, cap = c["n"], c["cap"]
            exists = (np.arange(cap)[None, :] < got["counts"][:, None]).reshape(-1)
            out.append(dict(image_ids=c["image_ids"], image=np.repeat(np.arange(n), cap)[exists], boxes=got["boxes"].reshape(-1, 4)[exists],
                            scores=got["scores"][exists], classes=got["classes"][exists], rank=got["rank"][exists],
                            flags=got["flags"].reshape(n * cap, -1)[exists]))
        return out

    RESULTS_FILE = "coco_instances_results.json"

    def evaluate(self, img_ids=None, resume: bool = False):
        """Rank 0 gathers every rank's detections, writes them to <output_dir>/coco_instances_results.json
        (os_coco_evaluation.py:259-263) and scores them; `resume=True` scores that file instead of new detections
        (train.py --resume_test, os_coco_evaluation.py:156-190). The known / unknown precision and recall arrays are saved
        next to it (:428-431)."""
        if resume:
            if self.output_dir is None:
                raise ValueError("resume=True needs output_dir (where a previous run wrote its detections)")
            if parallel.world_info()[0] != 0:
                return None
            with open(os.path.join(self.output_dir, self.RESULTS_FILE)) as f:
                dets = json.load(f)
        else:
            keep = self.output_dir is not None
            fetched = self._fetch()
            segments = [("host", self._predictions[s[1]:s[2]]) if s[0] == "host" else ("device", fetched[s[1]]) for s in self._segments]
            gathered = parallel.gather_to_rank0({"segments": segments, "host_reason": self._host_reason, "instances": self._saw_instances,
                                                 "proposals": self.proposals.state(keep=keep)})
            if gathered is None:
                return None
            dets = _Detections([s for part in gathered for s in part["segments"]], next((part["host_reason"] for part in gathered if part["host_reason"]), None))
            states = [part["proposals"] for part in gathered]
            box_proposals = self.proposals.results(states)
            if box_proposals is not None:
                if self.output_dir:
                    self.proposals.write(states, self.output_dir)
                res = {"box_proposals": box_proposals}  # (first, as in the reference)
                if any(part["instances"] for part in gathered):
                    res.update(self._score(dets, img_ids, write=True))
                return res
            return self._score(dets, img_ids, write=True)
        return self._score(dets, img_ids, write=False)

    def _get_tables(self) -> OpensetGroundTruthTables:
        if self._tables is None:
            self._tables = OpensetGroundTruthTables(self.gt, self.known_ids)
            self._class_slot = (self._tables.class_slots(self.reverse_id_map), None)
        return self._tables

    def _accumulate_device(self, dets: "_Detections", img_ids) -> OpensetCOCOEval:
        """The figures from the kernel's flags: no per-image matching on the host."""
        ev = OpensetCOCOEval(dict(images=self.gt["images"], annotations=[]), [], self.known_ids, self.max_dets, img_ids)
        tb, parts = self._get_tables(), [seg for _, seg in dets.segments]
        table = self._class_slot[0]
        index = {img: i for i, img in enumerate(ev.img_ids)}
        image = np.concatenate([np.array([index.get(i, -1) for i in q["image_ids"]], dtype=np.int64)[q["image"]] for q in parts])
        classes = np.concatenate([q["classes"] for q in parts])
        inside = (classes >= 0) & (classes < len(table))
        slot = np.where(inside, table[np.where(inside, classes, 0)], -1)
        if self.reverse_id_map is not None:
            bad = classes[(classes != UNKNOWN_CAT) & ~np.isin(classes, np.array(list(self.reverse_id_map), dtype=np.int64))]
            if bad.size:
                raise KeyError(int(bad[0]))  # (what instances_to_coco_json raises for a class outside the map)
        ev.accumulate_from_flags(image, slot, np.concatenate([q["rank"] for q in parts]), np.concatenate([q["scores"] for q in parts]),
                                 np.concatenate([q["flags"] for q in parts]), tb.npig(ev.area_rng, ev.img_ids))
        return ev

    def _score(self, dets, img_ids, write: bool):
        """dets: the records (a list, `resume`) or the gathered segments (_Detections)."""
        device = isinstance(dets, _Detections) and dets.device_only()
        if isinstance(dets, _Detections):
            if not device and dets.has_device() and dets.host_reason is None:  # (a host_reason was logged when it arose)
                logger.warning("OpensetCOCOEvaluator: the whole evaluation goes through the numpy OpensetCOCOEval (CPU and device predictions are mixed, or "
                               "an image was processed twice)")
            records = dets.records(self.reverse_id_map) if not device or (write and self.output_dir) else None
            count = len(dets)
        else:
            records, count = dets, len(dets)
        if write and self.output_dir:
            os.makedirs(self.output_dir, exist_ok=True)
            with open(os.path.join(self.output_dir, self.RESULTS_FILE), "w") as f:
                json.dump(records, f)
        if not count:
            return {"bbox": {m: float("nan") for m in METRICS}}
        if device:
            ev = self._accumulate_device(dets, img_ids)
        else:
            ev = OpensetCOCOEval(copy.deepcopy(self.gt), records, self.known_ids, self.max_dets, img_ids)
            ev.evaluate()
            ev.accumulate()
        if self.output_dir:
            for tag, e in (("known", ev.eval_kdt), ("unknown", ev.eval_unkdt)):
                np.save(os.path.join(self.output_dir, f"{tag}_precision_bbox.npy"), e["precision"])
                np.save(os.path.join(self.output_dir, f"{tag}_recall_bbox.npy"), e["recall"])
        return derive_results(ev.summarize())
