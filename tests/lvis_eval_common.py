"""Shared by the LVIS evaluator tests: small LVIS JSONs, and the numpy LVISEval's per-image results laid out like osr_lvis_match's
outputs (flags, rank, match)."""
import json
import os

import numpy as np
import torch


def lvis_json(image_ids, cats, anns, neg=None, nex=None):
    """cats: (id, frequency) pairs; anns: dicts with image_id, category_id, bbox (xywh) and optionally area (default w * h) and
    ignore; neg / nex: {image id: [category ids]} for neg_category_ids / not_exhaustive_category_ids. Images carry a coco_url and no
    file_name, as LVIS v1 does."""
    neg, nex = neg or {}, nex or {}
    return dict(images=[dict(id=i, coco_url=f"http://images.cocodataset.org/val2017/{i:012d}.jpg", height=480, width=640,
                             neg_category_ids=list(neg.get(i, [])), not_exhaustive_category_ids=list(nex.get(i, []))) for i in image_ids],
                categories=[dict(id=c, name=f"c{c}", frequency=f) for c, f in cats],
                annotations=[dict({"area": float(a["bbox"][2] * a["bbox"][3])}, **a, id=k + 1) for k, a in enumerate(anns)])


def det(image_id, category_id, xywh, score):
    return dict(image_id=image_id, category_id=category_id, bbox=[float(v) for v in xywh], score=float(score))


def run_lvis(gt, dets, **kw):
    from openset_rcnn_amd.host.lvis_evaluation import LVISEval
    ev = LVISEval(gt, dets, **kw)
    ev.evaluate()
    ev.accumulate()
    return ev


def batch_tables(gt, image_ids):
    """-> (tables, gt rows, entries, img_off, ev_gt_off, the largest group) of the batch."""
    from openset_rcnn_amd.host.lvis_evaluation import _LVISTables
    tb = _LVISTables(gt)
    return (tb,) + tb.batch(image_ids)


def reference_outputs(gt, image_ids, boxes, scores, classes, counts, max_dets):
    """The numpy LVISEval on the padded lists -> (flags (n, cap, A) uint32, rank (n, cap) int32, match (n, cap, A, T) int32). A row whose
    class is outside [0, K) becomes a record of a category the JSON does not have: it takes part in the cut and in nothing else."""
    from openset_rcnn_amd.host.coco_evaluation import detection_records
    from openset_rcnn_amd.host.lvis_evaluation import AREA_RNG, IOU_THRS, LVISEval
    tb, _, ents, img_off, ev_gt_off, _ = batch_tables(gt, image_ids)
    K = len(tb.cat_ids)
    rev = dict(enumerate(tb.cat_ids))
    for c in np.unique(classes):
        if not 0 <= int(c) < K:
            rev[int(c)] = -1000 - abs(int(c))  # (no such category)
    n, cap = scores.shape
    records, where = [], []
    for i in range(n):
        rows = list(range(int(counts[i])))
        records += detection_records(image_ids[i], boxes[i, rows], scores[i, rows], classes[i, rows], None, rev)
        where += [(i, r) for r in rows]
    ev = LVISEval(gt, records, max_dets=max_dets)
    ev.evaluate()
    T, A = len(IOU_THRS), len(AREA_RNG)
    flags, rank = np.zeros((n, cap, A), dtype=np.uint32), -np.ones((n, cap), dtype=np.int32)
    match = -np.ones((n, cap, A, T), dtype=np.int32)
    img_index = {img: i for i, img in enumerate(image_ids)}
    cat_pos = {c: k for k, c in enumerate(tb.cat_ids)}
    entry = {(i, int(tb.ent_cat[e])): img_off[i] + j for i in range(n) for j, e in enumerate(ents[img_off[i]:img_off[i + 1]])}
    for (img, cat, a), e in ev.eval_imgs.items():
        i = img_index[img]
        g0 = ev_gt_off[entry[i, cat_pos[cat]]]
        for d, did in enumerate(e["dt_ids"]):
            ii, r = where[did - 1]
            assert ii == i
            rank[i, r] = d
            for t in range(T):
                if e["dt_matched"][t, d]:
                    flags[i, r, a] |= np.uint32(1 << t)
                    match[i, r, a, t] = g0 + e["dt_gt"][t, d]
                if e["dt_ignore"][t, d]:
                    flags[i, r, a] |= np.uint32(1 << (16 + t))
    return flags, rank, match


def device_match(osr, dev, gt, image_ids, boxes, scores, classes, counts, max_dets, want_sim=False):
    """ops.lvis_match on the same inputs -> (flags uint32, rank, match, sim or None) as numpy arrays."""
    from openset_rcnn_amd.host.lvis_evaluation import AREA_RNG, IOU_THRS
    tb, rows, ents, img_off, ev_gt_off, max_group = batch_tables(gt, image_ids)
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).to(dev)  # noqa: E731
    flags, rank, match, sim = osr.ops.lvis_match(
        t(boxes, np.float32), t(scores, np.float32), t(classes, np.int64), t(counts, np.int32), len(tb.cat_ids), t(img_off, np.int32), t(tb.ent_cat[ents]),
        t(ev_gt_off, np.int32), t(tb.ent_flags[ents]), t(tb.box[rows]), t(tb.area[rows]), t(tb.flags[rows]), max_group, IOU_THRS, AREA_RNG, max_dets,
        want_match=True, want_sim=want_sim)
    return flags.cpu().numpy().view(np.uint32), rank.cpu().numpy(), match.cpu().numpy(), sim.cpu().numpy() if sim is not None else None


def register(tmp_path, gt, tag):
    from openset_rcnn_amd.host import datasets as D
    path = os.path.join(str(tmp_path), f"{tag}.json")
    with open(path, "w") as f:
        json.dump(gt, f)
    name = f"lvis_{tmp_path.name}_{tag}"
    if name not in D.DatasetCatalog:
        D.register_lvis_instances(name, {}, path, str(tmp_path))
    return name


def instances(d, device="cpu"):
    from openset_rcnn_amd.host.structures import Boxes, Instances
    return Instances((480, 640), pred_boxes=Boxes(torch.from_numpy(d["boxes"]).to(device)), scores=torch.from_numpy(d["scores"]).to(device),
                     pred_classes=torch.from_numpy(d["classes"]).to(device))


def seeded_lvis(seed, n_images=6, n_cats=9, gts_per_image=7, dets_per_image=40, neutral=False):
    """A small LVIS JSON and per-image detections near its ground truths. Categories 1 .. n_cats with frequencies r, c, f in turn.
    neutral: nothing ignored, nothing not exhaustive, and every category an image has no ground truth of is negative (COCO's rules);
    otherwise some ground truths carry `ignore`, an image lists a few negatives and marks one of its positives not exhaustive, and the
    detections include categories that are not evaluated in their image."""
    from tests.coco_eval_common import jitter_xyxy, random_boxes_xywh
    rng = np.random.default_rng(seed)
    image_ids = [11 + 3 * i for i in range(n_images)]
    cat_ids = list(range(1, n_cats + 1))
    anns, dets, neg, nex = [], [], {}, {}
    for img in image_ids:
        g = random_boxes_xywh(rng, gts_per_image)
        gc = rng.integers(0, n_cats, size=gts_per_image)
        for j in range(gts_per_image):
            a = dict(image_id=img, category_id=cat_ids[gc[j]], bbox=g[j].tolist(), area=float(g[j, 2] * g[j, 3] * 0.8))
            if not neutral and rng.random() < 0.15:
                a["ignore"] = 1
            anns.append(a)
        absent = [c for k, c in enumerate(cat_ids) if k not in set(gc.tolist())]
        neg[img] = absent if neutral else absent[::2]
        if not neutral:
            nex[img] = [cat_ids[gc[0]]]
        src = rng.integers(0, gts_per_image, size=dets_per_image)
        c = np.where(rng.random(dets_per_image) < 0.7, gc[src], rng.integers(0, n_cats, size=dets_per_image)).astype(np.int64)
        dets.append(dict(boxes=jitter_xyxy(rng, g[src], 5.0), scores=(rng.integers(1, 40, size=dets_per_image) / 40.0).astype(np.float32), classes=c))
    return lvis_json(image_ids, [(c, "rcf"[k % 3]) for k, c in enumerate(cat_ids)], anns, neg, nex), image_ids, dets
