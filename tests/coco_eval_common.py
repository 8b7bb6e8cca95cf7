"""Shared by the COCO evaluator tests: small COCO JSONs, seeded detections in the engines' padded list form, and the numpy COCOeval's
per-image results laid out like osr_coco_match's outputs (flags, rank, match, similarities)."""
import json
import os

import numpy as np
import torch


def coco_json(image_ids, cat_ids, anns, names=None):
    """anns: dicts with image_id, category_id, bbox (xywh) and whatever else COCO allows; ids are assigned in order from 1."""
    return dict(images=[dict(id=i, file_name=f"{i}.jpg", height=480, width=640) for i in image_ids],
                categories=[dict(id=c, name=(names[k] if names else f"c{c}")) for k, c in enumerate(cat_ids)],
                annotations=[dict(a, id=k + 1) for k, a in enumerate(anns)])


def det(image_id, category_id, xywh, score, **kw):
    return dict(image_id=image_id, category_id=category_id, bbox=[float(v) for v in xywh], score=float(score), **kw)


def run_eval(osr, gt, dets, iou_type="bbox", **kw):
    from openset_rcnn_amd.host.coco_evaluation import COCOeval
    ev = COCOeval(gt, dets, iou_type, **kw)
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev


def random_boxes_xywh(rng, n, extent=260.0):
    """Boxes on a quarter-pixel grid (exact in fp32) whose areas straddle COCO's 32^2 and 96^2 limits."""
    side = rng.choice([6.0, 14.0, 30.0, 34.0, 60.0, 95.0, 97.0, 130.0], size=(n, 2)) + rng.integers(0, 8, size=(n, 2)) / 4.0
    xy = rng.integers(0, int(extent * 4), size=(n, 2)) / 4.0
    return np.concatenate([xy, side], axis=1)


def jitter_xyxy(rng, xywh, scale=6.0):
    """Detections near the given boxes: xyxy fp32 on the quarter-pixel grid."""
    b = np.asarray(xywh, dtype=np.float64)
    out = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], axis=1) + rng.integers(-int(scale * 4), int(scale * 4) + 1, size=(len(b), 4)) / 4.0
    out[:, 2:] = np.maximum(out[:, 2:], out[:, :2] + 0.25)
    return out.astype(np.float32)


def reference_outputs(osr, gt, image_ids, boxes, scores, classes, counts, task, max_det, keypoints=None, sigmas=None):
    """The numpy COCOeval on the padded lists -> (flags (n, cap, A) uint32, rank (n, cap) int32, match (n, cap, A, T) int32, sims:
    {(image index, category index): (M, G) matrix over the ranked detections and the group's ground truths}, tables, seg_off)."""
    from openset_rcnn_amd.host.coco_evaluation import COCOeval, Params, _GroundTruthTables, detection_records
    tb = _GroundTruthTables(gt)
    K = len(tb.cat_ids)
    rev = dict(enumerate(tb.cat_ids))
    n, cap = scores.shape
    records, where = [], []
    for i in range(n):
        rows = [r for r in range(int(counts[i])) if 0 <= int(classes[i, r]) < K]
        records += detection_records(image_ids[i], boxes[i, rows], scores[i, rows], classes[i, rows], keypoints[i, rows] if keypoints is not None else None, rev)
        where += [(i, r) for r in rows]
    ev = COCOeval(gt, records, task, kpt_oks_sigmas=sigmas, max_dets=[max_det])
    ev.evaluate()
    p = Params(task)
    T, A, I = len(p.iou_thrs), len(p.area_rng), len(ev.img_ids)
    flags, rank = np.zeros((n, cap, A), dtype=np.uint32), -np.ones((n, cap), dtype=np.int32)
    match = -np.ones((n, cap, A, T), dtype=np.int32)
    _, seg_off, _ = tb.batch(image_ids)
    img_index = {img: i for i, img in enumerate(image_ids)}
    sims = {}
    for k in range(K):
        for a in range(A):
            for e in ev.eval_imgs[(k * A + a) * I:(k * A + a + 1) * I]:
                if e is None or e["image_id"] not in img_index:
                    continue
                i = img_index[e["image_id"]]
                sims[i, k] = ev.ious[e["image_id"], e["category_id"]]
                for d, did in enumerate(e["dt_ids"]):
                    ii, r = where[did - 1]
                    assert ii == i
                    rank[i, r] = d
                    for t in range(T):
                        if e["dt_matched"][t, d]:
                            flags[i, r, a] |= np.uint32(1 << t)
                            match[i, r, a, t] = seg_off[i * K + k] + e["dt_gt"][t, d]
                        if e["dt_ignore"][t, d]:
                            flags[i, r, a] |= np.uint32(1 << (16 + t))
    return flags, rank, match, sims, tb, seg_off


def device_match(osr, dev, gt, image_ids, boxes, scores, classes, counts, task, max_det, keypoints=None, sigmas=None, want_sim=False):
    """ops.coco_match on the same inputs -> (flags uint32, rank, match, sim or None) as numpy arrays."""
    import torch
    from openset_rcnn_amd.host.coco_evaluation import Params, _GroundTruthTables
    tb = _GroundTruthTables(gt)
    rows, seg_off, max_group = tb.batch(image_ids)
    p = Params(task)
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).to(dev)  # noqa: E731
    kp = keypoints is not None
    ng = len(rows)
    flags, rank, match, sim = osr.ops.coco_match(
        t(boxes, np.float32), t(scores, np.float32), t(classes, np.int64), t(counts, np.int32), len(tb.cat_ids), t(seg_off, np.int32), t(tb.box[rows]),
        t(tb.area[rows]), t(tb.flags[task][rows]), max_group, p.iou_thrs, p.area_rng, max_det, keypoints=t(keypoints, np.float32) if kp else None,
        gt_kpts=t(tb.kpts[rows] if ng else np.zeros((0, len(sigmas), 3))) if kp else None, sigmas=t(sigmas, np.float64) if kp else None, want_match=True,
        want_sim=want_sim)
    return flags.cpu().numpy().view(np.uint32), rank.cpu().numpy(), match.cpu().numpy(), sim.cpu().numpy() if sim is not None else None


def seeded_dataset(seed, n_images=6, n_cats=3, keypoints=0, gts_per_image=7, dets_per_image=14):
    """A small COCO JSON and per-image detections (boxes xyxy fp32, scores, classes[, keypoints]) near its ground truths: every
    category has small, medium and large ground truths, some crowd, and scores repeat."""
    rng = np.random.default_rng(seed)
    image_ids = [11 + 3 * i for i in range(n_images)]
    cat_ids = [2 + 5 * k for k in range(n_cats)]
    anns, dets = [], []
    for i, img in enumerate(image_ids):
        g = random_boxes_xywh(rng, gts_per_image)
        gc = rng.integers(0, n_cats, size=gts_per_image)
        gc[:n_cats] = np.arange(n_cats)
        for j in range(gts_per_image):
            a = dict(image_id=img, category_id=cat_ids[gc[j]], bbox=g[j].tolist(), iscrowd=int(rng.random() < 0.15), area=float(g[j, 2] * g[j, 3] * 0.8))
            if keypoints:
                v = rng.integers(0, 3, size=keypoints)
                pts = np.stack([g[j, 0] + rng.random(keypoints) * g[j, 2], g[j, 1] + rng.random(keypoints) * g[j, 3], v], axis=1)
                pts[v == 0, :2] = 0
                a["keypoints"], a["num_keypoints"] = np.round(pts, 2).reshape(-1).tolist(), int((v > 0).sum())
            anns.append(a)
        src = rng.integers(0, gts_per_image, size=dets_per_image)
        b = jitter_xyxy(rng, g[src], 5.0)
        c = np.where(rng.random(dets_per_image) < 0.8, gc[src], rng.integers(0, n_cats, size=dets_per_image)).astype(np.int64)
        s = (rng.integers(1, 40, size=dets_per_image) / 40.0).astype(np.float32)
        d = dict(boxes=b, scores=s, classes=c)
        if keypoints:
            kp = np.zeros((dets_per_image, keypoints, 3), dtype=np.float32)
            for r in range(dets_per_image):
                gk = np.array(anns[len(anns) - gts_per_image + src[r]]["keypoints"]).reshape(-1, 3)
                kp[r, :, :2] = np.where(gk[:, 2:3] > 0, gk[:, :2], g[src[r], :2] + g[src[r], 2:] / 2) + rng.normal(0, 0.04 * np.sqrt(g[src[r], 2] * g[src[r], 3]), size=(keypoints, 2)) + 0.5
                kp[r, :, 2] = rng.random(keypoints)
            d["keypoints"] = kp
        dets.append(d)
    return coco_json(image_ids, cat_ids, anns), image_ids, dets


def register(osr, tmp_path, gt, tag):
    from openset_rcnn_amd.host import datasets as D
    path = os.path.join(str(tmp_path), f"{tag}.json")
    with open(path, "w") as f:
        json.dump(gt, f)
    name = f"coco_{tmp_path.name}_{tag}"
    if name not in D.DatasetCatalog:
        D.register_coco_instances(name, {}, path, str(tmp_path))
    return name


def instances(osr, d, device="cpu"):
    from openset_rcnn_amd.host.structures import Boxes, Instances
    inst = Instances((480, 640), pred_boxes=Boxes(torch.from_numpy(d["boxes"]).to(device)), scores=torch.from_numpy(d["scores"]).to(device),
                     pred_classes=torch.from_numpy(d["classes"]).to(device))
    if "keypoints" in d:
        inst.pred_keypoints = torch.from_numpy(d["keypoints"]).to(device)
    return inst
