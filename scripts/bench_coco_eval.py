"""COCOEvaluator (host/coco_evaluation.py, csrc/osr_coco_eval.hip) on a synthetic set the size of COCO val2017: 5000 images, 100
detections and about 7 ground truths per image, in batches of 16. Two sets: "bbox" with 80 categories (the detection models), and
"keypoints" with the one person category and 17 keypoints (Keypoint R-CNN: both tasks per batch).

Reported, per set: the median / min / max device-event time of ops.coco_match per batch and task (the two memsets and the launch),
the host clock of everything `process` does for the whole set (padding, the tables' upload, the launches), and of `evaluate` split
into the one copy, the records + results file, and the accumulation from the flags per task. For comparison the numpy
COCOeval.evaluate() (the per-image half that the kernel replaces) on the first --slice images, scaled to the set by images.
Nothing is asserted in advance. Writes profiles/coco_eval_line.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

DEV = "cuda:0"


def make_set(rng, images, cats, dets, kp):
    """-> (COCO JSON dict, per image (boxes xyxy fp32, scores, classes[, keypoints])). Ground truths per image: 1 .. 13 (7 on
    average), sides 8 .. 300 px; detections: jittered copies of the image's ground truths with the right class four times in five."""
    gt = dict(images=[dict(id=i + 1, file_name=f"{i}.jpg", height=800, width=1333) for i in range(images)],
              categories=[dict(id=k + 1, name=f"c{k}") for k in range(cats)], annotations=[])
    out = []
    for i in range(images):
        g = int(rng.integers(1, 14))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), size=(g, 2)))
        xy = rng.uniform(0, 1, size=(g, 2)) * (np.array([1333, 800]) - wh).clip(min=1)
        gc = rng.integers(0, cats, size=g)
        pts = None
        if kp:
            v = rng.integers(0, 3, size=(g, kp))
            pts = np.concatenate([xy[:, None] + rng.uniform(0, 1, size=(g, kp, 2)) * wh[:, None], v[..., None]], axis=2)
            pts[v == 0, :2] = 0
        for j in range(g):
            a = dict(id=len(gt["annotations"]) + 1, image_id=i + 1, category_id=int(gc[j]) + 1, bbox=[*xy[j].tolist(), *wh[j].tolist()],
                     area=float(wh[j, 0] * wh[j, 1] * 0.7), iscrowd=int(rng.random() < 0.03))
            if kp:
                a["keypoints"], a["num_keypoints"] = pts[j].reshape(-1).tolist(), int((pts[j, :, 2] > 0).sum())
            gt["annotations"].append(a)
        src = rng.integers(0, g, size=dets)
        noise = rng.normal(0, 0.08, size=(dets, 4)) * np.concatenate([wh[src], wh[src]], axis=1)
        b = (np.concatenate([xy[src], xy[src] + wh[src]], axis=1) + noise).astype(np.float32)
        c = np.where(rng.random(dets) < 0.8, gc[src], rng.integers(0, cats, size=dets)).astype(np.int64)
        d = dict(boxes=b, scores=rng.random(dets).astype(np.float32), classes=c)
        if kp:
            k = pts[src].astype(np.float32)
            k[..., :2] += rng.normal(0, 0.05, size=(dets, kp, 2)).astype(np.float32) * np.sqrt(wh[src, 0] * wh[src, 1])[:, None, None].astype(np.float32) + 0.5
            k[..., 2] = rng.random((dets, kp))
            d["keypoints"] = k
        out.append(d)
    return gt, out


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), calls=len(ms))


def run_set(tag, images, cats, dets, kp, batch, slice_images, tmp):
    from openset_rcnn_amd.host import coco_evaluation as CE, datasets as D, ops
    from openset_rcnn_amd.host.structures import Boxes, Instances
    rng = np.random.default_rng(0)
    gt, per_image = make_set(rng, images, cats, dets, kp)
    path = os.path.join(tmp, f"{tag}.json")
    with open(path, "w") as f:
        json.dump(gt, f)
    name = f"bench_coco_{tag}"
    D.register_coco_instances(name, {}, path, tmp)
    ev = CE.COCOEvaluator(name, output_dir=os.path.join(tmp, tag))
    dev = [{k: torch.from_numpy(v).to(DEV) for k, v in d.items()} for d in per_image]

    def instances(d):
        inst = Instances((800, 1333), pred_boxes=Boxes(d["boxes"]), scores=d["scores"], pred_classes=d["classes"])
        if kp:
            inst.pred_keypoints = d["keypoints"]
        return inst
    outputs = [dict(instances=instances(d)) for d in dev]
    inputs = [dict(image_id=i + 1) for i in range(images)]
    marks, real = [], ops.coco_match

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(*a, **kw)
        e1.record()
        marks.append(("keypoints" if kw.get("keypoints") is not None else "bbox", e0, e1))
        return r
    ev.process(inputs[:batch], outputs[:batch])  # warm-up
    torch.cuda.synchronize()
    ev.reset()
    ops.coco_match = timed
    try:
        t0 = time.perf_counter()
        for lo in range(0, images, batch):
            ev.process(inputs[lo:lo + batch], outputs[lo:lo + batch])
        torch.cuda.synchronize()
        process_s = time.perf_counter() - t0
    finally:
        ops.coco_match = real
    res = dict(images=images, categories=cats, detections_per_image=dets, ground_truths=len(gt["annotations"]), keypoints=kp, batch=batch,
               batches=(images + batch - 1) // batch, tasks=list(ev.tasks), process_host_s=round(process_s, 3))
    for task in ev.tasks:
        res[f"coco_match_{task}_per_batch"] = dict(stats([e0.elapsed_time(e1) for t, e0, e1 in marks if t == task]), clock="device events")
    # evaluate(), step by step on the host clock
    t0 = time.perf_counter()
    part = ev._fetch()
    t1 = time.perf_counter()
    records = ev._records_from(part)
    os.makedirs(ev.output_dir, exist_ok=True)
    with open(os.path.join(ev.output_dir, ev.RESULTS_FILE), "w") as f:
        json.dump(records, f)
    t2 = time.perf_counter()
    res["evaluate_host_s"] = dict(one_copy=round(t1 - t0, 3), records_and_results_file=round(t2 - t1, 3), clock="host clock")
    figures = {}
    for task in ev.tasks:
        t3 = time.perf_counter()
        precision, recall, p = ev._accumulate_from_flags([part], task, None)
        figures[task] = CE.derive_coco_results(CE.summarize_stats(precision, recall, p), precision, task, None)
        res["evaluate_host_s"][f"accumulate_{task}"] = round(time.perf_counter() - t3, 3)
    res["figures"] = {t: {k: round(v, 3) for k, v in f.items()} for t, f in figures.items()}
    # the numpy per-image half on a slice
    ids = [i + 1 for i in range(min(slice_images, images))]
    chosen = set(ids)
    sl = [r for r in records if r["image_id"] in chosen]
    res["numpy_evaluate"] = dict(slice_images=len(ids), clock="host clock")
    for task in ev.tasks:
        ref = CE.COCOeval(gt, sl, task, img_ids=ids, kpt_oks_sigmas=None, max_dets=ev.max_dets[task])
        t4 = time.perf_counter()
        ref.evaluate()
        dt = time.perf_counter() - t4
        ref.accumulate()
        part_dev = ev._accumulate_from_flags([part], task, ids)
        res["numpy_evaluate"][task] = dict(slice_s=round(dt, 3), scaled_to_set_s=round(dt * images / len(ids), 1),
                                           slice_precision_equal_to_device_path=bool(np.array_equal(ref.eval["precision"], part_dev[0])))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_line.json"))
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--slice", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coco_eval.py measures on the GPU; none found")
    ge.load_package()
    res = dict(gpu=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as tmp:
        res["bbox_set"] = run_set("bbox", args.images, 80, args.dets, 0, args.batch, args.slice, tmp)
        res["keypoint_set"] = run_set("keypoints", args.images, 1, args.dets, 17, args.batch, args.slice, tmp)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
