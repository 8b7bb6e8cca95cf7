"""LVISEvaluator (host/lvis_evaluation.py, csrc/osr_lvis_eval.hip) on a synthetic set shaped like LVIS v1 val: 19 809 images, 1203
categories (337 rare, 461 common, 405 frequent, drawn with a long tail), about 12 ground truths and 300 detections per image, per image
about four negative categories and a not-exhaustive mark on one positive category in ten (lengths from memory of the v1 val JSON), in
batches of 16.

Reported over --reps repetitions of the whole set (median, min, max): the device-event time of ops.lvis_match per batch (the memsets
and the two launches), the host clock of everything `process` does for the set (padding, the tables' upload, the launches), and of
`evaluate` split into the one copy and the accumulation from the flags; the records + results file are written once. For comparison
the numpy LVISEval.evaluate() (the per-image half that the kernels replace) on the first --slice images, scaled to the set by images,
and whether its precision equals the device path's on that slice. Nothing is asserted in advance. Writes profiles/lvis_eval_line.json
(or --out)."""
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
FREQUENCY = [("r", 337), ("c", 461), ("f", 405)]


def say(msg):
    print(f"[bench_lvis_eval] {msg}", file=sys.stderr, flush=True)


def make_set(rng, images, cats, dets):
    """-> (LVIS JSON dict, boxes (images, dets, 4) fp32 xyxy, scores (images, dets), classes (images, dets)). Ground truths per image:
    1 .. 23 (12 on average), sides 8 .. 300 px, categories by weight (a frequent one 100x a rare one); detections: jittered copies of
    the image's ground truths, with the right class three times in five, a class the image evaluates one time in five, any class else."""
    freq = [f for f, n in FREQUENCY for _ in range(n)]
    freq = (freq * (cats // len(freq) + 1))[:cats]
    weight = np.array([{"r": 1.0, "c": 10.0, "f": 100.0}[f] for f in freq])
    weight /= weight.sum()
    gt = dict(images=[], categories=[dict(id=k + 1, name=f"c{k}", frequency=freq[k]) for k in range(cats)], annotations=[])
    boxes, scores = np.zeros((images, dets, 4), dtype=np.float32), rng.random((images, dets)).astype(np.float32)
    classes = np.zeros((images, dets), dtype=np.int64)
    for i in range(images):
        g = int(rng.integers(1, 24))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), size=(g, 2)))
        xy = rng.uniform(0, 1, size=(g, 2)) * (np.array([1333, 800]) - wh).clip(min=1)
        gc = rng.choice(cats, size=g, p=weight)
        positive = np.unique(gc)
        negative = np.setdiff1d(rng.choice(cats, size=int(rng.integers(0, 9)), p=weight), positive)
        gt["images"].append(dict(id=i + 1, coco_url=f"http://images.cocodataset.org/val2017/{i:012d}.jpg", height=800, width=1333,
                                 neg_category_ids=(negative + 1).tolist(), not_exhaustive_category_ids=(positive[rng.random(len(positive)) < 0.1] + 1).tolist()))
        for j in range(g):
            gt["annotations"].append(dict(id=len(gt["annotations"]) + 1, image_id=i + 1, category_id=int(gc[j]) + 1, bbox=[*xy[j].tolist(), *wh[j].tolist()],
                                          area=float(wh[j, 0] * wh[j, 1] * 0.7)))
        src = rng.integers(0, g, size=dets)
        noise = rng.normal(0, 0.08, size=(dets, 4)) * np.concatenate([wh[src], wh[src]], axis=1)
        boxes[i] = np.concatenate([xy[src], xy[src] + wh[src]], axis=1) + noise
        evaluated = np.concatenate([positive, negative])
        u = rng.random(dets)
        classes[i] = np.where(u < 0.6, gc[src], np.where(u < 0.8, evaluated[rng.integers(0, len(evaluated), size=dets)], rng.integers(0, cats, size=dets)))
    return gt, boxes, scores, classes


def spread(values, digits=4):
    return dict(median=round(statistics.median(values), digits), min=round(min(values), digits), max=round(max(values), digits), reps=len(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lvis_eval_line.json"))
    ap.add_argument("--images", type=int, default=19809)
    ap.add_argument("--cats", type=int, default=1203)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slice", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lvis_eval.py measures on the GPU; none found")
    ge.load_package()
    from openset_rcnn_amd.host import datasets as D, lvis_evaluation as LE, ops
    from openset_rcnn_amd.host.structures import Boxes, Instances
    images, batch = args.images, args.batch
    gt, boxes, scores, classes = make_set(np.random.default_rng(0), images, args.cats, args.dets)
    say(f"set: {images} images, {len(gt['annotations'])} ground truths")
    res = dict(gpu=torch.cuda.get_device_name(0), images=images, categories=args.cats, detections_per_image=args.dets, ground_truths=len(gt["annotations"]),
               negatives=sum(len(im["neg_category_ids"]) for im in gt["images"]), not_exhaustive=sum(len(im["not_exhaustive_category_ids"]) for im in gt["images"]),
               batch=batch, batches=(images + batch - 1) // batch)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "lvis.json")
        with open(path, "w") as f:
            json.dump(gt, f)
        D.register_lvis_instances("bench_lvis", {}, path, tmp)
        ev = LE.LVISEvaluator("bench_lvis", output_dir=os.path.join(tmp, "out"))
        res["evaluated_entries"] = int(len(ev.tables.ent_cat))
        d_boxes, d_scores, d_classes = (torch.from_numpy(a).to(DEV) for a in (boxes, scores, classes))
        outputs = [dict(instances=Instances((800, 1333), pred_boxes=Boxes(d_boxes[i]), scores=d_scores[i], pred_classes=d_classes[i])) for i in range(images)]
        inputs = [dict(image_id=i + 1) for i in range(images)]
        marks, real = [], ops.lvis_match

        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real(*a, **kw)
            e1.record()
            marks.append((e0, e1))
            return r
        ev.process(inputs[:batch], outputs[:batch])  # warm-up
        torch.cuda.synchronize()
        per_batch, process_s, copy_s, accumulate_s = [], [], [], []
        ops.lvis_match = timed
        try:
            for rep in range(args.reps):
                ev.reset()
                del marks[:]
                t0 = time.perf_counter()
                for lo in range(0, images, batch):
                    ev.process(inputs[lo:lo + batch], outputs[lo:lo + batch])
                torch.cuda.synchronize()
                process_s.append(time.perf_counter() - t0)
                per_batch.append(statistics.median(e0.elapsed_time(e1) for e0, e1 in marks))
                t0 = time.perf_counter()
                part = ev._fetch()
                t1 = time.perf_counter()
                precision = ev._accumulate_from_flags([part], None)
                copy_s.append(t1 - t0)
                accumulate_s.append(time.perf_counter() - t1)
                say(f"rep {rep}: process {process_s[-1]:.2f} s, lvis_match {per_batch[-1]:.4f} ms per batch, copy {copy_s[-1]:.2f} s, accumulate {accumulate_s[-1]:.2f} s")
        finally:
            ops.lvis_match = real
        res["lvis_match_per_batch_ms"] = dict(spread(per_batch), of="each repetition's median over its batches", clock="device events")
        res["process_host_s"] = dict(spread(process_s, 3), clock="host clock")
        res["evaluate_host_s"] = dict(one_copy=spread(copy_s, 3), accumulate=spread(accumulate_s, 3), clock="host clock")
        res["figures"] = {k: round(v, 3) for k, v in LE.lvis_figures(precision, ev.tables.frequency).items()}
        res["listed_detections"] = int((part["rank"] >= 0).sum())
        t0 = time.perf_counter()
        records = ev._records_from(part)
        os.makedirs(ev.output_dir, exist_ok=True)
        with open(os.path.join(ev.output_dir, ev.RESULTS_FILE), "w") as f:
            json.dump(records, f)
        res["evaluate_host_s"]["records_and_results_file"] = dict(seconds=round(time.perf_counter() - t0, 3), reps=1)
        say(f"results file: {res['evaluate_host_s']['records_and_results_file']['seconds']} s")
        # the numpy per-image half on a slice
        ids = [i + 1 for i in range(min(args.slice, images))]
        ref = LE.LVISEval(gt, records[:len(ids) * args.dets], img_ids=ids)
        t0 = time.perf_counter()
        ref.evaluate()
        dt = time.perf_counter() - t0
        ref.accumulate()
        res["numpy_evaluate"] = dict(slice_images=len(ids), slice_s=round(dt, 3), scaled_to_set_s=round(dt * images / len(ids), 1), clock="host clock",
                                     slice_precision_equal_to_device_path=bool(np.array_equal(ref.eval["precision"], ev._accumulate_from_flags([part], ids))))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
