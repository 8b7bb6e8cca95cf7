"""OpensetCOCOEvaluator (host/os_coco_evaluation.py, csrc/osr_os_coco_eval.hip) on a synthetic set shaped like one GraspNet test
split: 7680 images, 88 categories of which 28 are known, about 10 ground truths and 100 detections per image, batches of 16.

Reported: the median / min / max device-event time of ops.os_coco_match per batch (the three memsets and the launch), the host
clock of everything `process` does for the whole set (padding, the table's upload, the launches), and of `evaluate` split into the
one copy, the accumulation from the flags and the summary. For comparison the numpy path, OpensetCOCOEval.evaluate() + accumulate(),
in the same run on the first --numpy-images images (records rebuilt from the fetched arrays), scaled linearly to the set by images
and labelled as scaled; on that subset the device path's arrays must equal numpy's. Nothing else is asserted in advance.
Writes profiles/os_coco_eval_line.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

DEV = "cuda:0"
UNKNOWN = 1000


def make_set(rng, images, cats, known, dets):
    """-> (COCO JSON dict, known names, contiguous -> dataset id, per image (boxes xyxy fp32, scores, classes)). Ground truths per
    image: 4 .. 16 (10 on average), sides 8 .. 300 px; detections: jittered copies of the image's ground truths, seven in ten with the
    source's class (1000 when its category is not known), the rest a random known class or 1000."""
    gt = dict(images=[dict(id=i + 1, file_name=f"{i}.png", height=720, width=1280) for i in range(images)],
              categories=[dict(id=k + 1, name=f"c{k}") for k in range(cats)], annotations=[])
    known_cats = np.sort(rng.permutation(cats)[:known])
    is_known = np.zeros(cats, dtype=bool)
    is_known[known_cats] = True
    out = []
    for i in range(images):
        g = int(rng.integers(4, 17))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), size=(g, 2)))
        xy = rng.uniform(0, 1, size=(g, 2)) * (np.array([1280, 720]) - wh).clip(min=1)
        gc = rng.integers(0, cats, size=g)
        for j in range(g):
            gt["annotations"].append(dict(id=len(gt["annotations"]) + 1, image_id=i + 1, category_id=int(gc[j]) + 1, bbox=[*xy[j].tolist(), *wh[j].tolist()],
                                          area=float(wh[j, 0] * wh[j, 1] * 0.7), iscrowd=int(rng.random() < 0.03)))
        src = rng.integers(0, g, size=dets)
        noise = rng.normal(0, 0.08, size=(dets, 4)) * np.concatenate([wh[src], wh[src]], axis=1)
        b = (np.concatenate([xy[src], xy[src] + wh[src]], axis=1) + noise).astype(np.float32)
        own = np.where(is_known[gc[src]], gc[src], UNKNOWN)
        other = np.where(rng.random(dets) < 0.7, known_cats[rng.integers(0, known, size=dets)], UNKNOWN)
        c = np.where(rng.random(dets) < 0.7, own, other).astype(np.int64)
        out.append(dict(boxes=b, scores=rng.random(dets).astype(np.float32), classes=c))
    return gt, [f"c{k}" for k in known_cats], {k: k + 1 for k in range(cats)}, out


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "os_coco_eval_line.json"))
    ap.add_argument("--images", type=int, default=7680)
    ap.add_argument("--cats", type=int, default=88)
    ap.add_argument("--known", type=int, default=28)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--numpy-images", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_os_coco_eval.py measures on the GPU; none found")
    ge.load_package()
    from openset_rcnn_amd.host import ops, os_coco_evaluation as OE
    from openset_rcnn_amd.host.structures import Boxes, Instances
    images, batch = args.images, args.batch
    gt, names, reverse_map, per_image = make_set(np.random.default_rng(0), images, args.cats, args.known, args.dets)
    ev = OE.OpensetCOCOEvaluator(gt, names, reverse_map)
    outputs = [dict(instances=Instances((720, 1280), pred_boxes=Boxes(torch.from_numpy(d["boxes"]).to(DEV)), scores=torch.from_numpy(d["scores"]).to(DEV),
                                        pred_classes=torch.from_numpy(d["classes"]).to(DEV))) for d in per_image]
    inputs = [dict(image_id=i + 1) for i in range(images)]
    marks, real = [], ops.os_coco_match

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(*a, **kw)
        e1.record()
        marks.append((e0, e1))
        return r
    t0 = time.perf_counter()
    ev.process(inputs[:batch], outputs[:batch])  # warm-up: the tables, the code object, the allocator
    torch.cuda.synchronize()
    tables_s = time.perf_counter() - t0
    ev.reset()
    ops.os_coco_match = timed
    try:
        t0 = time.perf_counter()
        for lo in range(0, images, batch):
            ev.process(inputs[lo:lo + batch], outputs[lo:lo + batch])
        torch.cuda.synchronize()
        process_s = time.perf_counter() - t0
    finally:
        ops.os_coco_match = real
    if len(ev._chunks) != (images + batch - 1) // batch or ev._predictions:
        raise SystemExit(f"the device path was not taken: {ev._host_reason}")
    launches = [e0.elapsed_time(e1) for e0, e1 in marks]
    res = dict(gpu=torch.cuda.get_device_name(0), images=images, categories=args.cats, known=args.known, detections_per_image=args.dets,
               ground_truths=len(gt["annotations"]), batch=batch, batches=len(ev._chunks), first_batch_with_tables_host_s=round(tables_s, 3),
               os_coco_match_per_batch=dict(spread(launches), sum_ms_for_the_set=round(sum(launches), 2), clock="device events"),
               process_host_s=round(process_s, 3))
    # evaluate(), step by step on the host clock
    t0 = time.perf_counter()
    fetched = ev._fetch()
    t1 = time.perf_counter()
    dets = OE._Detections([("device", q) for q in fetched], None)
    full = ev._accumulate_device(dets, None)
    t2 = time.perf_counter()
    figures = OE.derive_results(full.summarize())
    t3 = time.perf_counter()
    res["evaluate_host_s"] = dict(one_copy=round(t1 - t0, 3), accumulate_from_flags=round(t2 - t1, 3), summarize=round(t3 - t2, 4), clock="host clock")
    res["device_path_end_to_end_s"] = round(process_s + (t3 - t0), 3)
    res["figures"] = {k: {m: round(v, 3) for m, v in f.items()} for k, f in figures.items()}
    # the numpy path on the first images, in the same run
    ids = [i + 1 for i in range(min(args.numpy_images, images))]
    chosen = set(ids)
    records = [r for r in dets.records(reverse_map) if r["image_id"] in chosen]
    ref = OE.OpensetCOCOEval(gt, records, ev.known_ids, ev.max_dets, ids)
    t4 = time.perf_counter()
    ref.evaluate()
    t5 = time.perf_counter()
    ref.accumulate()
    t6 = time.perf_counter()
    part = ev._accumulate_device(dets, ids)
    t7 = time.perf_counter()
    equal = all(np.array_equal(part.eval_kdt[k], v) for k, v in ref.eval_kdt.items()) and all(np.array_equal(part.eval_unkdt[k], v) for k, v in ref.eval_unkdt.items())
    scale = images / len(ids)
    res["numpy_path"] = dict(subset_images=len(ids), evaluate_s=round(t5 - t4, 2), accumulate_s=round(t6 - t5, 2), clock="host clock",
                             scaled_linearly_to_the_set_s=round((t6 - t4) * scale, 1), scale=round(scale, 3),
                             device_accumulate_on_the_subset_s=round(t7 - t6, 3), subset_arrays_equal_to_device_path=bool(equal))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not equal:
        raise SystemExit("the device path's arrays differ from numpy's on the subset")


if __name__ == "__main__":
    main()
