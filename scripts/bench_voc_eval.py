"""PascalVOCDetectionEvaluator (host/evaluation.py, csrc/osr_voc_eval.hip) on a synthetic set shaped like a VOC-COCO test split:
10 000 images, 81 class names of which 20 are known, about 7 objects and 100 detections per image, batches of 16.

Reported, each over --reps repetitions (median / min / max): the device-event time of ops.voc_match per batch (the memset and the
launch); the host clock of everything `process` does for the whole set (padding, the launches) until its last call returns and
until the device is idle; `evaluate()` without an output_dir as one wall time, and split into the one copy, the accumulation from the
flags, the rebuilding of the text records and the writing of the <class>.txt files. For comparison the numpy path (CPU tensors:
`process` with its per-image copies and text records, `evaluate` with voc_eval) in the same run on the first --numpy-images images,
scaled linearly to the set by images and labelled as scaled; on that subset the device path's results must equal the numpy path's
with kind="stable". Nothing else is asserted in advance. Writes profiles/voc_eval_line.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

DEV = "cuda:0"


def make_set(rng, images, names, known, dets):
    """-> (annotations, image ids, per image dict(boxes xyxy fp32, scores, classes)). Objects per image: 2 .. 12, sides 8 .. 300 px,
    half of them of a known class and half "unknown", one in twenty difficult; detections: jittered copies of the image's objects,
    seven in ten with the source's class, the rest a random known class or "unknown"."""
    C = len(names)
    ids = [f"{i:06d}" for i in range(images)]
    annos, out = {}, []
    for im in ids:
        g = int(rng.integers(2, 13))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), size=(g, 2)))
        xy = rng.uniform(0, 1, size=(g, 2)) * (np.array([500, 375]) - wh).clip(min=1) + 1
        gc = np.where(rng.random(g) < 0.5, rng.integers(0, known, size=g), C - 1)
        box = np.rint(np.concatenate([xy, xy + wh], axis=1)).astype(np.int64)
        annos[im] = [dict(name=names[int(c)], difficult=int(rng.random() < 0.05), bbox=b.tolist()) for c, b in zip(gc, box)]
        src = rng.integers(0, g, size=dets)
        noise = rng.normal(0, 0.08, size=(dets, 4)) * np.concatenate([wh[src], wh[src]], axis=1)
        b = (box[src] - [1, 1, 0, 0] + noise).astype(np.float32)
        other = np.where(rng.random(dets) < 0.7, rng.integers(0, known, size=dets), C - 1)
        c = np.where(rng.random(dets) < 0.7, gc[src], other).astype(np.int64)
        out.append(dict(boxes=b, scores=rng.random(dets).astype(np.float32), classes=c))
    return annos, ids, out


def spread(values, unit="s", digits=3):
    return {f"median_{unit}": round(statistics.median(values), digits), f"min_{unit}": round(min(values), digits), f"max_{unit}": round(max(values), digits),
            "n": len(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voc_eval_line.json"))
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--names", type=int, default=81)
    ap.add_argument("--known", type=int, default=20)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-images", type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voc_eval.py measures on the GPU; none found")
    ge.load_package()
    from openset_rcnn_amd.host import evaluation as E, ops
    from openset_rcnn_amd.host.structures import Boxes, Instances
    images, batch = args.images, args.batch
    names = [f"known{i}" for i in range(args.known)] + [f"unseen{i}" for i in range(args.names - args.known - 1)] + [E.UNKNOWN_NAME]
    annos, ids, per_image = make_set(np.random.default_rng(0), images, names, args.known, args.dets)

    def outputs_on(device, upto):
        return [dict(instances=Instances((375, 500), pred_boxes=Boxes(torch.from_numpy(d["boxes"]).to(device)), scores=torch.from_numpy(d["scores"]).to(device),
                                         pred_classes=torch.from_numpy(d["classes"]).to(device))) for d in per_image[:upto]]
    outputs = outputs_on(DEV, images)
    inputs = [dict(image_id=im) for im in ids]
    ev = E.PascalVOCDetectionEvaluator("", "", names, args.known, annotations=annos, image_ids=ids)

    def process_all(e, outs, upto):
        for lo in range(0, upto, batch):
            e.process(inputs[lo:min(lo + batch, upto)], outs[lo:min(lo + batch, upto)])

    t0 = time.perf_counter()
    ev.process(inputs[:batch], outputs[:batch])  # warm-up: the table and its upload, the code object, the allocator
    torch.cuda.synchronize()
    table_s = time.perf_counter() - t0
    marks, real = [], ops.voc_match

    def timed(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(*a, **kw)
        e1.record()
        marks.append((e0, e1))
        return r
    launches, enqueue, idle, whole, copy, accumulate, records, files = [], [], [], [], [], [], [], []
    results = None
    for _ in range(args.reps):
        # pass A: process, then evaluate() as its caller sees it
        ev.reset()
        process_all(ev, outputs, images)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results = ev.evaluate()
        whole.append(time.perf_counter() - t0)
        # pass B: process under device events, then evaluate()'s steps one by one
        ev.reset()
        del marks[:]
        ops.voc_match = timed
        try:
            t0 = time.perf_counter()
            process_all(ev, outputs, images)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        finally:
            ops.voc_match = real
        if [kind for kind, _ in ev._segments] != ["device"] * ((images + batch - 1) // batch):
            raise SystemExit(f"the device path was not taken: {ev._host_reason}")
        launches += [e0.elapsed_time(e1) for e0, e1 in marks]
        enqueue.append(t1 - t0)
        idle.append(t2 - t0)
        t0 = time.perf_counter()
        segments = ev._host_segments()
        t1 = time.perf_counter()
        again = ev.accumulate_from_flags([c for _, c in segments])
        t2 = time.perf_counter()
        predictions = ev._records(segments)
        t3 = time.perf_counter()
        with tempfile.TemporaryDirectory() as d:
            for cls_id, name in enumerate(names):
                with open(os.path.join(d, name + ".txt"), "w") as f:
                    f.write("\n".join(predictions.get(cls_id, [""])))
            t4 = time.perf_counter()
        if json.dumps(again) != json.dumps(results):
            raise SystemExit("two evaluations of the same detections differ")
        copy.append(t1 - t0), accumulate.append(t2 - t1), records.append(t3 - t2), files.append(t4 - t3)
    # does process() make the host wait for the device? torch reports synchronising calls when asked to
    sync_warnings = None
    try:
        ev.reset()
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            process_all(ev, outputs, 8 * batch)
        sync_warnings = sum("synchroniz" in str(w.message).lower() for w in caught)
    except Exception as e:  # (a build without the debug mode)
        sync_warnings = f"not checked: {e}"
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    res = dict(gpu=torch.cuda.get_device_name(0), images=images, class_names=len(names), known=args.known, detections_per_image=args.dets,
               ground_truths=int(sum(len(v) for v in annos.values())), batch=batch, batches=(images + batch - 1) // batch, repetitions=args.reps,
               first_batch_with_table_host_s=round(table_s, 3),
               voc_match_per_batch=dict(spread(launches, "ms", 4), clock="device events"),
               process=dict(until_the_last_call_returns=spread(enqueue), until_the_device_is_idle=spread(idle), clock="host clock",
                            synchronising_calls_torch_reported_in_8_batches=sync_warnings),
               evaluate_without_output_dir=dict(spread(whole), clock="host clock"),
               evaluate_steps=dict(one_copy=spread(copy), accumulate_from_flags=spread(accumulate), rebuild_text_records=spread(records),
                                   write_class_files=spread(files), clock="host clock"),
               figures=results)
    # the numpy path on the first images, in the same run
    sub = min(args.numpy_images, images)
    sub_annos, sub_ids = {im: annos[im] for im in ids[:sub]}, ids[:sub]
    cpu_outputs = outputs_on("cpu", sub)
    ref = E.PascalVOCDetectionEvaluator("", "", names, args.known, annotations=sub_annos, image_ids=sub_ids)
    t0 = time.perf_counter()
    process_all(ref, cpu_outputs, sub)
    t1 = time.perf_counter()
    ref_results = ref.evaluate()
    t2 = time.perf_counter()
    stable = E.PascalVOCDetectionEvaluator("", "", names, args.known, annotations=sub_annos, image_ids=sub_ids, sort_kind="stable")
    stable._segments = ref._segments
    stable_results = stable.evaluate()
    part = E.PascalVOCDetectionEvaluator("", "", names, args.known, annotations=sub_annos, image_ids=sub_ids)
    process_all(part, outputs, sub)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    part_results = part.evaluate()
    t4 = time.perf_counter()
    equal = json.dumps(part_results) == json.dumps(stable_results)
    scale = images / sub
    res["numpy_path"] = dict(subset_images=sub, process_s=round(t1 - t0, 2), evaluate_s=round(t2 - t1, 2), clock="host clock", scale=round(scale, 3),
                             process_scaled_linearly_to_the_set_s=round((t1 - t0) * scale, 1), evaluate_scaled_linearly_to_the_set_s=round((t2 - t1) * scale, 1),
                             device_evaluate_on_the_subset_s=round(t4 - t3, 3), figures_default_ties=ref_results, figures_stable_ties=stable_results,
                             device_figures_on_the_subset=part_results, subset_results_equal_to_device_path=bool(equal))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not equal:
        raise SystemExit("the device path's results differ from the numpy path's (stable ties) on the subset")


if __name__ == "__main__":
    main()
