"""Shared by the open-set VOC evaluator's device tests: a seeded small dataset (annotations with known, renamed-to-unknown and
difficult objects, duplicate boxes, images without objects) with detections as fp32 arrays, the padded-list form osr_voc_match reads,
and the numpy specification's outputs as per-batch chunks. Coordinates lie on a 0.05 grid, so exact .x5 rounding ties occur; scores
lie on a 0.0005 grid, so rounded scores tie and raw scores straddle a rounding boundary."""
import json
from types import SimpleNamespace

import numpy as np

UNKNOWN = "unknown"


def class_names(num_known=4, num_unseen=3):
    """Known names, then names of unseen categories (which never occur in an annotation: they are renamed), then "unknown"."""
    return [f"known{i}" for i in range(num_known)] + [f"unseen{i}" for i in range(num_unseen)] + [UNKNOWN]


def seeded_voc(seed, num_images=40, num_known=4, num_unseen=3, max_objects=7, max_dets=30):
    """-> (annos {id: [dict(name, difficult, bbox)]}, image_ids, class names, num_known, dets [dict(boxes, scores, classes)])."""
    rng = np.random.default_rng(seed)
    names = class_names(num_known, num_unseen)
    C = len(names)
    ids = [f"im{i:03d}" for i in range(num_images)]
    annos, dets = {}, []
    for i, im in enumerate(ids):
        objs = []
        for _ in range(0 if i % 9 == 4 else int(rng.integers(1, max_objects + 1))):
            x0, y0 = int(rng.integers(1, 300)), int(rng.integers(1, 200))
            w, h = int(rng.integers(8, 120)), int(rng.integers(8, 120))
            cls = int(rng.integers(0, num_known)) if rng.random() < 0.65 else C - 1
            objs.append(dict(name=names[cls], difficult=int(rng.random() < 0.2), bbox=[x0, y0, x0 + w, y0 + h]))
            if rng.random() < 0.2:  # the same box once more: under the same name (a duplicate), or as an unknown object next to a known one
                twin = dict(objs[-1], difficult=0)
                if rng.random() < 0.5:
                    twin["name"] = names[C - 1] if cls != C - 1 else names[0]
                objs.append(twin)
        annos[im] = objs
        m = 0 if i % 11 == 7 else int(rng.integers(1, max_dets + 1))
        boxes, classes = np.zeros((m, 4), dtype=np.float64), np.zeros(m, dtype=np.int64)
        for d in range(m):
            if objs and rng.random() < 0.8:
                o = objs[int(rng.integers(0, len(objs)))]
                b = np.array(o["bbox"], dtype=np.float64) - [1, 1, 0, 0]  # the loader's 0-based corner
                jitter = rng.choice([0.0, 2.0, 12.0, 40.0])
                boxes[d] = b + rng.uniform(-jitter, jitter, size=4)
                own = names.index(o["name"])
                classes[d] = own if rng.random() < 0.6 else int(rng.integers(0, C))
            else:
                x0, y0 = rng.uniform(0, 300), rng.uniform(0, 200)
                boxes[d] = [x0, y0, x0 + rng.uniform(5, 120), y0 + rng.uniform(5, 120)]
                classes[d] = int(rng.integers(0, C))
        boxes = (np.rint(boxes * 20.0) / 20.0).astype(np.float32)                            # the 0.05 grid
        scores = (rng.integers(1, 2000, size=m) / 2000.0).astype(np.float32)                 # the 0.0005 grid
        if m > 3:
            scores[1] = scores[0]                                                            # an exact tie,
            scores[2] = np.float32((np.rint(float(scores[0]) * 1000.0) + 0.4) / 1000.0)      # and a raw score that only ties once rounded
        dets.append(dict(boxes=boxes, scores=scores, classes=classes))
    return annos, ids, names, num_known, dets


def padded(dets, cap):
    """Per-image detections -> the engines' padded lists (boxes, scores, classes, counts)."""
    n = len(dets)
    boxes, scores = np.zeros((n, cap, 4), dtype=np.float32), np.zeros((n, cap), dtype=np.float32)
    classes, counts = np.full((n, cap), -1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    for i, d in enumerate(dets):
        m = len(d["scores"])
        boxes[i, :m], scores[i, :m], classes[i, :m], counts[i] = d["boxes"], d["scores"], d["classes"], m
    return boxes, scores, classes, counts


def cap_of(dets):
    return max((max(len(d["scores"]) for d in dets) + 7) // 8 * 8, 8)


def table_of(annos, ids, names):
    from openset_rcnn_amd.host.evaluation import VocGroundTruthTable
    return VocGroundTruthTable(annos, ids, names)


def reference_chunks(annos, ids, names, dets, batches):
    """voc_match_reference per batch -> the chunks accumulate_from_flags reads (flat arrays over the rows that exist, arrival order)."""
    from openset_rcnn_amd.host.evaluation import voc_match_reference
    tb = table_of(annos, ids, names)
    chunks = []
    for lo, hi in batches:
        boxes, scores, classes, counts = padded(dets[lo:hi], cap_of(dets[lo:hi]))
        index = np.array([tb.index[im] for im in ids[lo:hi]], dtype=np.int32)
        flags, milli, _, _, status = voc_match_reference(boxes, scores, classes, counts, index, len(names), tb.img_off, tb.box, tb.cls, tb.difficult)
        assert status[0] == 0
        exists = np.arange(boxes.shape[1])[None, :] < counts[:, None]
        chunks.append(dict(classes=classes[exists], flags=flags[exists], milli=milli[exists]))
    return chunks


def device_match(osr, device, lists, index, num_classes, tb, ovthresh=0.5):
    """ops.voc_match on padded lists -> (flags, milli, match, deci, status) as numpy arrays."""
    import torch
    boxes, scores, classes, counts = lists
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)  # noqa: E731
    out = osr.ops.voc_match(t(boxes, np.float32), t(scores, np.float32), t(classes, np.int64), t(counts, np.int32), t(index, np.int32), num_classes,
                            t(tb.img_off, np.int32), t(tb.box, np.float64).reshape(-1, 4), t(tb.cls, np.int32), t(tb.difficult, np.uint8), tb.max_per_image,
                            ovthresh, want_match=True, want_deci=True)
    return tuple(o.cpu().numpy() for o in out)


def instances(osr, d, device, plain=False):
    """One image's detections as `Instances`, or as the bare namespaces tests/trained_parity.py hands over."""
    import torch
    b, s, c = (torch.from_numpy(np.ascontiguousarray(d[k])).to(device) for k in ("boxes", "scores", "classes"))
    if plain:
        return SimpleNamespace(pred_boxes=SimpleNamespace(tensor=b), scores=s, pred_classes=c)
    from openset_rcnn_amd.host.structures import Boxes, Instances
    inst = Instances((480, 640))
    inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(b), s, c
    return inst


def run_evaluator(osr, annos, ids, names, num_known, dets, batches, devices, output_dir=None, sort_kind=None, plain=False):
    """The evaluator over `batches` [(lo, hi)] with batch b's tensors on devices[b] -> (evaluator, results, per-class detail)."""
    from openset_rcnn_amd.host.evaluation import PascalVOCDetectionEvaluator
    ev = PascalVOCDetectionEvaluator("", "", names, num_known, output_dir=output_dir, annotations=annos, image_ids=ids, sort_kind=sort_kind)
    for (lo, hi), device in zip(batches, devices):
        ev.process([dict(image_id=im) for im in ids[lo:hi]], [dict(instances=instances(osr, d, device, plain)) for d in dets[lo:hi]])
    detail = {}
    return ev, ev.evaluate(detail=detail), detail


def same_results(a, b):
    """Two result dicts: the same keys in the same order with the same values (mAP is NaN when a class name without ground truth has
    detections, and NaN has to equal NaN here)."""
    return json.dumps(a) == json.dumps(b)


def same_detail(a, b):
    """Two {class id: voc_eval's return value}: every array and number equal bit for bit."""
    if sorted(a) != sorted(b):
        return False
    for c in a:
        for x, y in zip(a[c], b[c]):
            if (x is None) != (y is None) or (x is not None and not np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)):
                return False
    return True
