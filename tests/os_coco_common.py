"""Shared by the open-set COCO evaluator tests: seeded open-set data in the engines' padded list form, and the numpy
OpensetCOCOEval's per-image results laid out like osr_os_coco_match's outputs (flags, rank, match)."""
import numpy as np
import torch

from tests.coco_eval_common import coco_json, jitter_xyxy, random_boxes_xywh

UNKNOWN = 1000
MAX_DETS = (10, 20, 30, 50, 100)


def names_of(gt, known_ids):
    return [c["name"] for c in gt["categories"] if c["id"] in set(known_ids)]


def records(osr, image_ids, boxes, scores, classes, counts, reverse_map):
    """The host path's records for the padded lists, row by row, and where each came from."""
    from openset_rcnn_amd.host.os_coco_evaluation import records_from_arrays
    recs, where = [], []
    for i, img in enumerate(image_ids):
        m = int(counts[i])
        recs += records_from_arrays([img] * m, boxes[i, :m], scores[i, :m], classes[i, :m], reverse_map)
        where += [(i, r) for r in range(m)]
    return recs, where


def reference_outputs(osr, gt, known_ids, image_ids, boxes, scores, classes, counts, reverse_map, max_det=100):
    """The numpy OpensetCOCOEval.evaluate() on the padded lists -> (flags (n, cap, A, 3) uint32, rank (n, cap) int32, match
    (n, cap, A, 3, T) int32 with indices into the batch's table, tables, (rows, img_off, max_img), the evaluated class)."""
    from openset_rcnn_amd.host.os_coco_evaluation import OpensetCOCOEval, OpensetGroundTruthTables
    recs, where = records(osr, image_ids, boxes, scores, classes, counts, reverse_map)
    ev = OpensetCOCOEval(gt, recs, known_ids, [max_det])
    ev.evaluate()
    tb = OpensetGroundTruthTables(gt, known_ids)
    rows, img_off, max_img = tb.batch(image_ids)
    order = np.lexsort((tb.pos, tb.slot, tb.img))
    assert np.array_equal(order, np.arange(len(order)))  # the table is sorted as the header says
    # annotation id -> index into the batch's table
    anns = sorted(gt["annotations"], key=lambda a: (tb.img_pos[a["image_id"]], tb.known_ids.index(a["category_id"]) if a["category_id"] in tb.known_ids else tb.num_known))
    flat = {a["id"]: k for k, a in enumerate(anns)}  # (sorted() is stable: annotation order within (image, slot)) -> index into the full table
    in_batch = {int(r): k for k, r in enumerate(rows)}
    T, A, I, K = len(ev.iou_thrs), len(ev.area_rng), len(ev.img_ids), len(ev.cat_ids)
    n, cap = scores.shape
    flags, rank = np.zeros((n, cap, A, 3), dtype=np.uint32), -np.ones((n, cap), dtype=np.int32)
    match = -np.ones((n, cap, A, 3, T), dtype=np.int32)
    img_index = {img: i for i, img in enumerate(image_ids)}

    def lay(i, dts, a, s, dtm, dtig):
        for d, det in enumerate(dts):
            ii, r = where[det["id"] - 1]
            assert ii == i
            rank[i, r] = d
            for t in range(T):
                if dtm[t, d]:
                    flags[i, r, a, s] |= np.uint32(1 << t)
                    match[i, r, a, s, t] = in_batch[flat[int(dtm[t, d])]]
                if dtig[t, d]:
                    flags[i, r, a, s] |= np.uint32(1 << (16 + t))

    for p, img in enumerate(ev.img_ids):
        if img not in img_index:
            continue
        i = img_index[img]
        for a in range(A):
            for k, c in enumerate(ev.cat_ids):
                e = ev.eval_imgs_kdt[(k * A + a) * I + p]
                dts = ev._sorted_dets(ev._k_dts[img, c], max_det)
                assert [d["score"] for d in dts] == e["scores"]
                for s, (mk, ik) in enumerate((("m_k", "ig_k"), ("m_ok", "ig_ok"), ("m_u", "ig_u"))):
                    lay(i, dts, a, s, e[mk], e[ik])
            e = ev.eval_imgs_unkdt[a * I + p]
            if e is not None:
                dts = ev._sorted_dets(ev._unk_dts[img], max_det)
                for s, (mk, ik) in enumerate((("m_u", "ig_u"), ("m_k", "ig_k"))):
                    lay(i, dts, a, s, e[mk], e[ik])
    return flags, rank, match, tb, (rows, img_off, max_img), ev


def device_match(osr, dev, gt, known_ids, image_ids, boxes, scores, classes, counts, reverse_map, max_det=100):
    """ops.os_coco_match on the same inputs -> (flags uint32, rank, match) as numpy arrays."""
    from openset_rcnn_amd.host.os_coco_evaluation import OpensetCOCOEval, OpensetGroundTruthTables
    tb = OpensetGroundTruthTables(gt, known_ids)
    rows, img_off, max_img = tb.batch(image_ids)
    p = OpensetCOCOEval(dict(images=[], annotations=[]), [], known_ids)
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).to(dev)  # noqa: E731
    flags, rank, match = osr.ops.os_coco_match(t(boxes, np.float32), t(scores, np.float32), t(classes, np.int64), t(counts, np.int32),
                                               t(tb.class_slots(reverse_map)), tb.num_known, t(img_off), t(tb.box[rows]), t(tb.area[rows]), t(tb.slot[rows]),
                                               t(tb.pos[rows]), t(tb.crowd[rows]), max_img, p.iou_thrs, p.area_rng, max_det, want_match=True)
    return flags.cpu().numpy().view(np.uint32), rank.cpu().numpy(), match.cpu().numpy()


def seeded_openset(seed, n_images=6, n_cats=5, n_known=3, gts_per_image=8, dets_per_image=18):
    """A small COCO JSON (annotation ids from 1, some crowd, areas that straddle the range limits) whose known categories are NOT the
    first ones, a contiguous-id map over all categories, and per-image detections near the ground truths: known classes, the unknown
    class 1000 and classes of categories that are not known (dropped), boxes on the quarter-pixel grid, scores that repeat.
    -> (gt, image_ids, known_ids, reverse_map, dets: per image dict(boxes, scores, classes))."""
    rng = np.random.default_rng(seed)
    image_ids = [11 + 3 * i for i in range(n_images)]
    cat_ids = [2 + 5 * k for k in range(n_cats)]
    known_ids = sorted(rng.permutation(cat_ids)[:n_known].tolist())
    reverse_map = dict(enumerate(cat_ids))
    anns, dets = [], []
    for img in image_ids:
        g = random_boxes_xywh(rng, gts_per_image)
        gc = rng.integers(0, n_cats, size=gts_per_image)
        gc[:n_cats] = rng.permutation(n_cats)  # every category, in no particular order
        for j in range(gts_per_image):
            anns.append(dict(image_id=img, category_id=cat_ids[gc[j]], bbox=g[j].tolist(), iscrowd=int(rng.random() < 0.15), area=float(g[j, 2] * g[j, 3] * 0.8)))
        src = rng.integers(0, gts_per_image, size=dets_per_image)
        b = jitter_xyxy(rng, g[src], 4.0)
        b[:4] = jitter_xyxy(rng, g[src[:4]], 0.0)
        c = np.where(rng.random(dets_per_image) < 0.6, gc[src], rng.integers(0, n_cats, size=dets_per_image)).astype(np.int64)
        c[rng.random(dets_per_image) < 0.3] = UNKNOWN
        s = (rng.integers(1, 24, size=dets_per_image) / 24.0).astype(np.float32)
        dets.append(dict(boxes=b, scores=s, classes=c))
    return coco_json(image_ids, cat_ids, anns), image_ids, known_ids, reverse_map, dets


def padded(dets, cap=None):
    """Per-image detections -> (boxes (n, cap, 4), scores, classes, counts); rows past the counts hold plausible values."""
    n = len(dets)
    cap = cap or max(max(len(d["scores"]) for d in dets), 1)
    rng = np.random.default_rng(99)
    boxes = jitter_xyxy(rng, random_boxes_xywh(rng, n * cap)).reshape(n, cap, 4)
    scores = (rng.integers(1, 24, size=(n, cap)) / 24.0).astype(np.float32)
    classes = rng.integers(0, 3, size=(n, cap)).astype(np.int64)
    counts = np.zeros(n, dtype=np.int32)
    for i, d in enumerate(dets):
        m = len(d["scores"])
        boxes[i, :m], scores[i, :m], classes[i, :m], counts[i] = d["boxes"], d["scores"], d["classes"], m
    return boxes, scores, classes, counts


def instances(osr, d, device="cpu"):
    from openset_rcnn_amd.host.structures import Boxes, Instances
    return Instances((480, 640), pred_boxes=Boxes(torch.from_numpy(d["boxes"]).to(device)), scores=torch.from_numpy(d["scores"]).to(device),
                     pred_classes=torch.from_numpy(d["classes"]).to(device))


def flat_detections(ev, tb, image_ids, classes, counts, reverse_map):
    """Per existing row: (image index into ev.img_ids or -1, slot) as accumulate_from_flags wants them, and the row mask."""
    n, cap = classes.shape
    exists = np.arange(cap)[None, :] < np.asarray(counts)[:, None]
    index = {img: i for i, img in enumerate(ev.img_ids)}
    image = np.repeat(np.array([index.get(i, -1) for i in image_ids], dtype=np.int64), cap).reshape(n, cap)
    table = tb.class_slots(reverse_map)
    ok = (classes >= 0) & (classes < len(table))
    slot = np.where(ok, table[np.where(ok, classes, 0)], -1)
    return image[exists], slot[exists], exists
