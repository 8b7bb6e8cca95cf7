"""numpy / float64 references for the segmentation evaluators' kernels and figures, written from the rules in include/osr.h
(osr_semseg_confusion, osr_panoptic_pair_counts, osr_pq_accumulate) and in the evaluators' docstrings. Nothing here imports the
host module: only the input formats are shared."""
import numpy as np


def blocky(rng, h, w, n, cell=8):
    """An (h, w) map of values 0 .. n - 1 drawn per cell x cell block (runs of equal values, block edges inside tiles)."""
    small = rng.integers(0, n, size=((h + cell - 1) // cell, (w + cell - 1) // cell))
    return np.kron(small, np.ones((cell, cell), dtype=np.int64))[:h, :w].astype(np.int64)


def argmax_lowest(values):
    """(C, h, w) -> (h, w): strict comparisons from class 0 up (the lowest class wins a tie, NaN never replaces the incumbent)."""
    best, arg = values[0].copy(), np.zeros(values.shape[1:], dtype=np.int64)
    for c in range(1, values.shape[0]):
        better = values[c] > best
        best = np.where(better, values[c], best)
        arg = np.where(better, c, arg)
    return arg


def confusion_reference(labels, gt, num_classes, ignore_value):
    """-> ((C + 1, C + 1) int64 [pred][gt], invalid): np.bincount over the countable pixels."""
    c = num_classes
    labels, gt = np.asarray(labels, dtype=np.int64).reshape(-1), np.asarray(gt, dtype=np.int64).reshape(-1)
    ignored = gt == ignore_value
    bad = (~ignored & (gt >= c)) | (labels < 0) | (labels >= c)
    col = np.where(ignored, c, gt)
    conf = np.bincount((labels * (c + 1) + col)[~bad], minlength=(c + 1) ** 2).reshape(c + 1, c + 1)
    return conf.astype(np.int64), int(bad.sum())


def ids_to_rgb(ids):
    ids = np.asarray(ids, dtype=np.int64)
    return np.stack((ids % 256, ids // 256 % 256, ids // 65536 % 256), axis=-1).astype(np.uint8)


def pair_counts_reference(rgb, gt_ids, pred, num_pred):
    """-> ((G + 2, P + 1) int32, flags[0]): np.unique over (row, predicted id) of the countable pixels."""
    rgb = np.asarray(rgb, dtype=np.int64)
    ids = (rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]).reshape(-1)
    pred = np.asarray(pred, dtype=np.int64).reshape(-1)
    g = len(gt_ids)
    row_of = {int(v): 1 + i for i, v in enumerate(gt_ids)}
    row_of[0] = 0
    rows = np.array([row_of.get(int(v), g + 1) for v in ids], dtype=np.int64)
    ok = (pred >= 0) & (pred <= num_pred)
    counts = np.zeros((g + 2, num_pred + 1), dtype=np.int32)
    keys, n = np.unique(rows[ok] * (num_pred + 1) + pred[ok], return_counts=True)
    counts.reshape(-1)[keys] = n
    return counts, int((~ok).sum())


class PQReference:
    """The running statistics of osr_pq_accumulate, one image at a time, with python floats (float64) added in (g, p) order."""

    def __init__(self, ncat):
        self.counts = np.zeros((ncat, 3), dtype=np.int64)
        self.iou = [0.0] * ncat
        self.flags = np.zeros(3, dtype=np.int64)
        self.ncat = ncat

    def add(self, counts, gt_meta, pred_slot):
        counts = np.asarray(counts, dtype=np.int64)
        g_n, p_n = counts.shape[0] - 2, counts.shape[1] - 1
        area_p = counts.sum(axis=0)
        g_matched, p_matched = set(), set()
        for g in range(g_n):
            slot, crowd, area_g, _ = (int(v) for v in gt_meta[g])
            if not 0 <= slot < self.ncat:
                continue
            for p in range(1, p_n + 1):
                inter = int(counts[1 + g, p])
                if inter <= 0 or crowd or int(pred_slot[p - 1]) != slot:
                    continue
                union = int(area_p[p]) + area_g - inter - int(counts[0, p])
                iou = float(inter) / float(union)
                if iou > 0.5:
                    self.counts[slot, 0] += 1
                    self.iou[slot] += iou
                    g_matched.add(g)
                    p_matched.add(p)
        crowd_row = {}
        for g in range(g_n):
            slot, crowd, _, pick = (int(v) for v in gt_meta[g])
            if not 0 <= slot < self.ncat:
                self.flags[2] += 1
                continue
            if pick:
                crowd_row[slot] = g
            if not crowd and g not in g_matched:
                self.counts[slot, 2] += 1
        for p in range(1, p_n + 1):
            slot = int(pred_slot[p - 1])
            if not 0 <= slot < self.ncat:
                self.flags[2] += 1
                continue
            if area_p[p] == 0:
                self.flags[1] += 1
                continue
            if p in p_matched:
                continue
            covered = int(counts[0, p]) + (int(counts[1 + crowd_row[slot], p]) if slot in crowd_row else 0)
            if float(covered) / float(area_p[p]) > 0.5:
                continue
            self.counts[slot, 1] += 1


def pq_matches(counts, gt_meta, pred_slot, ncat):
    """The matches of one table in the contract's (g, p) order: [(g, p, slot, iou)] (g a row of gt_meta, p a predicted id).
    PQReference.add restated as a list, for the checks on the synthesized tables below."""
    counts = np.asarray(counts, dtype=np.int64)
    area_p = counts.sum(axis=0)
    out = []
    for g in range(counts.shape[0] - 2):
        slot, crowd, area_g, _ = (int(v) for v in gt_meta[g])
        if crowd or not 0 <= slot < ncat:
            continue
        for p in np.nonzero(counts[1 + g, 1:])[0] + 1:
            if int(pred_slot[p - 1]) != slot:
                continue
            inter = int(counts[1 + g, p])
            iou = float(inter) / float(int(area_p[p]) + area_g - inter - int(counts[0, p]))
            if iou > 0.5:
                out.append((g, int(p), slot, iou))
    return out


PQ_LARGE = dict(G=1023, P=2047, ncat=1500, hot=(7, 1300))


def pq_large_table(seed=0, G=PQ_LARGE["G"], P=PQ_LARGE["P"], ncat=PQ_LARGE["ncat"], hot=PQ_LARGE["hot"]):
    """A sparse seeded (G + 2, P + 1) count table with consistent areas, built without pixels -> (counts int32, gt_meta (G, 4) int32,
    pred_slot (P) int32). Every predicted id has one main row (the first G ids a permutation of the rows, so that every row has a
    partner), up to two small side rows, VOID and unlisted-row mass on a fifth each; a few ids are empty. A quarter of the rows lie
    in each of the two `hot` slots (one below 1024, one above), the others in random slots; some rows and ids carry slots outside
    [0, ncat) on both sides; 6 % of the rows are crowds; hot[0] and every second other slot that has crowds mark their last one
    crowd_pick, hot[1] marks none.
    The last row and the last predicted id are partners in hot[1]."""
    rng = np.random.default_rng(seed)
    counts = np.zeros((G + 2, P + 1), dtype=np.int64)
    slot_g = rng.integers(0, ncat, size=G)
    u = rng.random(G)
    slot_g[u < 0.25], slot_g[(u >= 0.25) & (u < 0.5)] = hot[0], hot[1]
    slot_g[rng.choice(G - 1, size=6, replace=False)] = [-1, -7, ncat, ncat + 1, ncat + 500, -2]
    slot_g[G - 1] = hot[1]
    crowd = rng.random(G) < 0.06
    crowd[G - 1] = False
    main = np.concatenate((rng.permutation(G), rng.integers(0, G, size=P - G)))
    slot_p = np.where(rng.random(P) < 0.75, slot_g[main], rng.integers(0, ncat, size=P))
    slot_p[rng.choice(P - 1, size=6, replace=False)] = [-3, -1, ncat, ncat + 2, 2 * ncat, -100]
    slot_p[P - 1] = hot[1]
    empty = rng.choice(np.arange(1, P), size=5, replace=False)  # predicted ids without a pixel (never the last)
    for p in range(1, P + 1):
        if p in empty:
            continue
        counts[1 + main[p - 1], p] = rng.integers(60, 300) if p <= G else rng.integers(3, 40)  # (a row's first partner dominates it)
        for g in rng.integers(0, G, size=rng.integers(0, 3)):
            counts[1 + g, p] += rng.integers(1, 60)
        if rng.random() < 0.2:
            counts[0, p] = rng.integers(1, 80)      # VOID under the prediction
        if rng.random() < 0.2:
            counts[G + 1, p] = rng.integers(1, 80)  # ids the JSON does not list
    counts[:, 0] = rng.integers(0, 50, size=G + 2)  # pixels without a prediction
    counts[G, 1:], counts[:, P] = 0, 0                # the last row and the last id are partners, and little else
    counts[G, P], counts[0, P], counts[G + 1, P] = 150, 7, 9
    area_g = counts[1:G + 1].sum(axis=1)
    pick = np.zeros(G, dtype=bool)
    for i, s in enumerate(np.unique(slot_g[crowd])):
        if s == hot[0] or (s != hot[1] and i % 2 == 0):
            pick[np.nonzero(crowd & (slot_g == s))[0][-1]] = True
    meta = np.stack((slot_g, crowd.astype(np.int64), area_g, pick.astype(np.int64)), axis=1)
    return counts.astype(np.int32), meta.astype(np.int32), slot_p.astype(np.int32)


def pq_multi_match_table(seed=5, G=40, P=90, ncat=4, slot=1, multi=(9, 17, 18, 30)):
    """A table whose gt_meta areas are SMALLER than the row sums for the rows in `multi` (inconsistent areas: impossible from pixels,
    allowed by the contract), so that those rows match two or three predicted ids each with IoU > 0.5. Every row lies in `slot` and
    has one ordinary partner except the `multi` rows; the ids in between belong to another slot or overlap too little. The multi
    rows' partners are spread over the ids, so that a row's terms are not neighbours in p.
    -> (counts int32, gt_meta (G, 4) int32, pred_slot (P) int32)."""
    rng = np.random.default_rng(seed)
    counts = np.zeros((G + 2, P + 1), dtype=np.int64)
    slot_p = np.full(P, (slot + 1) % ncat, dtype=np.int64)
    area_g = np.zeros(G, dtype=np.int64)
    ids = rng.permutation(P) + 1
    nxt = 0
    for g in range(G):
        n = int(rng.integers(2, 4)) if g in multi else 1
        inters = rng.integers(85, 100, size=n) if g in multi else rng.integers(60, 100, size=n)
        for inter in inters:
            p = ids[nxt]
            nxt += 1
            counts[1 + g, p] = inter
            counts[G + 1, p] = rng.integers(0, 15)  # the prediction's pixels elsewhere
            slot_p[p - 1] = slot
        counts[1 + g, 0] = rng.integers(0, 10)
        area_g[g] = int(inters.max()) + counts[1 + g, 0]  # (what one partner alone would leave of the row)
    for p in ids[nxt:]:  # the other ids: the wrong slot, or the right one with too little overlap
        g = int(rng.integers(0, G))
        counts[1 + g, p] = rng.integers(1, 10)
        counts[G + 1, p] = 100
        slot_p[p - 1] = slot if rng.random() < 0.5 else (slot + 1) % ncat
    single = np.array([g not in multi for g in range(G)])
    area_g[single] = counts[1:G + 1].sum(axis=1)[single]
    meta = np.stack((np.full(G, slot), np.zeros(G, dtype=np.int64), area_g, np.zeros(G, dtype=np.int64)), axis=1)
    return counts.astype(np.int32), meta.astype(np.int32), slot_p.astype(np.int32)


def sem_seg_figures(conf, names):
    """mIoU / fwIoU / mACC / pACC and the per-class figures from the (C + 1, C + 1) matrix, x100, with python loops."""
    m = np.asarray(conf, dtype=np.int64)[:-1, :-1]
    c = m.shape[0]
    gt_total = int(m.sum())
    ious, accs, fw, tp_total = [], [], 0.0, 0
    res = {}
    for i in range(c):
        tp, pos_gt, pos_pred = int(m[i, i]), int(m[:, i].sum()), int(m[i, :].sum())
        tp_total += tp
        if pos_gt > 0:
            acc, iou = tp / pos_gt, tp / (pos_gt + pos_pred - tp)
            accs.append(acc)
            ious.append(iou)
            fw += iou * (pos_gt / gt_total)
        else:
            acc = iou = float("nan")
        res[f"IoU-{names[i]}"], res[f"ACC-{names[i]}"] = 100 * iou, 100 * acc
    res.update(mIoU=100 * sum(ious) / len(ious), fwIoU=100 * fw, mACC=100 * sum(accs) / len(accs), pACC=100 * tp_total / gt_total)
    return res


def pq_figures(counts, iou, isthing):
    res = {}
    for suffix, want in (("", None), ("_th", True), ("_st", False)):
        rows = []
        for i in range(len(isthing)):
            tp, fp, fn = (int(v) for v in counts[i])
            if (want is None or bool(isthing[i]) == want) and tp + fp + fn > 0:
                den = tp + fp / 2 + fn / 2
                rows.append((iou[i] / den, iou[i] / tp if tp else 0.0, tp / den))
        for k, key in enumerate(("PQ", "SQ", "RQ")):
            res[key + suffix] = 100 * sum(r[k] for r in rows) / len(rows) if rows else 0.0
    return res
