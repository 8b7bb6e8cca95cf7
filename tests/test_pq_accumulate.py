"""osr_pq_accumulate (csrc/osr_seg_eval.hip) on maps of a few dozen pixels with known answers, fed through
osr_panoptic_pair_counts: tp / fp / fn equal to the hand count and to the reference (tests/seg_eval_common.py), the IoU sums
bit-equal to the float64 reference that adds in (image, gt id, pred id) order.

At its table limits the kernel gets count tables synthesized in numpy (tests/seg_eval_common.py; their reach is asserted on the CPU in
tests/test_pq_table_reference.py): G = 1023, P = 2047, ncat = 1500, where every strided loop of the one workgroup takes a second step
and the LDS tables are filled to their ends; rows with several matches (the full-row walk of phase 3); two calls into one result."""
import numpy as np
import pytest
import torch

from tests.seg_eval_common import PQ_LARGE, PQReference, ids_to_rgb, pair_counts_reference, pq_large_table, pq_multi_match_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NCAT = 4


def tables(gt_segs):
    """gt_segs in the JSON's order: dicts {id, slot, area, iscrowd} -> (gt_ids ascending, gt_meta rows in that order)."""
    last_crowd = {}
    for s in gt_segs:
        if s.get("iscrowd", 0):
            last_crowd[s["slot"]] = s["id"]
    segs = sorted(gt_segs, key=lambda s: s["id"])
    meta = [[s["slot"], int(s.get("iscrowd", 0)), s["area"], int(last_crowd.get(s["slot"]) == s["id"])] for s in segs]
    return [s["id"] for s in segs], np.array(meta, dtype=np.int32).reshape(-1, 4)


class Pair:
    """The device statistics and the reference, fed with the same images."""

    def __init__(self, osr, ncat=NCAT):
        self.ops = osr.ops
        self.counts = torch.zeros((ncat, 3), dtype=torch.int64, device=DEV)
        self.iou = torch.zeros((ncat,), dtype=torch.float64, device=DEV)
        self.flags = torch.zeros((3,), dtype=torch.int64, device=DEV)
        self.ref = PQReference(ncat)

    def add(self, gt_map, gt_segs, pred_map, pred_slots):
        gt_map, pred_map = np.asarray(gt_map, dtype=np.int64), np.asarray(pred_map, dtype=np.int64)
        for s in gt_segs:
            s.setdefault("area", int((gt_map == s["id"]).sum()))
        ids, meta = tables(gt_segs)
        rgb = ids_to_rgb(gt_map)
        table = self.ops.panoptic_pair_counts(torch.from_numpy(rgb).to(DEV), torch.tensor(ids, dtype=torch.int32, device=DEV),
                                              torch.from_numpy(pred_map.astype(np.int32)).to(DEV), len(pred_slots), self.flags)
        ref_table, _ = pair_counts_reference(rgb, ids, pred_map, len(pred_slots))
        assert np.array_equal(table.cpu().numpy(), ref_table)
        self.ops.pq_accumulate(table, torch.from_numpy(meta).to(DEV), torch.tensor(pred_slots, dtype=torch.int32, device=DEV), self.counts, self.iou, self.flags)
        self.ref.add(ref_table, meta, pred_slots)
        return self

    def check(self, counts=None, flags=(0, 0, 0)):
        got = self.counts.cpu().numpy()
        assert np.array_equal(got, self.ref.counts), (got, self.ref.counts)
        if counts is not None:
            assert got.tolist() == counts
        assert self.flags.tolist() == list(flags) and self.ref.flags.tolist()[1:] == list(flags)[1:]
        iou = self.iou.cpu().numpy()
        assert iou.tobytes() == np.array(self.ref.iou, dtype=np.float64).tobytes(), (iou, self.ref.iou)  # bit-equal
        return iou


def test_a_perfect_match(osr):
    m = [[7, 7, 7, 0], [7, 7, 7, 0]]
    iou = Pair(osr).add(m, [dict(id=7, slot=2)], [[1, 1, 1, 0], [1, 1, 1, 0]], [2]).check([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]])
    assert iou.tolist() == [0.0, 0.0, 1.0, 0.0]


def test_iou_of_exactly_one_half_is_no_match(osr):
    """Areas 3 and 3, intersection 2, union 4. The fourth pixel carries another pair that overlaps nothing of its own category."""
    gt = [[5, 5, 5, 6]]
    pred = [[2, 1, 1, 1]]
    iou = Pair(osr).add(gt, [dict(id=5, slot=0), dict(id=6, slot=1)], pred, [0, 2]).check([[0, 1, 1], [0, 0, 1], [0, 1, 0], [0, 0, 0]])
    assert iou.tolist() == [0.0] * 4


def test_a_match_that_the_void_subtraction_makes(osr):
    """gt [A A A .], pred [. 1 1 1]: intersection 2, areas 3 and 3, but one predicted pixel lies on VOID: union 3, IoU 2 / 3."""
    iou = Pair(osr).add([[5, 5, 5, 0]], [dict(id=5, slot=0)], [[0, 1, 1, 1]], [0]).check([[1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
    assert iou[0] == 2.0 / 3.0


def test_a_category_mismatch(osr):
    Pair(osr).add([[9, 9], [9, 9]], [dict(id=9, slot=1)], [[1, 1], [1, 1]], [2]).check([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, 0]])


def test_a_crowd_is_never_tp_or_fn_and_shields_above_one_half_only(osr):
    """Crowd C (6 pixels, slot 3); prediction 1 covers 4 of them (IoU 4 / 6 if C were not crowd): shielded, no tp, no fp. Prediction 2
    (slot 3) has 2 of its 4 pixels on C, exactly half: not shielded, fp. D (slot 1) has no partner: fn."""
    gt = [[30, 30, 30, 30, 30, 30, 40, 40]]
    pred = [[1, 1, 1, 1, 2, 2, 2, 2]]
    p = Pair(osr).add(gt, [dict(id=30, slot=3, iscrowd=1), dict(id=40, slot=1)], pred, [3, 3])
    p.check([[0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 1, 0]])


def test_of_two_crowds_the_last_in_json_order_shields(osr):
    """Crowds 20 and 10 of slot 3, listed as [20, 10]: the shield is 10 (the JSON's last), while the sorted rows end with 20.
    Prediction 1 lies on 20: fp. Prediction 2 lies on 10: shielded."""
    gt = [[20, 20, 20, 10, 10, 10]]
    pred = [[1, 1, 1, 2, 2, 2]]
    segs = [dict(id=20, slot=3, iscrowd=1), dict(id=10, slot=3, iscrowd=1)]
    ids, meta = tables([dict(s, area=3) for s in segs])
    assert ids == [10, 20] and meta[:, 3].tolist() == [1, 0]
    Pair(osr).add(gt, segs, pred, [3, 3]).check([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 1, 0]])


def test_an_unlisted_id_only_adds_to_the_areas(osr):
    """Id 99 is painted but not listed. Prediction 1 = A plus two pixels of 99: area 5, IoU 3 / 5, a match that 99's pixels make worse but
    do not break; prediction 2 lies on 99 alone: fp, no fn for 99."""
    gt = [[5, 5, 5, 99, 99, 99, 99]]
    pred = [[1, 1, 1, 1, 1, 2, 2]]
    iou = Pair(osr).add(gt, [dict(id=5, slot=0)], pred, [0, 1]).check([[1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0]])
    assert iou[0] == 3.0 / 5.0


def test_an_empty_prediction_and_an_unknown_slot_become_flags(osr):
    gt = [[5, 5, 5, 5]]
    pred = [[1, 1, 1, 3]]  # id 2 is listed and has no pixel; id 3 has slot -1
    p = Pair(osr).add(gt, [dict(id=5, slot=0)], pred, [0, 1, -1])
    p.check([[1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], flags=(0, 1, 1))
    p.add(gt, [dict(id=5, slot=0)], pred, [0, 1, NCAT]).check([[2, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], flags=(0, 2, 2))


def test_no_segments_at_all(osr):
    Pair(osr).add([[0, 0]], [], [[0, 0]], []).check([[0, 0, 0]] * 4)
    Pair(osr).add([[4, 4]], [dict(id=4, slot=1)], [[0, 0]], []).check([[0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0]])
    Pair(osr).add([[0, 0]], [], [[1, 1]], [2]).check([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])  # all of it on VOID: no fp


def _strips(rng, n, length, slots):
    """n rows; row k holds gt id k + 1 on [0, a) and predicted id k + 1 on [s, s + b): IoUs of many different denominators."""
    gt, pred = np.zeros((n, length), dtype=np.int64), np.zeros((n, length), dtype=np.int64)
    for k in range(n):
        a, s = int(rng.integers(6, length - 2)), int(rng.integers(0, 4))
        b = int(rng.integers(4, length - s + 1))
        gt[k, :a], pred[k, s:s + b] = k + 1, k + 1
    segs = [dict(id=k + 1, slot=int(slots[k])) for k in range(n)]
    return gt, segs, pred, [int(v) for v in slots]


def test_three_images_accumulate_in_order(osr):
    rng = np.random.default_rng(0)
    p = Pair(osr)
    for n in (7, 12, 9):
        p.add(*_strips(rng, n, 19, rng.integers(0, 2, size=n)))  # two slots: several matches per slot and image
    iou = p.check()
    tp = p.counts.cpu().numpy()[:, 0]
    assert tp[:2].min() >= 5  # (the ordered sums have many terms)
    # the order is observable: some other order of the same terms gives other bits for at least one slot
    terms = {0: [], 1: []}
    probe = PQReference(NCAT)
    rng = np.random.default_rng(0)
    for n in (7, 12, 9):
        gt, segs, pred, slots = _strips(rng, n, 19, rng.integers(0, 2, size=n))
        for s in segs:
            s["area"] = int((gt == s["id"]).sum())
        ids, meta = tables(segs)
        before = list(probe.iou)
        table, _ = pair_counts_reference(ids_to_rgb(gt), ids, pred, len(slots))
        for g in range(len(ids)):  # one row at a time exposes each term
            one = PQReference(NCAT)
            row = np.zeros_like(table)
            row[0], row[1 + g], row[-1] = table[0], table[1 + g], table[1:].sum(axis=0) - table[1 + g]
            one.add(row, meta, slots)
            for s in (0, 1):
                if one.iou[s]:
                    terms[s].append(one.iou[s])
        probe.add(table, meta, slots)
        assert before != probe.iou
    assert all(sum(terms[s]) == iou[s] for s in (0, 1))
    assert any(sum(sorted(terms[s])) != iou[s] or sum(reversed(terms[s])) != iou[s] for s in (0, 1))


class Tables:
    """The device statistics and the reference, fed with the same synthesized count tables."""

    def __init__(self, osr, ncat):
        self.ops = osr.ops
        self.counts = torch.zeros((ncat, 3), dtype=torch.int64, device=DEV)
        self.iou = torch.zeros((ncat,), dtype=torch.float64, device=DEV)
        self.flags = torch.zeros((3,), dtype=torch.int64, device=DEV)
        self.ref = PQReference(ncat)

    def add(self, table, meta, slots):
        self.ops.pq_accumulate(torch.from_numpy(table).to(DEV), torch.from_numpy(meta).to(DEV), torch.from_numpy(slots).to(DEV), self.counts, self.iou, self.flags)
        self.ref.add(table, meta, slots)
        return self

    def check(self):
        got = self.counts.cpu().numpy()
        assert np.array_equal(got, self.ref.counts), np.nonzero((got != self.ref.counts).any(axis=1))[0]
        assert self.flags.tolist() == self.ref.flags.tolist()
        iou, want = self.iou.cpu().numpy(), np.array(self.ref.iou, dtype=np.float64)
        assert iou.tobytes() == want.tobytes(), np.nonzero(iou != want)[0]  # bit-equal
        return got


def test_the_largest_table_with_more_slots_than_threads(osr):
    """G = 1023, P = 2047, ncat = 1500: 1025 table rows, 2047 ids, 2 094 081 pairs and 1500 slots for 1024 threads; matches in the last row,
    the last column and slots on both sides of 1024; crowds with and without crowd_pick, VOID, unlisted rows, empty ids, unknown slots."""
    t = Tables(osr, PQ_LARGE["ncat"]).add(*pq_large_table())
    got = t.check()
    assert got[:, 0].max() >= 100 and got[1024:, 0].sum() > 0 and got[:, 1].sum() > 0 and got[:, 2].sum() > 0 and min(t.flags.tolist()[1:]) > 0
    again = Tables(osr, PQ_LARGE["ncat"]).add(*pq_large_table())
    assert torch.equal(again.iou, t.iou) and torch.equal(again.counts, t.counts)


def test_rows_with_several_matches_are_walked_in_p_order(osr):
    """Inconsistent areas give four rows three matches each (g_nmatch > 1), between ordinary rows of the same slot: the sum is bit-equal
    to the (g, p) order, which differs from the reversed, the p-major and the multi-rows-last orders (asserted on the CPU)."""
    t = Tables(osr, 4).add(*pq_multi_match_table())
    got = t.check()
    assert got[1, 0] >= 3 * 2 + 2  # three rows with two matches and an ordinary row on either side, at the least


def test_two_tables_of_different_size_accumulate(osr):
    """The large table, then the multi-match table in the large one's first hot slot: the second call goes on from the first's sums."""
    ncat, slot = PQ_LARGE["ncat"], PQ_LARGE["hot"][0]
    t = Tables(osr, ncat).add(*pq_large_table())
    first = t.check()[slot].copy()
    before = float(t.iou[slot])
    second = t.add(*pq_multi_match_table(ncat=ncat, slot=slot)).check()[slot]
    assert second[0] > first[0] >= 100 and float(t.iou[slot]) > before > 0
