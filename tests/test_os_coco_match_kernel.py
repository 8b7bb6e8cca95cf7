"""osr_os_coco_match (csrc/osr_os_coco_eval.hip) against the numpy OpensetCOCOEval's per-image results: flags, rank and match bit
for bit with nothing left out. The shapes are the smallest that reach every path: the three sets and their two tie orders, crowd
and out-of-range ground truths, sets with more ground truths than a wave has lanes, a list longer than max_det, images without
detections or without ground truth, and a grid of more groups than the part has CUs."""
import numpy as np
import pytest

from tests.coco_eval_common import coco_json, jitter_xyxy, random_boxes_xywh
from tests.os_coco_common import UNKNOWN, device_match, padded, reference_outputs, seeded_openset

DEV = "cuda:0"


def _check(osr, gt, known_ids, image_ids, boxes, scores, classes, counts, reverse_map, max_det=100):
    flags, rank, match, tb, batch, ev = reference_outputs(osr, gt, known_ids, image_ids, boxes, scores, classes, counts, reverse_map, max_det)
    f, r, m = device_match(osr, DEV, gt, known_ids, image_ids, boxes, scores, classes, counts, reverse_map, max_det)
    assert np.array_equal(r, rank)
    assert np.array_equal(f, flags)
    assert np.array_equal(m, match)
    return f, r, m, tb, batch


def seeded_case():
    gt, image_ids, known_ids, reverse_map, dets = seeded_openset(11)
    gt["images"].append(dict(id=40, file_name="40.jpg", height=480, width=640))  # an image without ground truth, with detections
    image_ids = image_ids + [40]
    dets.append(dict(dets[0]))
    dets[2] = {k: v[:0] for k, v in dets[2].items()}  # an image without detections
    dets[4] = {k: v[:7] for k, v in dets[4].items()}
    return gt, image_ids, known_ids, reverse_map, padded(dets, cap=24)


@pytest.fixture(scope="module")
def seeded_ref(osr):
    gt, image_ids, known_ids, reverse_map, lists = seeded_case()
    return (gt, image_ids, known_ids, reverse_map, lists) + reference_outputs(osr, gt, known_ids, image_ids, *lists, reverse_map)[:3]


@pytest.mark.gpu
def test_seeded_set_equals_the_numpy_class(osr, seeded_ref):
    gt, image_ids, known_ids, reverse_map, (boxes, scores, classes, counts), flags, rank, match = seeded_ref
    # the case holds what it claims: known, unknown and dropped classes, counts below cap, both kinds of empty image, all three words
    known_classes = [c for c, d in reverse_map.items() if d in known_ids]
    live = np.arange(24)[None, :] < counts[:, None]
    assert (counts < 24).all() and counts[2] == 0 and counts[6] > 0 and (classes[live] == UNKNOWN).any()
    assert np.isin(classes[live], known_classes).any() and (~np.isin(classes[live], known_classes + [UNKNOWN])).any()
    assert ((rank == -1) & live).any() and (rank[~live] == -1).all() and len(np.unique(scores[live])) < 24
    assert all((flags[..., s] & 0xffff).any() and (flags[..., s] >> 16).any() for s in range(3))
    f, r, m = device_match(osr, DEV, gt, known_ids, image_ids, boxes, scores, classes, counts, reverse_map)
    assert np.array_equal(r, rank)
    assert np.array_equal(f, flags)
    assert np.array_equal(m, match)


@pytest.mark.gpu
def test_repeats_are_bit_identical(osr, seeded_ref):
    gt, image_ids, known_ids, reverse_map, lists = seeded_ref[:5]
    a = device_match(osr, DEV, gt, known_ids, image_ids, *lists, reverse_map)
    b = device_match(osr, DEV, gt, known_ids, image_ids, *lists, reverse_map)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_the_two_tie_orders(osr):
    """One box annotated twice: first as category 2, then as category 1 (both known). A detection of the third known category meets
    them in annotation order and takes the LATER annotation (category 1); an unknown detection meets them ordered by slot and takes
    the HIGHER slot (category 2)."""
    box = [20.0, 30.0, 60.0, 40.0]
    gt = coco_json([1], [1, 2, 3, 4], [dict(image_id=1, category_id=2, bbox=box), dict(image_id=1, category_id=1, bbox=box)])
    boxes = np.array([[[20, 30, 80, 70], [20, 30, 80, 70]]], dtype=np.float32)
    scores, classes = np.array([[0.9, 0.8]], dtype=np.float32), np.array([[3, UNKNOWN]], dtype=np.int64)
    f, r, m, tb, (rows, _, _) = _check(osr, gt, [1, 2, 3], [1], boxes, scores, classes, np.array([2], dtype=np.int32), None)
    assert tb.slot[rows].tolist() == [0, 1] and tb.pos[rows].tolist() == [1, 0]  # the table: category 1 (annotated second), category 2
    assert (m[0, 0, 0, 1] == 0).all() and (f[0, 0, 0, 1] & 0xffff) == 0x3ff  # known slot, other-known set: the later annotation
    assert (m[0, 1, 0, 1] == 1).all() and (f[0, 1, 0, 1] & 0xffff) == 0x3ff  # unknown slot, known set: the higher slot
    assert (m[0, :, :, 0] == -1).all() and (m[0, :, :, 2] == -1).all() and r.tolist() == [[0, 0]]


@pytest.mark.gpu
def test_crowd_is_shared_and_an_out_of_range_ground_truth_comes_last(osr):
    """Two detections on a crowd ground truth both take it. A detection that overlaps a large ground truth closely and a small one
    less so takes the large one where both count, and the small one in the range where the large one is ignored."""
    anns = [dict(image_id=1, category_id=1, bbox=[200, 200, 50, 50], iscrowd=1),
            dict(image_id=1, category_id=1, bbox=[10, 10, 40, 40]),     # area 1600: medium
            dict(image_id=1, category_id=1, bbox=[10, 10, 40, 24])]     # area 960: small
    gt = coco_json([1], [1, 2], anns)
    boxes = np.array([[[200, 200, 250, 250], [205, 205, 245, 245], [10, 10, 50, 46]]], dtype=np.float32)
    scores, classes = np.array([[0.9, 0.8, 0.7]], dtype=np.float32), np.zeros((1, 3), dtype=np.int64)
    f, r, m, _, _ = _check(osr, gt, [1], [1], boxes, scores, classes, np.array([3], dtype=np.int32), {0: 1, 1: 2})
    assert (m[0, :2, 0, 0, 0] == 0).all() and (f[0, :2, 0, 0] >> 16 & 1).all()     # both on the crowd, both ignored
    assert m[0, 2, 0, 0, 0] == 1 and m[0, 2, 2, 0, 0] == 1                          # all / medium: the closer, medium one (IoU 0.9)
    assert m[0, 2, 1, 0, 0] == 2 and not (f[0, 2, 1, 0] >> 16 & 1)                  # small: the small one (IoU 0.67), not ignored
    assert m[0, 2, 3, 0, 0] == 1 and (f[0, 2, 3, 0] >> 16 & 1)                      # large: both out of range; the closer one, ignored


@pytest.mark.gpu
def test_sets_past_one_wavefront_and_a_list_past_max_det(osr):
    rng = np.random.default_rng(4)
    g = random_boxes_xywh(rng, 210, 300.0)
    g[60:70], g[130:140], g[200:210] = g[:10], g[:10], g[:10]  # duplicates inside and across the sets: ties
    cats = [1] * 70 + [int(c) for c in rng.choice([2, 3], size=70)] + [int(c) for c in rng.choice([4, 5], size=70)]
    anns = [dict(image_id=7, category_id=c, bbox=b.tolist(), iscrowd=int(rng.random() < 0.1)) for b, c in zip(g, cats)]
    rng.shuffle(anns)
    gt = coco_json([7], [1, 2, 3, 4, 5], anns)
    cap = 130
    src = rng.integers(0, 210, size=cap)
    boxes = jitter_xyxy(rng, g[src], 3.0)
    boxes[:40] = jitter_xyxy(rng, g[src[:40]], 0.0)
    classes = np.full(cap, 0, dtype=np.int64)
    rows = rng.permutation(128)
    classes[rows[120:124]], classes[rows[124:128]] = 1, UNKNOWN
    scores = (rng.integers(1, 32, size=cap) / 32.0).astype(np.float32)
    f, r, m, tb, _ = _check(osr, gt, [1, 2, 3], [7], boxes[None], scores[None], classes[None], np.array([128], dtype=np.int32), dict(enumerate([1, 2, 3, 4, 5])))
    assert np.bincount(tb.slot, minlength=4).tolist() == [70, 70 - cats[70:140].count(3), cats[70:140].count(3), 70]
    assert (classes[:128] == 0).sum() == 120 and r.max() == 99 and (r[0, :128][classes[:128] == 0] == -1).sum() == 20 and (r[0, 128:] == -1).all()
    assert all((m[0, :, 0, s] >= 64).any() for s in range(3))  # ground truths past the first 64 of the image are taken in every set


@pytest.mark.gpu
def test_a_grid_of_1160_groups(osr):
    rng = np.random.default_rng(8)
    n, n_cats, K, cap = 40, 40, 28, 12
    ids = list(range(100, 100 + n))
    cat_ids = list(range(1, n_cats + 1))
    known_ids = sorted(rng.permutation(cat_ids)[:K].tolist())
    anns, boxes, classes = [], np.zeros((n, cap, 4), dtype=np.float32), np.zeros((n, cap), dtype=np.int64)
    for i, img in enumerate(ids):
        g = random_boxes_xywh(rng, 6)
        gc = rng.integers(0, n_cats, size=6)
        anns += [dict(image_id=img, category_id=int(c) + 1, bbox=b.tolist(), iscrowd=int(rng.random() < 0.2)) for b, c in zip(g, gc)]
        src = rng.integers(0, 6, size=cap)
        boxes[i] = jitter_xyxy(rng, g[src], 3.0)
        classes[i] = np.where(rng.random(cap) < 0.3, UNKNOWN, np.where(rng.random(cap) < 0.7, gc[src], rng.integers(0, n_cats, size=cap)))
    gt = coco_json(ids, cat_ids, anns)
    scores = (rng.integers(1, 16, size=(n, cap)) / 16.0).astype(np.float32)
    counts = rng.integers(0, cap + 1, size=n).astype(np.int32)
    f, r, m, tb, _ = _check(osr, gt, known_ids, ids, boxes, scores, classes, counts, dict(enumerate(cat_ids)))
    assert tb.num_known + 1 == 29 and all((f[..., s] & 0xffff).any() for s in range(3)) and (f[20:] & 0xffff).any()
