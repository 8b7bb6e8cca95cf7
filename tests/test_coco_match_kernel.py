"""osr_coco_match (csrc/osr_coco_eval.hip) against the numpy COCOeval's per-image results: flags, rank and match bit for bit with
nothing left out. The shapes are the smallest that reach every path: a group with more detections than max_det and more ground
truths than a wave has lanes, empty groups of both kinds, an image without detections, a grid of more groups than the part has
CUs, and the keypoint task with both OKS branches."""
import numpy as np
import pytest
import torch

from tests.coco_eval_common import coco_json, device_match, jitter_xyxy, random_boxes_xywh, reference_outputs

DEV = "cuda:0"
IMAGE_IDS = [5, 9, 12]


def bbox_case():
    """n = 3, K = 3, cap = 160. Image 0: class 0 has 130 detections (max_det 100 cuts them) against 70 ground truths, ten of them
    duplicates, some crowd, areas on both sides of the range limits; class 1 ground truths only; class 2 detections only; a few rows
    carry a class outside [0, K). Image 1: the exact 0.5 and 0.75 pairs, plus a small mixed group. Image 2: counts = 0. Scores are
    multiples of 1/32 in shuffled rows, so they repeat."""
    rng = np.random.default_rng(20)
    n, cap = 3, 160
    g0 = random_boxes_xywh(rng, 70, 300.0)
    g0[60:] = g0[:10]
    anns = [dict(image_id=5, category_id=1, bbox=b.tolist(), iscrowd=int(rng.random() < 0.15), area=float(b[2] * b[3])) for b in g0]
    anns += [dict(image_id=5, category_id=2, bbox=b.tolist()) for b in random_boxes_xywh(rng, 4)]
    anns += [dict(image_id=9, category_id=1, bbox=[0, 0, 1, 1]), dict(image_id=9, category_id=2, bbox=[0, 0, 3, 1])]
    g1 = random_boxes_xywh(rng, 10)
    anns += [dict(image_id=9, category_id=3, bbox=b.tolist(), iscrowd=int(k == 3)) for k, b in enumerate(g1)]
    anns += [dict(image_id=12, category_id=1, bbox=b.tolist()) for b in random_boxes_xywh(rng, 3)]
    rng.shuffle(anns)  # (the JSON need not be grouped)
    gt = coco_json(IMAGE_IDS, [1, 2, 3], anns)
    boxes = jitter_xyxy(rng, random_boxes_xywh(rng, n * cap)).reshape(n, cap, 4)  # rows past counts hold plausible values that must not count
    scores = (rng.integers(1, 32, size=(n, cap)) / 32.0).astype(np.float32)
    classes = rng.integers(0, 3, size=(n, cap)).astype(np.int64)
    src = rng.integers(0, 70, size=130)
    b0 = jitter_xyxy(rng, g0[src], 4.0)
    b0[:25] = jitter_xyxy(rng, g0[src[:25]], 0.0)  # exact copies: IoU 1, and ties where the ground truth is duplicated
    rows = rng.permutation(155)
    boxes[0, rows[:130]], classes[0, rows[:130]] = b0, 0
    classes[0, rows[130:150]] = 2
    classes[0, rows[150:153]], classes[0, rows[153:155]] = -1, 3
    boxes[1, 0], classes[1, 0], scores[1, 0] = [0, 0, 2, 1], 0, 0.5
    boxes[1, 1], classes[1, 1], scores[1, 1] = [0, 0, 4, 1], 1, 0.5
    boxes[1, 2:14], classes[1, 2:14] = jitter_xyxy(rng, g1[rng.integers(0, 10, size=12)], 3.0), 2
    counts = np.array([155, 14, 0], dtype=np.int32)
    return gt, boxes, scores, classes, counts


@pytest.fixture(scope="module")
def bbox_ref(osr):
    gt, boxes, scores, classes, counts = bbox_case()
    return (gt, boxes, scores, classes, counts) + reference_outputs(osr, gt, IMAGE_IDS, boxes, scores, classes, counts, "bbox", 100)


@pytest.mark.gpu
def test_bbox_flags_rank_and_match_equal_the_numpy_cocoeval(osr, bbox_ref):
    gt, boxes, scores, classes, counts, flags, rank, match, sims, tb, seg_off = bbox_ref
    # the case holds what it claims
    assert (classes[0, :155] == 0).sum() == 130 and rank[0].max() == 99 and (rank[0, :155][classes[0, :155] == 0] == -1).sum() == 30
    assert seg_off[1] - seg_off[0] == 70 and seg_off[2] - seg_off[1] == 4 and seg_off[3] == seg_off[2] and (rank[2] == -1).all()
    assert flags[1, 0, 0] & 0x3ff == 0x001 and flags[1, 1, 0] & 0x3ff == 0x03f  # IoU exactly 0.5 and 0.75: matched up to that threshold
    assert len(np.unique(scores[0, :155])) < 40
    f, r, m, sim = device_match(osr, DEV, gt, IMAGE_IDS, boxes, scores, classes, counts, "bbox", 100, want_sim=True)
    assert np.array_equal(r, rank)
    assert np.array_equal(f, flags)
    assert np.array_equal(m, match)
    K, mcap = 3, 100
    for (i, k), s in sims.items():  # the similarities themselves are numpy's, bit for bit
        if s.size:
            g = seg_off[i * K + k]
            assert np.array_equal(sim[g * mcap: g * mcap + s.size].reshape(s.shape), s), (i, k)


@pytest.mark.gpu
def test_bbox_at_max_det_128_fills_the_second_half_of_the_result_byte(osr, bbox_ref):
    """The same arrays with max_det = 128, the kernel's limit: the 130 detections of class 0 are ranked up to 127, so the detections
    64 .. 127 of a pass (bits 2-3 of a lane's result byte) are all in use."""
    gt, boxes, scores, classes, counts = bbox_ref[:5]
    flags, rank, match, _, _, _ = reference_outputs(osr, gt, IMAGE_IDS, boxes, scores, classes, counts, "bbox", 128)
    # conditions on the input
    assert rank[0].max() == 127 and (rank[0, :155][classes[0, :155] == 0] == -1).sum() == 2
    assert ((flags[0] & 0xffff).any(axis=1) & (rank[0] >= 100)).any()  # a detection beyond rank 99 is matched
    f, r, m, _ = device_match(osr, DEV, gt, IMAGE_IDS, boxes, scores, classes, counts, "bbox", 128)
    assert np.array_equal(r, rank)
    assert np.array_equal(f, flags)
    assert np.array_equal(m, match)


@pytest.mark.gpu
def test_repeats_are_bit_identical_and_no_image_launches_nothing(osr, bbox_ref):
    gt, boxes, scores, classes, counts = bbox_ref[:5]
    a = device_match(osr, DEV, gt, IMAGE_IDS, boxes, scores, classes, counts, "bbox", 100)
    b = device_match(osr, DEV, gt, IMAGE_IDS, boxes, scores, classes, counts, "bbox", 100)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)  # noqa: E731
    flags, rank, _, _ = osr.ops.coco_match(z(0, 8, 4), z(0, 8), z(0, 8, dt=torch.int64), z(0, dt=torch.int32), 3, z(1, dt=torch.int32), z(0, 4, dt=torch.float64),
                                           z(0, dt=torch.float64), z(0, dt=torch.uint8), 0, [0.5], [[0, 1e10]], 100)
    assert tuple(flags.shape) == (0, 8, 1) and tuple(rank.shape) == (0, 8)


@pytest.mark.gpu
def test_a_grid_of_320_groups_equals_the_images_one_at_a_time(osr):
    rng = np.random.default_rng(3)
    n, K, cap = 4, 80, 16
    ids = [3, 4, 8, 9]
    anns, boxes, classes = [], np.zeros((n, cap, 4), dtype=np.float32), np.zeros((n, cap), dtype=np.int64)
    for i, img in enumerate(ids):
        g = random_boxes_xywh(rng, 7)
        gc = rng.choice([0, 1, 38, 39, 40, 78, 79], size=7)
        anns += [dict(image_id=img, category_id=int(c) + 1, bbox=b.tolist(), iscrowd=int(rng.random() < 0.2)) for b, c in zip(g, gc)]
        src = rng.integers(0, 7, size=cap)
        boxes[i], classes[i] = jitter_xyxy(rng, g[src], 3.0), np.where(rng.random(cap) < 0.8, gc[src], rng.integers(0, K, size=cap))
    gt = coco_json(ids, list(range(1, K + 1)), anns)
    scores = (rng.integers(1, 16, size=(n, cap)) / 16.0).astype(np.float32)
    counts = np.array([16, 12, 0, 15], dtype=np.int32)
    flags, rank, match, _, _, seg_off = reference_outputs(osr, gt, ids, boxes, scores, classes, counts, "bbox", 100)
    f, r, m, _ = device_match(osr, DEV, gt, ids, boxes, scores, classes, counts, "bbox", 100)
    assert np.array_equal(r, rank) and np.array_equal(f, flags) and np.array_equal(m, match)
    assert (f & 0xffff).any() and (r >= 0).sum() == 43
    for i in range(n):
        f1, r1, m1, _ = device_match(osr, DEV, gt, ids[i:i + 1], boxes[i:i + 1], scores[i:i + 1], classes[i:i + 1], counts[i:i + 1], "bbox", 100)
        assert np.array_equal(f1[0], f[i]) and np.array_equal(r1[0], r[i])
        assert np.array_equal(np.where(m1[0] >= 0, m1[0] + seg_off[i * K], -1), m[i])


def keypoint_case():
    """Kp = 17, max_det = 20, 25 detections against 5 ground truths of one category: three regular ones, one whose points all carry
    v = 0 although it counts three labelled ones (the k1 == 0 branch, not ignored), one with num_keypoints = 0 (ignored)."""
    rng = np.random.default_rng(1)
    kp, cap = 17, 32
    g = np.array([[20, 30, 90, 120], [150, 40, 60, 80], [60, 160, 120, 100], [220, 150, 40, 50], [10, 200, 45, 60]], dtype=np.float64)
    anns, pts = [], []
    for j, b in enumerate(g):
        v = rng.integers(0, 3, size=kp) if j < 3 else np.zeros(kp, dtype=np.int64)
        p = np.stack([b[0] + rng.random(kp) * b[2], b[1] + rng.random(kp) * b[3], v], axis=1)
        p[v == 0, :2] = 0
        p = np.round(p, 2)
        pts.append(p)
        anns.append(dict(image_id=1, category_id=1, bbox=b.tolist(), area=float(b[2] * b[3] * 0.7), keypoints=p.reshape(-1).tolist(),
                         num_keypoints=int((v > 0).sum()) if j < 3 else (3 if j == 3 else 0)))
    gt = coco_json([1], [1], anns)
    src = rng.integers(0, 5, size=cap)
    kpts = np.zeros((1, cap, kp, 3), dtype=np.float32)
    boxes = np.zeros((1, cap, 4), dtype=np.float32)
    for r in range(cap):
        b, p = g[src[r]], pts[src[r]]
        centre = b[:2] + b[2:] / 2 + (rng.random(2) - 0.5) * b[2:] * (3.0 if r % 3 == 0 else 0.5)  # (some land outside the doubled box)
        kpts[0, r, :, :2] = np.where(p[:, 2:3] > 0, p[:, :2], centre) + rng.normal(0, rng.choice([0.02, 0.05, 0.1]) * np.sqrt(b[2] * b[3]), size=(kp, 2)) + 0.5
        kpts[0, r, :, 2] = rng.random(kp)
        boxes[0, r] = [b[0], b[1], b[0] + b[2], b[1] + b[3]]
    scores = (rng.integers(1, 24, size=(1, cap)) / 24.0).astype(np.float32)
    from openset_rcnn_amd.host.coco_evaluation import COCO_KEYPOINT_OKS_SIGMAS
    return gt, boxes, scores, np.zeros((1, cap), dtype=np.int64), np.array([25], dtype=np.int32), kpts, COCO_KEYPOINT_OKS_SIGMAS


@pytest.mark.gpu
def test_keypoint_oks_and_flags_equal_the_numpy_cocoeval(osr):
    """The OKS must be within 1e-12 of numpy's float64 value: each exp(-e) term carries a few ulp of 1 (2.2e-16) plus the rounding of
    e (about six operations) times e * exp(-e) <= 0.37, under 1e-15 in all; the bound leaves a thousandfold margin. The inputs are
    seeded so that no OKS lies within 1e-6 of a threshold, six orders above that: the flags must then be equal, none excluded."""
    gt, boxes, scores, classes, counts, kpts, sigmas = keypoint_case()
    flags, rank, match, sims, tb, seg_off = reference_outputs(osr, gt, [1], boxes, scores, classes, counts, "keypoints", 20, kpts, sigmas)
    ref = sims[0, 0]
    thrs = np.linspace(.5, .95, 10)
    assert ref.shape == (20, 5) and np.abs(ref[:, :, None] - thrs).min() >= 1e-6  # a condition on the inputs
    assert (ref[:, 3] > 0.5).any() and (ref[:, 3] < 1e-3).any() and (ref[:, 3] == 1.0).any()  # the doubled-box branch: inside, near and far
    assert (rank[0, :25] == -1).sum() == 5 and (flags & 0xffff).any() and ((flags >> 16) & 0xffff).any()
    f, r, m, sim = device_match(osr, DEV, gt, [1], boxes, scores, classes, counts, "keypoints", 20, kpts, sigmas, want_sim=True)
    got = sim[:100].reshape(20, 5)
    print("max |oks - numpy|:", np.abs(got - ref).max())
    assert np.abs(got - ref).max() <= 1e-12
    assert np.array_equal(r, rank)
    assert np.array_equal(f, flags)
    assert np.array_equal(m, match)
