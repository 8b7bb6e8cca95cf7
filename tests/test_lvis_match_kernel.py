"""osr_lvis_match (csrc/osr_lvis_eval.hip) against the numpy LVISEval's per-image results: flags, rank and match bit for bit with nothing
left out, at LVIS's own sizes (K = 1203, max_dets = 300). The five images are the smallest that reach every path: one group of 300
detections (past the 128 and 256 a narrower result word would hold) against 70 ground truths (past a wave's 64 lanes) with a tie across
the cut; 330 categories in one image, most of them not evaluated, so that the groups are many and of one detection; an image without a
detection; an image with negatives only; and an image that holds every federated rule once. 5 x 300 workgroups are more than the part
has CUs."""
import numpy as np
import pytest

from tests.coco_eval_common import jitter_xyxy, random_boxes_xywh
from tests.lvis_eval_common import device_match, lvis_json, reference_outputs

DEV = "cuda:0"
K = 1203
IMAGE_IDS = [4, 9, 15, 20, 31]
CAP = 340


def xyxy(x, y, w, h):
    return [x, y, x + w, y + h]


def lvis_case():
    rng = np.random.default_rng(24)
    n = len(IMAGE_IDS)
    boxes = jitter_xyxy(rng, random_boxes_xywh(rng, n * CAP)).reshape(n, CAP, 4)  # rows past counts hold plausible values that must not count
    scores = np.full((n, CAP), 2.0, dtype=np.float32)  # ... and scores that would win every cut
    classes = np.full((n, CAP), 7, dtype=np.int64)
    anns, neg, nex = [], {}, {}
    cat = lambda k: int(k) + 1  # noqa: E731  (dataset id of contiguous class k)

    # image 0: 330 detections of class 7 against its 70 ground truths; positions 299 and 300 of the image's order share a score
    g0 = random_boxes_xywh(rng, 70, 300.0)
    g0[60:] = g0[:10]  # duplicates: equal IoUs
    anns += [dict(image_id=4, category_id=cat(7), bbox=b.tolist(), **({"ignore": 1} if rng.random() < 0.15 else {})) for b in g0]
    src = rng.integers(0, 70, size=330)
    b0 = jitter_xyxy(rng, g0[src], 4.0)
    b0[:40] = jitter_xyxy(rng, g0[src[:40]], 0.0)  # exact copies: IoU 1, and ties where the ground truth is duplicated
    order = (1000 - np.arange(330)) / 1024.0
    order[300], order[11], order[150] = order[299], order[10], order[149]
    perm = rng.permutation(330)
    boxes[0, perm], scores[0, perm] = b0[rng.permutation(330)], order.astype(np.float32)

    # image 1: 330 detections in 330 distinct classes, -1 and K among them with the best scores; some positive, some negative, most neither
    others = rng.permutation(np.setdiff1d(np.arange(1, K - 1), [7, 63, 64]))[:324]
    c1 = np.concatenate([[-1, K, 0, 63, 64, K - 1], others]).astype(np.int64)
    positive, negative = np.concatenate([[0, 64, K - 1], others[:40]]), np.concatenate([[63], others[40:80]])
    g1 = random_boxes_xywh(rng, len(positive))
    anns += [dict(image_id=9, category_id=cat(c), bbox=b.tolist()) for c, b in zip(positive, g1)]
    anns += [dict(image_id=9, category_id=cat(others[0]), bbox=g1[3].tolist())]  # (one category with two ground truths)
    neg[9], nex[9] = [cat(c) for c in negative], [cat(c) for c in others[:10]]
    b1 = jitter_xyxy(rng, random_boxes_xywh(rng, 330))
    where = {int(c): r for r, c in enumerate(c1)}
    for c, b in zip(positive, g1):
        b1[where[int(c)]] = jitter_xyxy(rng, b[None], 3.0 if c % 2 else 0.0)[0]
    s1 = rng.permutation(330)[:330] / 512.0
    s1[:6] = [0.99, 0.98, 0.9, 0.89, 0.88, 0.87]  # (the named classes stay inside the cut)
    rows = rng.permutation(330)
    boxes[1, rows], scores[1, rows], classes[1, rows] = b1, s1.astype(np.float32), c1

    # image 2: ground truths, no detection
    anns += [dict(image_id=15, category_id=cat(c), bbox=b.tolist()) for c, b in zip([7, 7, 300], random_boxes_xywh(rng, 3))]
    # image 3: negatives only; class 50 is not evaluated
    neg[20] = [cat(4), cat(7), cat(99)]
    classes[3, :20] = rng.choice([4, 7, 99, 50], size=20)
    scores[3, :20] = rng.integers(1, 8, size=20) / 8.0

    # image 4: every rule once
    A, B = [10, 10, 40, 40], [200, 200, 40, 40]
    anns += [dict(image_id=31, category_id=cat(10), bbox=A),                                    # 10: not exhaustive
             dict(image_id=31, category_id=cat(11), bbox=A),                                    # 11: two detections on one ground truth
             dict(image_id=31, category_id=cat(12), bbox=[0, 0, 40, 50], ignore=1), dict(image_id=31, category_id=cat(12), bbox=[8, 0, 40, 50]),
             dict(image_id=31, category_id=cat(13), bbox=A), dict(image_id=31, category_id=cat(13), bbox=A),   # 13: equal IoUs
             dict(image_id=31, category_id=cat(14), bbox=[0, 0, 1, 1]), dict(image_id=31, category_id=cat(15), bbox=[0, 0, 3, 1]),  # IoU 0.5 / 0.75
             dict(image_id=31, category_id=cat(18), bbox=[50, 50, 20, 20]), dict(image_id=31, category_id=cat(18), bbox=[100, 100, 120, 120]),  # small, large
             dict(image_id=31, category_id=cat(18), bbox=[300, 100, 20, 20], area=5000.0)]     # (the JSON's area decides, not the box)
    nex[31], neg[31] = [cat(10)], [cat(17)]
    mixed = [(10, xyxy(*A), .9), (10, xyxy(*B), .8), (11, xyxy(*A), .6), (11, xyxy(*A), .9), (12, [0, 0, 40, 50], .7), (13, xyxy(*A), .9), (13, xyxy(*A), .8),
             (13, xyxy(*A), .7), (14, [0, 0, 2, 1], .5), (15, [0, 0, 4, 1], .5), (16, xyxy(*A), .95), (17, xyxy(*A), .95), (18, [50, 50, 70, 70], .9),
             (18, [100, 100, 220, 220], .8), (18, [300, 100, 320, 120], .7), (18, [400, 300, 410, 310], .6), (18, [300, 300, 500, 470], .55)]
    for r, (c, b, s) in enumerate(mixed):
        classes[4, r], boxes[4, r], scores[4, r] = c, b, s
    counts = np.array([330, 330, 0, 20, len(mixed)], dtype=np.int32)
    gt = lvis_json(IMAGE_IDS, [(k + 1, "rcf"[k % 3]) for k in range(K)], anns, neg, nex)
    return gt, boxes, scores, classes, counts


@pytest.fixture(scope="module")
def case(osr):
    gt, boxes, scores, classes, counts = lvis_case()
    return (gt, boxes, scores, classes, counts) + reference_outputs(gt, IMAGE_IDS, boxes, scores, classes, counts, 300)


@pytest.mark.gpu
def test_flags_rank_and_match_equal_the_numpy_lviseval(osr, case):
    gt, boxes, scores, classes, counts, flags, rank, match = case
    # the case holds what it claims
    assert rank[0].max() == 299 and (rank[0, :330] == -1).sum() == 30 and (rank[:, 330:] == -1).all()
    tie = np.nonzero(scores[0, :330] == np.float32(701 / 1024.0))[0]
    assert len(tie) == 2 and rank[0, tie[0]] == 299 and rank[0, tie[1]] == -1  # the earlier row is kept
    assert ((flags[0] & 0xffff).any(axis=1) & (rank[0] >= 256)).any() and ((flags[0] >> 16).any(axis=1) & (rank[0] >= 256)).any()
    listed1 = rank[1, :330] >= 0
    assert 40 < listed1.sum() < 84 and rank[1].max() == 0 and (rank[1][np.isin(classes[1], [-1, K])] == -1).all()
    assert all(listed1[classes[1, :330] == c].all() for c in (0, 63, 64, K - 1))
    assert (rank[2] == -1).all() and (rank[3, :20] >= 0).sum() == (classes[3, :20] != 50).sum() and not (flags[3] & 0xffff).any() and not flags[3, :, 0].any()
    m = lambda r, a=0: (int(flags[4, r, a]) & 0x3ff, int(flags[4, r, a]) >> 16)  # noqa: E731  (matched, ignored) at row r
    assert m(0) == (0x3ff, 0) and m(1) == (0, 0x3ff)                         # not exhaustive: matched counts, unmatched is ignored
    assert m(3) == (0x3ff, 0) and m(2) == (0, 0)                             # one TP, one FP
    assert m(4) == (0x3ff, 0x3f0)                                            # the ignored ground truth is taken last, and its match is ignored
    assert match[4, 5, 0, 0] == match[4, 6, 0, 0] + 1 and m(7) == (0, 0)     # equal IoUs: the later ground truth first
    assert m(8) == (0x001, 0) and m(9) == (0x03f, 0)                         # IoU exactly 0.5 and 0.75
    assert rank[4, 10] == -1 and rank[4, 11] == 0 and m(11) == (0, 0)        # not evaluated: gone; negative: a false positive
    assert m(12, 1) == (0x3ff, 0) and m(13, 1) == (0x3ff, 0x3ff) and m(14, 1) == (0x3ff, 0x3ff) and m(15, 1) == (0, 0) and m(16, 1) == (0, 0x3ff)
    f, r, mt, _ = device_match(osr, DEV, gt, IMAGE_IDS, boxes, scores, classes, counts, 300)
    assert np.array_equal(r, rank)
    assert np.array_equal(f, flags)
    assert np.array_equal(mt, match)
    f2, r2, mt2, _ = device_match(osr, DEV, gt, IMAGE_IDS, boxes, scores, classes, counts, 300)  # repeats are bit-identical
    assert np.array_equal(f2, f) and np.array_equal(r2, r) and np.array_equal(mt2, mt)


@pytest.mark.gpu
def test_at_the_limit_of_512_no_row_is_cut_and_images_alone_equal_the_batch(osr, case):
    """max_dets = 512, the kernel's limit, is more than cap: the group of image 0 lists all 330 detections (six per lane) and the second
    kernel's grid is n x cap. Each image alone gives what it gave in the batch."""
    gt, boxes, scores, classes, counts = case[:5]
    flags, rank, match = reference_outputs(gt, IMAGE_IDS, boxes, scores, classes, counts, 512)
    assert rank[0].max() == 329 and (rank[1, :330] >= 0).sum() > (case[6][1, :330] >= 0).sum()
    f, r, m, sim = device_match(osr, DEV, gt, IMAGE_IDS, boxes, scores, classes, counts, 512, want_sim=True)
    assert np.array_equal(r, rank) and np.array_equal(f, flags) and np.array_equal(m, match)
    assert sim.shape == (CAP * len(gt["annotations"]),) and sim[:330 * 70].max() == 1.0  # image 0's block: [rank][ground truth], exact copies among them
    for i in (0, 2, 4):
        f1, r1, _, _ = device_match(osr, DEV, gt, IMAGE_IDS[i:i + 1], boxes[i:i + 1], scores[i:i + 1], classes[i:i + 1], counts[i:i + 1], 512)
        assert np.array_equal(f1[0], f[i]) and np.array_equal(r1[0], r[i])
    empty = device_match(osr, DEV, gt, [], boxes[:0], scores[:0], classes[:0], counts[:0], 300)
    assert empty[0].shape == (0, CAP, 4) and empty[1].shape == (0, CAP)
