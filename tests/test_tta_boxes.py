"""osr_tta_boxes_to_original / osr_tta_boxes_to_augmented against a numpy fp32 restatement of [d2]'s transform lists, bit for bit.

An augmentation of an input with image (hi, wi) and output resolution (ho, wo) is [resize (ho, wo) -> (hi, wi), only when they
differ], resize (hi, wi) -> (ha, wa), [hflip(wa)]. A resize multiplies x by f32(w'/w) and y by f32(h'/h) (ratio in double, rounded
once), a flip is f32(wa) - x; after each step the box is (min x, min y, max x, max y) of its corners.

n = 2, topk = 8: image 0 has (ho, wo) != (hi, wi), image 1 has them equal; a flipped augmentation with odd wa (85); scores at 1e-8
(no candidate) and nextafter(1e-8, 1) (a candidate); a NaN coordinate and an inf score (no candidates); a box that clips to zero
width (stays a candidate); padding rows are never candidates; an image with count 0.

n = 3, topk = 100 (counts of three entries): 300 rows, one per thread, in two 256-thread blocks; image 2 (rows 200 .. 299) straddles
the block boundary, so `img = t / topk` and the candidate row `img * cap + slot + j` are decoded in a second block. Images of
800 x 1067 with output resolutions 480 x 640 (differs), 800 x 1067 (equal) and 1200 x 1601 (larger); the augmentation 1200 x 1600
is an up-scaling whose ratio 1600 / 1067 is above 1 and no fp32 number. Counts (100, 37, 0) leave the second block nothing but
padding rows, (64, 0, 100) fill it with detections. Every output buffer is the test's own, pre-filled with -5."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.tta_common import forward_box as _forward, inverse_box as _inverse  # the numpy fp32 restatement

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
# counts of n entries choose the geometry: n -> (topk, sizes (n, 4) {hi, wi, ho, wo}, the scale of the (64, 85)-space detections)
GEOMETRY = {
    2: (8, np.array([[96, 128, 120, 160], [96, 128, 96, 128]], dtype=np.int32), 1.0),
    3: (100, np.array([[800, 1067, 480, 640], [800, 1067, 800, 1067], [800, 1067, 1200, 1601]], dtype=np.int32), 12.5),
}
AUGS = [(64, 85, True), (64, 85, False), (120, 160, True), (1200, 1600, True), (1200, 1600, False)]
AUG_IDS = ["64x85-flip", "64x85", "120x160-flip", "1200x1600-flip", "1200x1600"]


def _detections(counts):
    """Boxes in a (64, 85) augmentation's space times the geometry's scale, with the edge rows of the module docstring in image 0."""
    n = len(counts)
    topk, _, scale = GEOMETRY[n]
    rng = np.random.RandomState(5)
    x0 = rng.uniform(0, 50, size=(n, topk)).astype(F)
    y0 = rng.uniform(0, 40, size=(n, topk)).astype(F)
    boxes = np.stack([x0, y0, x0 + rng.uniform(2, 30, size=(n, topk)).astype(F), y0 + rng.uniform(2, 20, size=(n, topk)).astype(F)], axis=2)
    scores = rng.uniform(0.05, 1.0, size=(n, topk)).astype(F)
    classes = rng.randint(0, 5, size=(n, topk)).astype(np.int64)
    scores[0, 1] = F(1e-8)                        # not a candidate: the test is score > 1e-8
    scores[0, 2] = np.nextafter(F(1e-8), F(1))    # a candidate
    boxes[0, 3, 0] = np.nan                       # a NaN coordinate
    scores[0, 4] = np.inf                         # an inf score
    boxes[0, 5] = (F(90), F(10), F(99), F(20))    # right of the (64, 85) image: clips to zero width at x = wo, stays a candidate
    boxes = boxes * F(scale)                      # (scale 1: the same bits)
    for i, c in enumerate(counts):                # rows beyond the count hold garbage that must not come through
        boxes[i, c:] = 777.0
        scores[i, c:] = 0.9
    return boxes, scores, classes


def _reference_to_original(boxes, scores, classes, counts, sizes, ha, wa, flip):
    n, topk = scores.shape
    rb = np.zeros((n, topk, 4), dtype=F)
    rs = np.zeros((n, topk), dtype=F)
    rc = np.full((n, topk), -1, dtype=np.int32)
    cand = np.zeros((n, topk), dtype=np.int32)
    for i in range(n):
        ho, wo = int(sizes[i, 2]), int(sizes[i, 3])
        for j in range(counts[i]):
            b = _inverse(boxes[i, j].copy(), sizes[i], ha, wa, flip)
            fin = bool(np.isfinite(b).all() and np.isfinite(scores[i, j]))
            with np.errstate(invalid="ignore"):
                b = np.array([np.clip(b[0], F(0), F(wo)), np.clip(b[1], F(0), F(ho)), np.clip(b[2], F(0), F(wo)), np.clip(b[3], F(0), F(ho))], dtype=F)
            rb[i, j], rs[i, j], rc[i, j] = b, scores[i, j], classes[i, j]
            cand[i, j] = int(fin and scores[i, j] > F(1e-8))
    return rb, rs, rc, cand


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _to_augmented(osr, boxes, cnt, sizes, ha, wa, flip):
    """osr_tta_boxes_to_augmented into a buffer of the test's own, pre-filled with -5 (the ops wrapper allocates with torch.empty)."""
    n, topk = int(boxes.shape[0]), int(boxes.shape[1])
    out = torch.full((n, topk, 4), -5.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    status = osr._lib.load().osr_tta_boxes_to_augmented(p(boxes), p(cnt), p(sizes), n, topk, ha, wa, int(flip), p(out),
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("counts", [(7, 8), (7, 0), (100, 37, 0), (64, 0, 100)], ids=["counts-7-8", "counts-7-0", "counts-100-37-0", "counts-64-0-100"])
@pytest.mark.parametrize("ha, wa, flip", AUGS, ids=AUG_IDS)
def test_boxes_to_original(osr, counts, ha, wa, flip):
    ops = osr.ops
    n = len(counts)
    topk, sizes, _ = GEOMETRY[n]
    assert n == 2 or (n * topk > 256 and topk % 256 != 0 and 256 % topk != 0), "three images must straddle a block boundary"
    boxes, scores, classes = _detections(counts)
    rb, rs, rc, rcand = _reference_to_original(boxes, scores, classes, counts, sizes, ha, wa, flip)
    a_total, slot = 3, 1  # the middle third of a three-augmentation candidate list; the other rows must stay untouched
    cap = a_total * topk
    c_boxes = torch.full((n, cap, 4), -5.0, device=DEV)
    c_scores = torch.full((n, cap), -5.0, device=DEV)
    c_cls = torch.full((n, cap), -5, dtype=torch.int32, device=DEV)
    c_cand = torch.full((n, cap), -5, dtype=torch.int32, device=DEV)
    ops.tta_boxes_to_original(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(classes).to(DEV),
                              torch.tensor(counts, dtype=torch.int32, device=DEV), torch.from_numpy(sizes).to(DEV), ha, wa, flip, slot * topk,
                              c_boxes, c_scores, c_cls, c_cand)
    torch.cuda.synchronize()
    lo, hi = slot * topk, (slot + 1) * topk
    gb, gs, gc, gcand = (t.cpu().numpy() for t in (c_boxes, c_scores, c_cls, c_cand))
    for t in (gb, gs, gc, gcand):  # rows of the other augmentations, in every image
        assert (t[:, :lo] == -5).all() and (t[:, hi:] == -5).all()
    assert np.array_equal(gcand[:, lo:hi], rcand)  # (a row no thread wrote still holds -5 in all four lists)
    assert np.array_equal(gc[:, lo:hi], rc)
    assert np.array_equal(_bits(gs[:, lo:hi]), _bits(rs))
    finite = np.isfinite(rb).all(axis=2)  # (the row with a NaN coordinate is compared through its cand flag only)
    assert np.array_equal(_bits(gb[:, lo:hi][finite]), _bits(rb[finite]))
    assert not np.isfinite(gb[0, lo + 3]).all()
    # the documented rows
    assert rcand[0, 1] == 0 and rcand[0, 2] == 1 and rcand[0, 3] == 0 and rcand[0, 4] == 0
    if counts[0] == 7:
        assert rcand[0, 7] == 0 and (gb[0, lo + 7] == 0).all()  # padding
        if (ha, wa, flip) == (64, 85, False):
            assert rcand[0, 5] == 1 and rb[0, 5, 0] == rb[0, 5, 2] == 160.0  # clipped to zero width, still a candidate
    for i in range(n):
        if counts[i] == 0:
            assert (gcand[i, lo:hi] == 0).all() and (gb[i, lo:hi] == 0).all()
    assert int(rcand.sum()) >= 4


@pytest.mark.parametrize("ha, wa, flip, counts", [a + ((6, 3),) for a in AUGS[:3]] + [a + (c,) for a in AUGS for c in ((100, 37, 0), (64, 0, 100))],
                         ids=AUG_IDS[:3] + [f"{a}-counts-{c}" for a in AUG_IDS for c in ("100-37-0", "64-0-100")])
def test_boxes_to_augmented_and_round_trip(osr, ha, wa, flip, counts):
    ops = osr.ops
    n = len(counts)
    topk, SIZES, _ = GEOMETRY[n]
    rng = np.random.RandomState(9)
    boxes = np.zeros((n, topk, 4), dtype=F)
    for i in range(n):  # interior boxes of each image's output resolution
        ho, wo = int(SIZES[i, 2]), int(SIZES[i, 3])
        x0 = rng.uniform(1, wo * 0.6, size=topk).astype(F)
        y0 = rng.uniform(1, ho * 0.6, size=topk).astype(F)
        boxes[i] = np.stack([x0, y0, x0 + rng.uniform(2, wo * 0.3, size=topk).astype(F), y0 + rng.uniform(2, ho * 0.3, size=topk).astype(F)], axis=1)
    ref = np.zeros_like(boxes)
    for i in range(n):
        for j in range(counts[i]):
            ref[i, j] = _forward(boxes[i, j].copy(), SIZES[i], ha, wa, flip)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    sizes = torch.from_numpy(SIZES).to(DEV)
    got = _to_augmented(osr, torch.from_numpy(boxes).to(DEV), cnt, sizes, ha, wa, flip)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref))  # (zeros beyond the counts included; an unwritten row holds -5)
    # inverse then forward of an interior box: at most 2 ulp per step, three steps at the most -> 6 ulp of the coordinate
    aug_boxes = torch.from_numpy(ref).to(DEV)
    c_boxes = torch.full((n, topk, 4), -5.0, device=DEV)
    c_scores = torch.full((n, topk), -5.0, device=DEV)
    c_cls = torch.full((n, topk), -5, dtype=torch.int32, device=DEV)
    c_cand = torch.full((n, topk), -5, dtype=torch.int32, device=DEV)
    ops.tta_boxes_to_original(aug_boxes, torch.full((n, topk), 0.5, device=DEV), torch.zeros((n, topk), dtype=torch.int64, device=DEV), cnt, sizes,
                              ha, wa, flip, 0, c_boxes, c_scores, c_cls, c_cand)
    back = _to_augmented(osr, c_boxes, cnt, sizes, ha, wa, flip)
    back = back.cpu().numpy()
    worst = 0.0
    for i in range(n):
        assert (c_cand[i, :counts[i]] == 1).all() and (c_cand[i, counts[i]:] == 0).all()
        for j in range(counts[i]):
            ulps = np.abs(back[i, j].astype(np.float64) - ref[i, j].astype(np.float64)) / np.spacing(np.abs(ref[i, j])).astype(np.float64)
            worst = max(worst, float(ulps.max()))
    print(f"round trip: worst {worst:.2f} ulp")
    assert worst <= 6.0
