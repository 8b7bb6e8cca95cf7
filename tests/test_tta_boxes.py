"""osr_tta_boxes_to_original / osr_tta_boxes_to_augmented against a numpy fp32 restatement of [d2]'s transform lists, bit for bit.

An augmentation of an input with image (hi, wi) and output resolution (ho, wo) is [resize (ho, wo) -> (hi, wi), only when they
differ], resize (hi, wi) -> (ha, wa), [hflip(wa)]. A resize multiplies x by f32(w'/w) and y by f32(h'/h) (ratio in double, rounded
once), a flip is f32(wa) - x; after each step the box is (min x, min y, max x, max y) of its corners.

n = 2, topk = 8: image 0 has (ho, wo) != (hi, wi), image 1 has them equal; a flipped augmentation with odd wa (85); scores at 1e-8
(no candidate) and nextafter(1e-8, 1) (a candidate); a NaN coordinate and an inf score (no candidates); a box that clips to zero
width (stays a candidate); padding rows are never candidates; an image with count 0."""
import numpy as np
import pytest
import torch

from tests.tta_common import forward_box as _forward, inverse_box as _inverse  # the numpy fp32 restatement

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, TOPK = 2, 8
HI, WI = 96, 128
SIZES = np.array([[HI, WI, 120, 160], [HI, WI, HI, WI]], dtype=np.int32)
F = np.float32


def _detections(counts):
    """Boxes in a (64, 85) augmentation's space, with the edge rows of the module docstring in image 0."""
    rng = np.random.RandomState(5)
    x0 = rng.uniform(0, 50, size=(N, TOPK)).astype(F)
    y0 = rng.uniform(0, 40, size=(N, TOPK)).astype(F)
    boxes = np.stack([x0, y0, x0 + rng.uniform(2, 30, size=(N, TOPK)).astype(F), y0 + rng.uniform(2, 20, size=(N, TOPK)).astype(F)], axis=2)
    scores = rng.uniform(0.05, 1.0, size=(N, TOPK)).astype(F)
    classes = rng.randint(0, 5, size=(N, TOPK)).astype(np.int64)
    scores[0, 1] = F(1e-8)                        # not a candidate: the test is score > 1e-8
    scores[0, 2] = np.nextafter(F(1e-8), F(1))    # a candidate
    boxes[0, 3, 0] = np.nan                       # a NaN coordinate
    scores[0, 4] = np.inf                         # an inf score
    boxes[0, 5] = (F(90), F(10), F(99), F(20))    # right of the (64, 85) image: clips to zero width at x = wo, stays a candidate
    for i, c in enumerate(counts):                # rows beyond the count hold garbage that must not come through
        boxes[i, c:] = 777.0
        scores[i, c:] = 0.9
    return boxes, scores, classes


def _reference_to_original(boxes, scores, classes, counts, ha, wa, flip):
    rb = np.zeros((N, TOPK, 4), dtype=F)
    rs = np.zeros((N, TOPK), dtype=F)
    rc = np.full((N, TOPK), -1, dtype=np.int32)
    cand = np.zeros((N, TOPK), dtype=np.int32)
    for i in range(N):
        ho, wo = int(SIZES[i, 2]), int(SIZES[i, 3])
        for j in range(counts[i]):
            b = _inverse(boxes[i, j].copy(), SIZES[i], ha, wa, flip)
            fin = bool(np.isfinite(b).all() and np.isfinite(scores[i, j]))
            with np.errstate(invalid="ignore"):
                b = np.array([np.clip(b[0], F(0), F(wo)), np.clip(b[1], F(0), F(ho)), np.clip(b[2], F(0), F(wo)), np.clip(b[3], F(0), F(ho))], dtype=F)
            rb[i, j], rs[i, j], rc[i, j] = b, scores[i, j], classes[i, j]
            cand[i, j] = int(fin and scores[i, j] > F(1e-8))
    return rb, rs, rc, cand


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.mark.parametrize("counts", [(7, 8), (7, 0)], ids=["counts-7-8", "counts-7-0"])
@pytest.mark.parametrize("ha, wa, flip", [(64, 85, True), (64, 85, False), (120, 160, True)], ids=["64x85-flip", "64x85", "120x160-flip"])
def test_boxes_to_original(osr, counts, ha, wa, flip):
    ops = osr.ops
    boxes, scores, classes = _detections(counts)
    rb, rs, rc, rcand = _reference_to_original(boxes, scores, classes, counts, ha, wa, flip)
    a_total, slot = 3, 1  # the middle third of a three-augmentation candidate list; the other rows must stay untouched
    cap = a_total * TOPK
    c_boxes = torch.full((N, cap, 4), -5.0, device=DEV)
    c_scores = torch.full((N, cap), -5.0, device=DEV)
    c_cls = torch.full((N, cap), -5, dtype=torch.int32, device=DEV)
    c_cand = torch.full((N, cap), -5, dtype=torch.int32, device=DEV)
    ops.tta_boxes_to_original(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(classes).to(DEV),
                              torch.tensor(counts, dtype=torch.int32, device=DEV), torch.from_numpy(SIZES).to(DEV), ha, wa, flip, slot * TOPK,
                              c_boxes, c_scores, c_cls, c_cand)
    torch.cuda.synchronize()
    lo, hi = slot * TOPK, (slot + 1) * TOPK
    gb, gs, gc, gcand = (t.cpu().numpy() for t in (c_boxes, c_scores, c_cls, c_cand))
    for t in (gb, gs, gc, gcand):  # rows of the other augmentations
        assert (t[:, :lo] == -5).all() and (t[:, hi:] == -5).all()
    assert np.array_equal(gcand[:, lo:hi], rcand)
    assert np.array_equal(gc[:, lo:hi], rc)
    assert np.array_equal(_bits(gs[:, lo:hi]), _bits(rs))
    finite = np.isfinite(rb).all(axis=2)  # (the row with a NaN coordinate is compared through its cand flag only)
    assert np.array_equal(_bits(gb[:, lo:hi][finite]), _bits(rb[finite]))
    assert not np.isfinite(gb[0, lo + 3]).all()
    # the documented rows
    if counts[0] == 7:
        assert rcand[0, 1] == 0 and rcand[0, 2] == 1 and rcand[0, 3] == 0 and rcand[0, 4] == 0
        assert rcand[0, 7] == 0 and (gb[0, lo + 7] == 0).all()  # padding
        if (ha, wa, flip) == (64, 85, False):
            assert rcand[0, 5] == 1 and rb[0, 5, 0] == rb[0, 5, 2] == 160.0  # clipped to zero width, still a candidate
    if counts[1] == 0:
        assert (gcand[1, lo:hi] == 0).all() and (gb[1, lo:hi] == 0).all()
    assert int(rcand.sum()) >= 4


@pytest.mark.parametrize("ha, wa, flip", [(64, 85, True), (64, 85, False), (120, 160, True)], ids=["64x85-flip", "64x85", "120x160-flip"])
def test_boxes_to_augmented_and_round_trip(osr, ha, wa, flip):
    ops = osr.ops
    counts = (6, 3)
    rng = np.random.RandomState(9)
    boxes = np.zeros((N, TOPK, 4), dtype=F)
    for i in range(N):  # interior boxes of each image's output resolution
        ho, wo = int(SIZES[i, 2]), int(SIZES[i, 3])
        x0 = rng.uniform(1, wo * 0.6, size=TOPK).astype(F)
        y0 = rng.uniform(1, ho * 0.6, size=TOPK).astype(F)
        boxes[i] = np.stack([x0, y0, x0 + rng.uniform(2, wo * 0.3, size=TOPK).astype(F), y0 + rng.uniform(2, ho * 0.3, size=TOPK).astype(F)], axis=1)
    ref = np.zeros_like(boxes)
    for i in range(N):
        for j in range(counts[i]):
            ref[i, j] = _forward(boxes[i, j].copy(), SIZES[i], ha, wa, flip)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    sizes = torch.from_numpy(SIZES).to(DEV)
    got = ops.tta_boxes_to_augmented(torch.from_numpy(boxes).to(DEV), cnt, sizes, ha, wa, flip)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref))  # (zeros beyond the counts included)
    # inverse then forward of an interior box: at most 2 ulp per step, three steps at the most -> 6 ulp of the coordinate
    aug_boxes = torch.from_numpy(ref).to(DEV)
    c_boxes = torch.empty((N, TOPK, 4), device=DEV)
    c_scores = torch.empty((N, TOPK), device=DEV)
    c_cls = torch.empty((N, TOPK), dtype=torch.int32, device=DEV)
    c_cand = torch.empty((N, TOPK), dtype=torch.int32, device=DEV)
    ops.tta_boxes_to_original(aug_boxes, torch.full((N, TOPK), 0.5, device=DEV), torch.zeros((N, TOPK), dtype=torch.int64, device=DEV), cnt, sizes,
                              ha, wa, flip, 0, c_boxes, c_scores, c_cls, c_cand)
    back = ops.tta_boxes_to_augmented(c_boxes, cnt, sizes, ha, wa, flip)
    torch.cuda.synchronize()
    back = back.cpu().numpy()
    worst = 0.0
    for i in range(N):
        assert (c_cand[i, :counts[i]] == 1).all()
        for j in range(counts[i]):
            ulps = np.abs(back[i, j].astype(np.float64) - ref[i, j].astype(np.float64)) / np.spacing(np.abs(ref[i, j])).astype(np.float64)
            worst = max(worst, float(ulps.max()))
    print(f"round trip: worst {worst:.2f} ulp")
    assert worst <= 6.0
