"""osr_panoptic_combine (csrc/osr_panoptic.hip) against detectron2's loop (tests/panoptic_common.py combine_reference): exact equality
of the map, the segment table, the scores and the count on the 40 x 56 scene that reaches every branch (asserted on the CPU in
tests/test_panoptic_reference.py), on the same instances in shuffled order, with no instance, with a mask on the image border, on a
plane that is no multiple of 64 pixels with many random instances, and the k > 1024 refusal."""
import pytest
import torch

from tests.panoptic_common import SCENE_THRESHOLDS, combine_reference, combine_scene, segments_info_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run_and_compare(osr, masks, scores, classes, labels, thresholds, count=None):
    ops = osr.ops
    k = masks.shape[0] if count is None else count
    pan_ref, table_ref, scores_ref, events = combine_reference(masks[:k], scores[:k], classes[:k], labels, **thresholds)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
    args = (masks.to(DEV), scores.to(DEV), classes.to(DEV), labels.to(DEV), thresholds["overlap_thresh"], thresholds["stuff_area_limit"],
            thresholds["instances_confidence_thresh"], cnt)
    pan, table, seg_scores, seg_count = ops.panoptic_combine(*args)
    n = int(seg_count.item())
    assert n == len(table_ref), (n, table_ref)
    assert pan.dtype == torch.int32 and torch.equal(pan.cpu(), pan_ref)
    assert table.cpu()[:n].tolist() == table_ref
    assert seg_scores.cpu()[:n].tolist() == [float(torch.tensor(s, dtype=torch.float32)) for s in scores_ref]
    info = ops.segments_info_from_table(table, seg_scores, seg_count)
    want = segments_info_reference(table_ref, [float(torch.tensor(s, dtype=torch.float32)) for s in scores_ref])
    assert info == want
    again = ops.panoptic_combine(*args)
    assert all(torch.equal(a, b) for a, b in zip(again, (pan, table, seg_scores, seg_count)))
    return table_ref, events


def test_the_scene_reaches_every_branch_and_matches(osr):
    table, events = _run_and_compare(osr, *combine_scene(), SCENE_THRESHOLDS)
    assert table == [[1, 2, 0, 400], [1, 1, 2, 300], [1, 0, 4, 360], [0, 3, -1, 500]]
    assert ("overlap", 1) in events and ("clipped", 2) in events and ("empty", 3) in events and ("break", 5) in events


def test_the_input_order_does_not_matter(osr):
    masks, scores, classes, labels = combine_scene()
    perm = torch.tensor([4, 2, 5, 0, 3, 1])
    table, _ = _run_and_compare(osr, masks[perm].contiguous(), scores[perm].contiguous(), classes[perm].contiguous(), labels, SCENE_THRESHOLDS)
    inv = {int(p): i for i, p in enumerate(perm)}  # original index -> shuffled index
    assert table == [[1, 2, inv[0], 400], [1, 1, inv[2], 300], [1, 0, inv[4], 360], [0, 3, -1, 500]]
    # equal scores: the lower index goes first
    scores2 = torch.tensor([0.9, 0.9, 0.9, 0.9, 0.9, 0.9])
    _run_and_compare(osr, masks, scores2, classes, labels, SCENE_THRESHOLDS)


def test_no_instances_and_a_count_below_k(osr):
    masks, scores, classes, labels = combine_scene()
    table, _ = _run_and_compare(osr, masks[:0].contiguous(), scores[:0].contiguous(), classes[:0].contiguous(), labels, SCENE_THRESHOLDS)
    assert table == [[0, 3, -1, 800], [0, 7, -1, 800]]
    _run_and_compare(osr, masks, scores, classes, labels, SCENE_THRESHOLDS, count=0)
    _run_and_compare(osr, masks, scores, classes, labels, SCENE_THRESHOLDS, count=3)


def test_masks_on_the_image_border_and_a_ragged_plane(osr):
    """37 x 45 = 1665 pixels = 26 words and 1 pixel: rows straddle the 64-pixel words, the last word is partial; masks touch all four
    borders and both corners; thirty random rectangles with random scores exercise the walk order and the overlap test."""
    g = torch.Generator().manual_seed(3)
    h, w, k = 37, 45, 32
    masks = torch.zeros(k, h, w, dtype=torch.bool)
    masks[0, 0:6, 0:7] = True
    masks[1, h - 5:h, w - 9:w] = True
    for i in range(2, k):
        y0, x0 = int(torch.randint(0, h - 4, (1,), generator=g)), int(torch.randint(0, w - 4, (1,), generator=g))
        y1, x1 = y0 + int(torch.randint(2, 16, (1,), generator=g)), x0 + int(torch.randint(2, 16, (1,), generator=g))
        masks[i, y0:min(y1, h), x0:min(x1, w)] = True
    scores = torch.rand(k, generator=g) * 0.5 + 0.4  # (0.4 .. 0.9: some end the walk, none outranks the two border masks)
    scores[0], scores[1] = 0.99, 0.98
    classes = torch.randint(0, 5, (k,), generator=g)
    labels = torch.randint(0, 6, (h // 4 + 1, w // 4 + 1), generator=g).repeat_interleave(4, 0).repeat_interleave(4, 1)[:h, :w].to(torch.int32).contiguous()
    table, events = _run_and_compare(osr, masks, scores, classes, labels, dict(overlap_thresh=0.5, stuff_area_limit=20, instances_confidence_thresh=0.5))
    kinds = {e[0] for e in events}
    assert {"kept", "overlap", "clipped", "break", "stuff_kept"} <= kinds, kinds
    assert table[0][:3] == [1, int(classes[0]), 0] and table[1][:3] == [1, int(classes[1]), 1]


def test_more_than_1024_instances_are_refused(osr):
    ops = osr.ops
    labels = torch.zeros(4, 8, dtype=torch.int32, device=DEV)
    with pytest.raises(osr.OsrError, match="1024"):
        ops.panoptic_combine(torch.zeros(1025, 4, 8, dtype=torch.bool, device=DEV), torch.zeros(1025, device=DEV), torch.zeros(1025, dtype=torch.int64, device=DEV),
                             labels, 0.5, 0, 0.5)
    with pytest.raises(osr.OsrError):
        ops.panoptic_combine(torch.zeros(1, 4, 8, dtype=torch.bool), torch.zeros(1), torch.zeros(1, dtype=torch.int64), labels.cpu(), 0.5, 0, 0.5)
