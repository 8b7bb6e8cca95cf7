"""osr_panoptic_combine (csrc/osr_panoptic.hip) against detectron2's loop (tests/panoptic_common.py combine_reference): exact equality
of the map, the segment table, the scores and the count on the 40 x 56 scene that reaches every branch (asserted on the CPU in
tests/test_panoptic_reference.py), on the same instances in shuffled order, with no instance, with a mask on the image border, on a
plane that is no multiple of 64 pixels with many random instances, and the k > 1024 refusal.

Past the first block (the inputs' reach is asserted on the CPU in tests/test_panoptic_reference.py): a 300 x 333 plane of 1561 words,
where pc_walk_kernel's threads take a second stride and row ranges start past word 1024, with bool and uint8 masks and a count above k;
k = 1024 instances with 255 stuff labels, the full table; instances exactly on both thresholds; labels outside 0 .. 255."""
import pytest
import torch

from tests.panoptic_common import (LIMITS_THRESHOLDS, RAGGED_THRESHOLDS, SCENE_THRESHOLDS, combine_boundary_scene, combine_limits,
                                   combine_ragged_plane, combine_reference, combine_rounded_threshold_scene, combine_scene,
                                   combine_scene_with_ignored_labels, f32, segments_info_reference)

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


def test_an_image_sized_ragged_plane(osr):
    """300 x 333 = 1561 words, the last one partial: instance 0's row range is longer than 1024 words (the second stride of both word
    loops), instances 1, 2 and 11 are kept with a first word >= 1024, clipped and rejected instances cross word 1024; pc_pack_kernel
    runs seven workgroups per instance."""
    table, events = _run_and_compare(osr, *combine_ragged_plane(), RAGGED_THRESHOLDS)
    assert {"kept", "clipped", "overlap", "break", "stuff_kept", "stuff_small"} <= {e[0] for e in events}
    assert len(table) == 63 and sum(r[0] for r in table) == 15


def test_uint8_masks_with_any_non_zero_byte_and_a_count_above_k(osr):
    masks, scores, classes, labels = combine_ragged_plane()
    k, h, w = masks.shape
    fill = torch.tensor([2, 128, 255], dtype=torch.uint8)[(torch.arange(h * w) % 3).reshape(h, w)]
    bytes_ = masks.to(torch.uint8) * fill  # non-zero = set
    assert bytes_.dtype == torch.uint8 and set(torch.unique(bytes_).tolist()) == {0, 2, 128, 255} and torch.equal(bytes_ != 0, masks)
    table, _ = _run_and_compare(osr, bytes_, scores, classes, labels, RAGGED_THRESHOLDS)
    assert len(table) == 63
    _run_and_compare(osr, masks, scores, classes, labels, RAGGED_THRESHOLDS, count=k + 1000)  # a count above k clamps to k


def test_the_limits_together(osr):
    """k = 1024 single-pixel instances, all kept, and 255 stuff labels of two pixels each: 1279 rows, the table's capacity. The O(k^2)
    ranking runs on long runs of equal scores. Then the scores shifted by 0.25: the walk stops at the reference's instance."""
    masks, scores, classes, labels = combine_limits()
    table, events = _run_and_compare(osr, masks, scores, classes, labels, LIMITS_THRESHOLDS)
    assert len(table) == 1024 + 255 and not any(e[0] == "break" for e in events)
    table, events = _run_and_compare(osr, masks, (scores - 0.25).contiguous(), classes, labels, LIMITS_THRESHOLDS)
    n = sum(r[0] for r in table)
    assert 400 <= n <= 624 and events[n][0] == "break" and len(table) == n + 255


@pytest.mark.parametrize("frac", [0.5, 0.25])
def test_an_instance_exactly_on_either_threshold_is_kept(osr, frac):
    """inter / area == overlap_thresh and score == instances_confidence_thresh, both dyadic: kept (`>` and `<`); one column more is an
    overlap, the next fp32 score below ends the walk."""
    conf = 0.625
    table, events = _run_and_compare(osr, *combine_boundary_scene(frac, conf), dict(overlap_thresh=frac, stuff_area_limit=10, instances_confidence_thresh=conf))
    assert [r[2] for r in table] == [0, 1, 3, -1] and ("overlap", 2) in events and ("break", 4) in events


def test_a_non_dyadic_threshold_compares_as_the_c_float(osr):
    """0.7 reaches the kernel as the float 0.699999988 and is widened to double there (include/osr.h): the reference gets that value."""
    masks, scores, classes, labels = combine_rounded_threshold_scene()
    ops = osr.ops
    th = dict(overlap_thresh=f32(0.7), stuff_area_limit=10, instances_confidence_thresh=f32(0.7))
    pan_ref, table_ref, scores_ref, events = combine_reference(masks, scores, classes, labels, **th)
    assert ("overlap", 1) in events and ("kept", 2) in events and ("break", 3) in events
    pan, table, seg_scores, n = ops.panoptic_combine(masks.to(DEV), scores.to(DEV), classes.to(DEV), labels.to(DEV), 0.7, 10, 0.7)  # the plain Python 0.7
    assert int(n.item()) == len(table_ref) and torch.equal(pan.cpu(), pan_ref) and table.cpu()[:len(table_ref)].tolist() == table_ref
    assert seg_scores.cpu()[:len(table_ref)].tolist() == [f32(s) for s in scores_ref]
    _run_and_compare(osr, masks, scores, classes, labels, th)


def test_labels_outside_0_to_255_paint_nothing(osr):
    masks, scores, classes, dirty, clean = combine_scene_with_ignored_labels()
    th = dict(SCENE_THRESHOLDS, stuff_area_limit=20)
    ops = osr.ops
    pan_ref, table_ref, scores_ref, _ = combine_reference(masks, scores, classes, clean, **th)
    args = (masks.to(DEV), scores.to(DEV), classes.to(DEV), dirty.to(DEV), th["overlap_thresh"], th["stuff_area_limit"], th["instances_confidence_thresh"])
    pan, table, seg_scores, n = ops.panoptic_combine(*args)
    assert int(n.item()) == len(table_ref) and torch.equal(pan.cpu(), pan_ref) and table.cpu()[:len(table_ref)].tolist() == table_ref
    assert bool((pan.cpu()[(dirty != clean)] == 0).all())
    assert ops.segments_info_from_table(table, seg_scores, n) == segments_info_reference(table_ref, [f32(s) for s in scores_ref])
    assert all(torch.equal(a, b) for a, b in zip(ops.panoptic_combine(*args), (pan, table, seg_scores, n)))
