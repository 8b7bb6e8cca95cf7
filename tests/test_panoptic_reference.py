"""The inputs of the Panoptic FPN GPU tests are well conditioned, judged by the torch-CPU references alone (tests/panoptic_common.py and
the CPU network of tests/test_panoptic_engine.py): the share of near-tie pixels the label comparisons exclude, and the branches of
detectron2's combine loop that the scenes reach; for the image-sized and limit inputs, that they reach the word ranges, the table
capacity, the threshold boundaries and the class passes they are built for."""
import pytest
import torch

from tests.panoptic_common import (IGNORED_LABELS, LIMITS_THRESHOLDS, RAGGED_THRESHOLDS, RESAMPLE_CASES, RESAMPLE_WIDE_CASES, SCENE_THRESHOLDS,
                                   below, combine_boundary_scene, combine_limits, combine_ragged_plane, combine_reference,
                                   combine_rounded_threshold_scene, combine_scene, combine_scene_with_ignored_labels, f32, resample_logits,
                                   resample_reference, resample_wide_logits, segments_info_reference, top_two_gap, word_range)


def test_resample_near_ties_are_rare():
    logits = resample_logits()
    for crop, out_hw in RESAMPLE_CASES:
        ref = resample_reference(logits, crop, out_hw)
        assert tuple(ref.shape) == (54,) + out_hw
        share = float((top_two_gap(ref) < 1e-4 * float(ref.abs().max())).double().mean())
        print(f"[reference] resample {crop} -> {out_hw}: {100 * share:.3f} % near ties")
        assert share <= 0.005


def test_the_identity_resample_is_the_x4_upsample():
    logits = resample_logits()
    ref = resample_reference(logits, (64, 96), (64, 96))
    x4 = torch.nn.functional.interpolate(logits.double().permute(2, 0, 1)[None], scale_factor=4, mode="bilinear", align_corners=False)[0]
    assert torch.equal(ref, x4)


def test_the_scene_reaches_every_branch_of_the_loop():
    masks, scores, classes, labels = combine_scene()
    pan, table, seg_scores, events = combine_reference(masks, scores, classes, labels, **SCENE_THRESHOLDS)
    assert events == [("kept", 0), ("overlap", 1), ("clipped", 2), ("kept", 2), ("empty", 3), ("clipped", 4), ("kept", 4),
                      ("break", 5), ("stuff_kept", 3), ("stuff_small", 5), ("stuff_small", 7), ("stuff_small", 9)]
    assert table == [[1, 2, 0, 400], [1, 1, 2, 300], [1, 0, 4, 360], [0, 3, -1, 500]]
    # instance 4 sits exactly on the overlap threshold and is kept: the test is `>`
    inter4 = int((masks[4] & (masks[0] | masks[2])).sum())
    assert inter4 * 2 == int(masks[4].sum()) == 720
    assert int((pan == 4).sum()) == 500 and int(((labels == 7) & (pan == 0)).sum()) == 40
    info = segments_info_reference(table, seg_scores)
    assert [d["id"] for d in info] == [1, 2, 3, 4] and [d["isthing"] for d in info] == [True, True, True, False]
    assert info[3] == {"id": 4, "isthing": False, "category_id": 3, "area": 500}


def test_engine_reference_near_ties_are_few():
    """The label comparison of tests/test_panoptic_engine.py excludes pixels whose reference gap is under 1e-3 max |ref|: at most 5 %."""
    from tests.test_panoptic_engine import OUT_SIZES, setup
    s = setup()
    assert float(s["logits"].std()) > 0.5
    for ref, out_hw in zip(s["sem"], OUT_SIZES):
        assert tuple(ref.shape) == (54,) + out_hw
        share = float((top_two_gap(ref) < 1e-3 * float(ref.abs().max())).double().mean())
        print(f"[reference] engine sem_seg {out_hw}: {100 * share:.3f} % near ties, {len(torch.unique(ref.argmax(dim=0)))} labels present")
        assert share <= 0.05
        assert len(torch.unique(ref.argmax(dim=0))) >= 5


def test_the_ragged_plane_leaves_the_first_1024_words():
    """pc_walk_kernel gives thread t the words t, t + 1024, ... of an instance's row range: the plane has 1561 words, and kept, clipped
    and rejected instances lie past, across and over more than 1024 of them. Seed 4 with this draw order: 63 rows, 15 of them things;
    0 spans all 1561 words; 1, 2 and 11 are kept past word 1024; 16 and 43 are clipped across it; 3 is an overlap."""
    masks, scores, classes, labels = combine_ragged_plane()
    h, w = labels.shape
    assert (h, w, masks.shape[0]) == (300, 333, 48) and w % 64 != 0 and (h * w) % 64 != 0 and (h * w + 63) // 64 == 1561
    assert word_range(masks[0], w) == (0, 1561) and word_range(masks[1], w)[0] == 1092 and word_range(masks[2], w) == (1555, 1561)
    pan, table, seg_scores, events = combine_reference(masks, scores, classes, labels, **RAGGED_THRESHOLDS)
    kinds = {e[0] for e in events}
    assert {"kept", "clipped", "overlap", "break", "stuff_kept", "stuff_small"} <= kinds, kinds
    ranges = {kind: [word_range(masks[i], w) for k_, i in events if k_ == kind] for kind in ("kept", "clipped", "overlap")}
    print(f"[reference] ragged plane: {len(table)} rows, {sum(r[0] for r in table)} things; kept past word 1024: "
          f"{[i for k_, i in events if k_ == 'kept' and word_range(masks[i], w)[0] >= 1024]}")
    assert any(lo >= 1024 for lo, hi in ranges["kept"])
    assert any(hi - lo > 1024 for lo, hi in ranges["kept"])
    assert any(lo < 1024 < hi for lo, hi in ranges["overlap"]) and any(lo < 1024 < hi for lo, hi in ranges["clipped"])
    assert ("overlap", 3) in events and ("clipped", 1) in events and ("kept", 2) in events
    assert int(pan[299, 332]) > 0 and table[0][:3] == [1, int(classes[0]), 0]  # the last pixel of the partial last word is painted


def test_the_limits_fill_the_table():
    """k = 1024 kept instances and 255 kept labels: 1279 rows, the capacity k + 255; equal scores run long; a shift of the scores
    ends the walk about half way."""
    masks, scores, classes, labels = combine_limits()
    assert masks.shape == (1024, 32, 48) and bool((masks.reshape(1024, -1).sum(1) == 1).all()) and int(masks.any(0).sum()) == 1024
    assert len(torch.unique(scores)) == 8 and float(scores.min()) == 0.5 and float(scores.max()) == 1.0
    free = labels[~masks.any(0)]
    assert sorted(free.tolist()) == [0, 0] + sorted(list(range(1, 256)) * 2)
    pan, table, seg_scores, events = combine_reference(masks, scores, classes, labels, **LIMITS_THRESHOLDS)
    assert len(table) == 1279 and sum(r[0] for r in table) == 1024 and [r[1] for r in table[1024:]] == list(range(1, 256))
    things = [r[2] for r in table[:1024]]
    order = sorted(range(1024), key=lambda i: (-float(scores[i]), i))  # equal scores: the lower index first
    assert things == order and any(scores[a] == scores[b] and a + 1 < b for a, b in zip(things, things[1:]))
    shifted = scores - 0.25
    pan, table, seg_scores, events = combine_reference(masks, shifted, classes, labels, **LIMITS_THRESHOLDS)
    n = sum(r[0] for r in table)
    assert 400 <= n <= 624 and events[n][0] == "break" and n == int((shifted >= 0.5).sum())
    assert len(table) - n == 255  # the instance pixels left unpainted only add to the labels' areas


@pytest.mark.parametrize("frac", [0.5, 0.25])
def test_the_boundary_scene_sits_on_both_thresholds(frac):
    conf = 0.625
    masks, scores, classes, labels = combine_boundary_scene(frac, conf)
    assert f32(frac) == frac and f32(conf) == conf  # dyadic: the float the C interface takes is the reference's double
    pan, table, seg_scores, events = combine_reference(masks, scores, classes, labels, overlap_thresh=frac, stuff_area_limit=10,
                                                       instances_confidence_thresh=conf)
    assert events[:7] == [("kept", 0), ("clipped", 1), ("kept", 1), ("overlap", 2), ("kept", 3), ("break", 4), ("stuff_kept", 4)]
    inter = int((masks[1] & masks[0]).sum())
    assert inter == frac * int(masks[1].sum()) == frac * 64
    assert float(scores[3]) == conf and float(scores[4]) == below(conf) < conf and float(scores[5]) < float(scores[4])
    assert [r[2] for r in table] == [0, 1, 3, -1] and int(pan[masks[5]].max()) == 0


def test_a_non_dyadic_threshold_is_the_c_float():
    """include/osr.h compares in double with `(double)overlap_thresh` of a float: 0.7 there is 0.699999988. With that value instance 1
    (7 of 10 pixels covered) is an overlap and instance 2 (score float32(0.7)) is kept; with the double 0.7 both go the other way."""
    masks, scores, classes, labels = combine_rounded_threshold_scene()
    t = f32(0.7)
    assert t < 0.7 and float(scores[2]) == t
    th = dict(overlap_thresh=t, stuff_area_limit=10, instances_confidence_thresh=t)
    pan, table, seg_scores, events = combine_reference(masks, scores, classes, labels, **th)
    assert events[:4] == [("kept", 0), ("overlap", 1), ("kept", 2), ("break", 3)] and [r[2] for r in table] == [0, 2, -1]
    th = dict(overlap_thresh=0.7, stuff_area_limit=10, instances_confidence_thresh=0.7)
    pan, table, seg_scores, events = combine_reference(masks, scores, classes, labels, **th)
    assert events[:4] == [("kept", 0), ("clipped", 1), ("kept", 1), ("break", 2)]


def test_ignored_labels_would_take_rows_if_they_counted():
    masks, scores, classes, dirty, clean = combine_scene_with_ignored_labels()
    th = dict(SCENE_THRESHOLDS, stuff_area_limit=20)
    assert {int(v) for v in torch.unique(dirty)} >= set(IGNORED_LABELS)
    assert all(int((dirty == v).sum()) >= 20 for v in IGNORED_LABELS)
    pan_c, table_c, _, _ = combine_reference(masks, scores, classes, clean, **th)
    pan_d, table_d, _, _ = combine_reference(masks, scores, classes, dirty, **th)
    assert len(table_d) == len(table_c) + 3 and not torch.equal(pan_c, pan_d)


def test_wide_resample_near_ties_are_rare_and_every_pass_wins():
    """More than 56 classes go through the LDS tile in passes of 56 with the running argmax carried across: in cases b and c the
    reference's labels come from the second (>= 56) and the third (>= 112) pass often enough to show a lost carry."""
    for case in RESAMPLE_WIDE_CASES:
        name, c, pitch, (h4, w4), crop, out_hw = case
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            ref = resample_reference(resample_wide_logits(case).to(dtype), crop, out_hw)
            assert tuple(ref.shape) == (c,) + out_hw and pitch % 4 == 0 and c <= pitch < c + 4
            share = float((top_two_gap(ref) < 1e-4 * float(ref.abs().max())).double().mean())
            lab = ref.argmax(dim=0)
            third, second = float((lab >= 112).double().mean()), float((lab >= 56).double().mean())
            print(f"[reference] resample {name} {str(dtype)[6:]}: {100 * share:.3f} % near ties; labels >= 56: {100 * second:.0f} %, >= 112: {100 * third:.0f} %")
            assert share <= 0.005
            if name in ("b", "c"):
                assert third >= 0.10 and second >= 0.30
    assert RESAMPLE_WIDE_CASES[0][1] == 56 + 1 and RESAMPLE_WIDE_CASES[3][3][0] == 1 and RESAMPLE_WIDE_CASES[3][5][1] == 65
    assert RESAMPLE_WIDE_CASES[4][3] == (1, 1)
