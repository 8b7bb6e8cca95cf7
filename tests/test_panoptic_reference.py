"""The inputs of the Panoptic FPN GPU tests are well conditioned, judged by the torch-CPU references alone (tests/panoptic_common.py and
the CPU network of tests/test_panoptic_engine.py): the share of near-tie pixels the label comparisons exclude, and the branches of
detectron2's combine loop that the scenes reach."""
import torch

from tests.panoptic_common import (RESAMPLE_CASES, SCENE_THRESHOLDS, combine_reference, combine_scene, resample_logits, resample_reference,
                                   segments_info_reference, top_two_gap)


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
