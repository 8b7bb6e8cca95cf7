"""host/coco_evaluation.py on the CPU: the numpy COCOeval against hand-computed AP / AR and pycocotools' matching rules one at a
time, against the existing OpensetCOCOEval with every category known, computeOks on hand-computed values, the COCOEvaluator on CPU
tensors (results file round trip, segm, sigmas, dispatch), and osr_coco_match's refusals, which need no GPU."""
import ctypes
import json
import logging
import math
import os

import numpy as np
import pytest
import torch

from tests.coco_eval_common import coco_json, det, instances as _instances, register as _register, run_eval, seeded_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one_image(gts, cat_ids=(1,), image_ids=(1,)):
    return coco_json(list(image_ids), list(cat_ids), [dict(image_id=g.pop("image_id", image_ids[0]), category_id=g.pop("category_id", cat_ids[0]), **g) for g in gts])


def _img(ev, img=1, cat=1, area=0):
    """The per-image result of (img, cat) in area range `area`."""
    A, I = len(ev.params.area_rng), len(ev.img_ids)
    return ev.eval_imgs[(ev.cat_ids.index(cat) * A + area) * I + ev.img_ids.index(img)]


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
def test_perfect_detections_score_one(osr):
    boxes = [[10, 10, 20, 20], [50, 50, 40, 40], [100, 20, 100, 100]]  # small, medium, large
    gt = _one_image([dict(bbox=b) for b in boxes])
    ev = run_eval(osr, gt, [det(1, 1, b, 0.9 - 0.1 * i) for i, b in enumerate(boxes)])
    assert ev.stats.shape == (12,)
    assert ev.stats[[0, 1, 2, 3, 4, 5, 8, 9, 10, 11]] == pytest.approx(1.0, abs=1e-12)
    assert ev.stats[6] == pytest.approx(1 / 3, abs=1e-12) and ev.stats[7] == pytest.approx(1.0, abs=1e-12)  # AR@1: one of three found


def test_a_false_positive_above_the_only_true_positive_halves_the_precision(osr):
    """tp = [0, 1], fp = [1, 1]: recall [0, 1], precision [0, 1/2], envelope [1/2, 1/2]. Every one of the 101 recall thresholds reads
    1 / (2 + eps): AP = 1/2, at every IoU threshold (the true positive is exact). AR = 1."""
    gt = _one_image([dict(bbox=[10, 10, 50, 50])])
    ev = run_eval(osr, gt, [det(1, 1, [200, 200, 50, 50], 0.9), det(1, 1, [10, 10, 50, 50], 0.8)])
    assert ev.eval["precision"][:, :, 0, 0, 2] == pytest.approx(0.5, abs=1e-12)
    assert ev.stats[0] == pytest.approx(0.5, abs=1e-12) and ev.stats[8] == pytest.approx(1.0)


def test_a_false_positive_between_two_true_positives_gives_the_101_point_value(osr):
    """tp = [1, 1, 2], fp = [0, 1, 1]: recall [.5, .5, 1], precision [1, 1/2, 2/3], envelope [1, 2/3, 2/3]. searchsorted(left): the 51
    thresholds 0 .. 0.50 read index 0 (precision 1), the 50 thresholds 0.51 .. 1 read index 2 (2/3): AP = (51 + 50 * 2/3) / 101."""
    gt = _one_image([dict(bbox=[10, 10, 50, 50]), dict(bbox=[100, 100, 50, 50])])
    ev = run_eval(osr, gt, [det(1, 1, [10, 10, 50, 50], 0.9), det(1, 1, [300, 300, 50, 50], 0.8), det(1, 1, [100, 100, 50, 50], 0.7)])
    assert ev.stats[0] == pytest.approx((51 + 50 * 2 / 3) / 101, abs=1e-12)


def test_a_category_without_ground_truth_is_minus_one_and_left_out_of_the_mean(osr):
    gt = _one_image([dict(bbox=[10, 10, 50, 50])], cat_ids=(1, 2))
    ev = run_eval(osr, gt, [det(1, 1, [10, 10, 50, 50], 0.9), det(1, 2, [10, 10, 50, 50], 0.9)])
    assert (ev.eval["precision"][:, :, 1] == -1).all() and (ev.eval["recall"][:, 1] == -1).all()
    assert ev.stats[0] == pytest.approx(1.0, abs=1e-12)
    assert ev.stats[3] == -1 and ev.stats[5] == -1  # no small, no large ground truth at all


# ---- the matching rules, one case each -------------------------------------------------------------------------------------------------
def test_a_crowd_ground_truth_is_matched_twice(osr):
    gt = _one_image([dict(bbox=[0, 0, 100, 100], iscrowd=1)])
    ev = run_eval(osr, gt, [det(1, 1, [10, 10, 20, 20], 0.9), det(1, 1, [40, 40, 20, 20], 0.8)])  # inside the crowd: IoU = inter / det area = 1
    e = _img(ev)
    assert e["dt_matched"].all() and e["dt_ignore"].all() and (e["dt_gt"] == 0).all()


def test_a_sufficient_regular_ground_truth_beats_a_better_ignored_one(osr):
    gt = _one_image([dict(bbox=[0, 0, 100, 100], iscrowd=1), dict(bbox=[0, 0, 100, 80])])
    ev = run_eval(osr, gt, [det(1, 1, [0, 0, 100, 100], 0.9)])  # IoU 1 with the crowd, 0.8 with the regular one
    e = _img(ev)
    assert e["dt_gt"][:7, 0].tolist() == [1] * 7 and not e["dt_ignore"][:7].any()  # t <= 0.8: the regular one, the loop breaks before the crowd
    assert e["dt_gt"][7:, 0].tolist() == [0] * 3 and e["dt_ignore"][7:].all()      # above: only the crowd is left


def test_equal_ious_go_to_the_last_ground_truth(osr):
    gt = _one_image([dict(bbox=[10, 10, 40, 40]), dict(bbox=[10, 10, 40, 40]), dict(bbox=[10, 10, 40, 40])])
    ev = run_eval(osr, gt, [det(1, 1, [10, 10, 40, 40], 0.9), det(1, 1, [10, 10, 40, 40], 0.8)])
    e = _img(ev)
    assert (e["dt_gt"][:, 0] == 2).all() and (e["dt_gt"][:, 1] == 1).all()


def test_ious_of_exactly_a_half_and_three_quarters_still_match(osr):
    gt = _one_image([dict(bbox=[0, 0, 1, 1]), dict(bbox=[0, 0, 3, 1], category_id=2)], cat_ids=(1, 2))
    ev = run_eval(osr, gt, [det(1, 1, [0, 0, 2, 1], 0.9), det(1, 2, [0, 0, 4, 1], 0.9)])
    assert ev.ious[1, 1][0, 0] == 0.5 and ev.ious[1, 2][0, 0] == 0.75
    assert _img(ev, cat=1)["dt_matched"][:, 0].tolist() == [True] + [False] * 9
    assert _img(ev, cat=2)["dt_matched"][:, 0].tolist() == [True] * 6 + [False] * 4


def test_an_unmatched_detection_outside_the_area_range_is_ignored(osr):
    gt = _one_image([dict(bbox=[0, 0, 50, 50])])
    ev = run_eval(osr, gt, [det(1, 1, [300, 300, 10, 10], 0.9)])  # area 100: small
    assert not _img(ev, area=0)["dt_ignore"].any() and not _img(ev, area=1)["dt_ignore"].any()
    assert _img(ev, area=2)["dt_ignore"].all() and _img(ev, area=3)["dt_ignore"].all()
    assert not _img(ev, area=2)["dt_matched"].any()


def test_max_dets_truncates_at_1_10_and_100(osr):
    boxes = [[(i % 12) * 50, (i // 12) * 50, 40, 40] for i in range(120)]
    gt = _one_image([dict(bbox=b) for b in boxes])
    ev = run_eval(osr, gt, [det(1, 1, b, 1.0 - i / 200) for i, b in enumerate(boxes)])
    assert len(_img(ev)["dt_ids"]) == 100
    assert ev.stats[6:9] == pytest.approx([1 / 120, 10 / 120, 100 / 120], abs=1e-12)


def test_an_image_never_processed_still_counts_its_ground_truths(osr):
    gt = _one_image([dict(bbox=[10, 10, 50, 50]), dict(bbox=[10, 10, 50, 50], image_id=2)], image_ids=(1, 2))
    ev = run_eval(osr, gt, [det(1, 1, [10, 10, 50, 50], 0.9)])
    assert ev.stats[8] == pytest.approx(0.5, abs=1e-12)  # AR@100: one of two
    assert ev.stats[0] == pytest.approx(51 / 101, abs=1e-12)  # precision 1 up to recall 0.5, 0 beyond


# ---- against the existing open-set evaluator with every category known ---------------------------------------------------------------------
def test_bbox_ap_equals_the_openset_evaluator_with_every_category_known(osr):
    from openset_rcnn_amd.host.coco_evaluation import detection_records
    from openset_rcnn_amd.host.os_coco_evaluation import OpensetCOCOEval
    gt, image_ids, dets = seeded_dataset(5)
    cat_ids = sorted(c["id"] for c in gt["categories"])
    records = [r for img, d in zip(image_ids, dets) for r in detection_records(img, d["boxes"], d["scores"], d["classes"], None, dict(enumerate(cat_ids)))]
    ev = run_eval(osr, gt, records)
    other = OpensetCOCOEval(json.loads(json.dumps(gt)), records, cat_ids, max_dets=(1, 10, 100))
    other.evaluate()
    other.accumulate()
    st = other.summarize()
    assert (ev.stats[:6] > 0).all() and (ev.stats[:6] < 1).all()
    assert ev.stats[:6].tolist() == st[:6].tolist()                      # AP, AP50, AP75, APs, APm, APl
    assert ev.stats[[6, 7, 8]].tolist() == st[[6, 7, 8]].tolist()        # AR@1, AR@10, AR@100: its first three maxDets
    assert ev.stats[9:12].tolist() == st[11:14].tolist()                 # ARs, ARm, ARl


# ---- OKS ----------------------------------------------------------------------------------------------------------------------------------
def _kp_gt(points, bbox, area, **kw):
    return dict(bbox=bbox, area=area, keypoints=[float(v) for p in points for v in p], num_keypoints=sum(1 for p in points if p[2] > 0), **kw)


def test_one_visible_point_at_distance_d(osr):
    sig = [0.05, 0.1]
    gt = _one_image([_kp_gt([(30, 40, 2), (0, 0, 0)], [10, 10, 60, 60], 2500.0)])
    d = det(1, 1, [0, 0, 1, 1], 0.9, keypoints=[33.0, 44.0, 1.0, 90.0, 90.0, 1.0])  # 3-4-5: d = 5
    ev = run_eval(osr, gt, [d], "keypoints", kpt_oks_sigmas=sig)
    assert ev.ious[1, 1][0, 0] == pytest.approx(math.exp(-25.0 / (2 * 2500.0 * (2 * 0.05) ** 2)), rel=1e-14)
    assert ev.stats.shape == (10,)


def test_no_visible_point_compares_with_the_doubled_box(osr):
    sig = [0.05, 0.1]
    gt = _one_image([_kp_gt([(0, 0, 0), (0, 0, 0)], [100, 100, 20, 10], 200.0)])  # doubled: x in [80, 140], y in [90, 120]
    inside = det(1, 1, [0, 0, 1, 1], 0.9, keypoints=[80.0, 120.0, 1, 140.0, 90.0, 1])
    outside = det(1, 1, [0, 0, 1, 1], 0.8, keypoints=[77.0, 100.0, 1, 100.0, 124.0, 1])  # 3 left of it, 4 below it
    ev = run_eval(osr, gt, [inside, outside], "keypoints", kpt_oks_sigmas=sig)
    s = ev.ious[1, 1]
    assert s[0, 0] == 1.0
    expect = (math.exp(-9.0 / 0.01 / (200.0 + np.spacing(1)) / 2) + math.exp(-16.0 / 0.04 / (200.0 + np.spacing(1)) / 2)) / 2
    assert s[1, 0] == pytest.approx(expect, rel=1e-14)


def test_a_ground_truth_without_keypoints_is_ignored_and_the_detection_area_is_its_points_extent(osr):
    sig = [0.05, 0.1]
    gt = _one_image([_kp_gt([(0, 0, 0), (0, 0, 0)], [100, 100, 200, 200], 40000.0)])
    d = det(1, 1, [0, 0, 1, 1], 0.9, keypoints=[120.0, 130.0, 1, 160.0, 180.0, 1])  # extent 40 x 50 = 2000: medium, whatever its bbox says
    ev = run_eval(osr, gt, [d], "keypoints", kpt_oks_sigmas=sig)
    assert _img(ev)["gt_ignore"].tolist() == [1]
    assert _img(ev)["dt_matched"].all() and _img(ev)["dt_ignore"].all()
    assert ev.stats[0] == -1  # nothing but an ignored ground truth
    lone = run_eval(osr, _one_image([_kp_gt([(5, 5, 2), (9, 9, 2)], [0, 0, 10, 10], 5000.0)]), [d], "keypoints", kpt_oks_sigmas=sig)
    assert not _img(lone, area=1)["dt_ignore"].any() and _img(lone, area=2)["dt_ignore"].all()  # unmatched: medium by its own area, not large


# ---- the evaluator on CPU tensors -----------------------------------------------------------------------------------------------------------
def _cfg(*opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_list(list(opts))
    return cfg


@pytest.mark.parametrize("keypoints", [0, 17])
def test_results_file_round_trip_on_cpu_tensors(osr, tmp_path, keypoints):
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    gt, image_ids, dets = seeded_dataset(7, keypoints=keypoints)
    name = _register(osr, tmp_path, gt, f"rt{keypoints}")
    ev = COCOEvaluator(name, output_dir=str(tmp_path / "out"))
    for k in range(0, len(image_ids), 4):
        ev.process([dict(image_id=i) for i in image_ids[k:k + 4]], [dict(instances=_instances(osr, d)) for d in dets[k:k + 4]])
    res = ev.evaluate()
    assert list(res) == (["bbox", "keypoints"] if keypoints else ["bbox"])
    assert list(res["bbox"])[:6] == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and "AP-c7" in res["bbox"]
    assert all(0 < res["bbox"][k] < 100 for k in ("AP", "AP50", "APs", "APm", "APl"))
    if keypoints:
        assert list(res["keypoints"]) == ["AP", "AP50", "AP75", "APm", "APl"] and 0 < res["keypoints"]["AP50"] <= 100
    records = json.load(open(tmp_path / "out" / "coco_instances_results.json"))
    b = dets[0]["boxes"][0]
    assert records[0]["image_id"] == image_ids[0] and records[0]["category_id"] == 2 + 5 * int(dets[0]["classes"][0])
    assert records[0]["bbox"] == [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]
    if keypoints:
        assert records[0]["keypoints"][:3] == [float(dets[0]["keypoints"][0, 0, 0] - np.float32(0.5)), float(dets[0]["keypoints"][0, 0, 1] - np.float32(0.5)),
                                               float(dets[0]["keypoints"][0, 0, 2])]
    again = COCOEvaluator(name, tasks=tuple(res), output_dir=str(tmp_path / "out")).evaluate(resume=True)
    assert json.dumps(again) == json.dumps(res)  # (NaN-proof identity: the same keys, the same figures)


def test_segm_is_warned_about_once_and_refused_by_name(osr, tmp_path, caplog):
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    gt, image_ids, dets = seeded_dataset(7, n_images=2)
    name = _register(osr, tmp_path, gt, "segm")
    with caplog.at_level(logging.WARNING):
        ev = COCOEvaluator(name, _cfg("MODEL.MASK_ON", True))
    assert ev.tasks == ("bbox",) and sum("segm" in r.getMessage() for r in caplog.records) == 1
    ev.process([dict(image_id=image_ids[0])], [dict(instances=_instances(osr, dets[0]))])
    assert set(ev.evaluate()) == {"bbox"}
    with pytest.raises(NotImplementedError, match="segm"):
        COCOEvaluator(name, tasks=("segm",))
    assert COCOEvaluator(name, _cfg("MODEL.KEYPOINT_ON", True)).tasks == ("bbox", "keypoints")


def test_unknown_keypoint_count_without_sigmas_raises(osr, tmp_path):
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    gt, image_ids, dets = seeded_dataset(7, n_images=2, keypoints=5)
    name = _register(osr, tmp_path, gt, "sig")
    with pytest.raises(ValueError, match="TEST.KEYPOINT_OKS_SIGMAS"):
        COCOEvaluator(name).process([dict(image_id=image_ids[0])], [dict(instances=_instances(osr, dets[0]))])
    ev = COCOEvaluator(name, _cfg("MODEL.KEYPOINT_ON", True, "TEST.KEYPOINT_OKS_SIGMAS", [0.05] * 5))
    ev.process([dict(image_id=image_ids[0])], [dict(instances=_instances(osr, dets[0]))])
    assert set(ev.evaluate()) == {"bbox", "keypoints"}


def test_dispatch_coco_names_get_the_coco_evaluator_graspnet_keeps_its_own(osr, tmp_path, monkeypatch):
    from openset_rcnn_amd.host import datasets as D
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    from openset_rcnn_amd.host.os_coco_evaluation import OpensetCOCOEvaluator
    gt, _, _ = seeded_dataset(7, n_images=2)
    name = _register(osr, tmp_path, gt, "disp")
    meta = D.MetadataCatalog.get(name)
    assert meta.evaluator_type == "coco" and meta.closed_set is True
    ev = D.get_evaluator(_cfg("TEST.DETECTIONS_PER_IMAGE", 50), name, str(tmp_path / "o"))
    assert isinstance(ev, COCOEvaluator) and ev.max_dets["bbox"] == [1, 10, 50] and ev.tasks == ("bbox",)
    grasp = f"graspnet_{tmp_path.name}"
    D.register_graspnet_instances(grasp, meta.json_file, str(tmp_path))
    assert not getattr(D.MetadataCatalog.get(grasp), "closed_set", False)
    assert isinstance(D.get_evaluator(_cfg(), grasp, None), OpensetCOCOEvaluator)
    # the built-in names appear when their files do
    import run_net
    ann = tmp_path / "datasets" / "coco" / "annotations"
    os.makedirs(ann)
    for f in ("instances_val2017.json", "person_keypoints_val2017.json"):
        json.dump(gt, open(ann / f, "w"))
    monkeypatch.setenv("DETECTRON2_DATASETS", str(tmp_path / "datasets"))
    D2 = run_net.register_datasets(_cfg())
    assert "coco_2017_val" in D2.DatasetCatalog and "keypoints_coco_2017_val" in D2.DatasetCatalog and "coco_2017_train" not in D2.DatasetCatalog
    assert isinstance(D2.get_evaluator(_cfg(), "coco_2017_val", None), COCOEvaluator)


# ---- osr_coco_match refuses before it launches ---------------------------------------------------------------------------------------------
def test_coco_match_refusals_need_no_gpu(osr):
    lib = osr._lib.load()
    thr, rng = (ctypes.c_double * 17)(*([0.5] * 17)), (ctypes.c_double * 18)(*([0.0, 1e10] * 9))

    def call(cap=8, max_det=100, t=10, a=4, group=7, kp=0, task=0, n=1):
        return lib.osr_coco_match(task, None, None, None, None, None, n, cap, 3, kp, None, None, None, None, None, None, 10, group, thr, t, rng, a, max_det,
                                  None, None, None, None, None, 0, None)

    for kw, word in ((dict(cap=1025), b"cap 1025"), (dict(max_det=129), b"max_det 129"), (dict(t=17), b"17 thresholds"), (dict(a=9), b"9 area ranges"),
                     (dict(group=4097), b"4097 ground truths"), (dict(task=1, kp=33), b"33 keypoints")):
        assert call(**kw) == osr._lib.ERR_UNSUPPORTED, kw
        assert word in lib.osr_last_error(), (kw, lib.osr_last_error())
    assert call(task=2) == -1 and call() == -1 and b"null pointer" in lib.osr_last_error()
    assert call(n=0) == 0 and call(cap=0) == 0  # nothing to do: OK without a launch
    assert lib.osr_coco_match_workspace_bytes(160, 100, 77) == 100 * 77 * 8 and lib.osr_coco_match_workspace_bytes(20, 100, 5) == 20 * 5 * 8
    with pytest.raises(osr.OsrError):
        z = torch.zeros
        osr.ops.coco_match(z(1, 2, 4), z(1, 2), z(1, 2, dtype=torch.int64), z(1, dtype=torch.int32), 1, z(2, dtype=torch.int32), z(0, 4, dtype=torch.float64),
                           z(0, dtype=torch.float64), z(0, dtype=torch.uint8), 0, [0.5], [[0, 1e10]], 100)  # CPU tensors: refused, not computed on the host


# ---- run_net ---------------------------------------------------------------------------------------------------------------------------------
def test_run_net_logs_every_task_and_resume_test_rescores_the_file(osr, tmp_path, monkeypatch, caplog):
    """do_test on keypoints_coco_2017_val (found under detectron2's directory names) with --resume_test: the evaluator re-scores the
    detections a run left under OUTPUT_DIR, and the log carries one line for bbox and one for keypoints."""
    import types
    import run_net
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    gt, image_ids, dets = seeded_dataset(7, n_images=3, keypoints=17)
    ann = tmp_path / "datasets" / "coco" / "annotations"
    os.makedirs(ann)
    json.dump(gt, open(ann / "person_keypoints_val2017.json", "w"))
    monkeypatch.setenv("DETECTRON2_DATASETS", str(tmp_path / "datasets"))
    cfg = _cfg("MODEL.KEYPOINT_ON", True, "DATASETS.TEST", ("keypoints_coco_2017_val",), "OUTPUT_DIR", str(tmp_path / "out"))
    D = run_net.register_datasets(cfg)
    folder = os.path.join(cfg.OUTPUT_DIR, "inference", "keypoints_coco_2017_val", "Final")
    first = COCOEvaluator("keypoints_coco_2017_val", cfg, folder)
    first.process([dict(image_id=i) for i in image_ids], [dict(instances=_instances(osr, d)) for d in dets])
    expect = first.evaluate()
    with caplog.at_level(logging.INFO, logger="openset_rcnn"):
        res = run_net.do_test(cfg, types.SimpleNamespace(resume_test=True, test_batch=1), None, D)
    assert json.dumps(res) == json.dumps(expect) and list(res) == ["bbox", "keypoints"]
    lines = [r.getMessage().strip() for r in caplog.records]
    assert any(m.startswith("bbox:") and "AP50=" in m for m in lines) and any(m.startswith("keypoints:") and "APm=" in m for m in lines), lines
