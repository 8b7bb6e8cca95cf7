"""The numpy LVISEval (host/lvis_evaluation.py), one hand-computed case per federated rule, an independent cross-check against the numpy
COCOeval under conditions where the two must agree, the LVIS loader / registration / dispatch, and osr_lvis_match's refusals, which
need no GPU."""
import ctypes
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests.lvis_eval_common import det, instances, lvis_json, register, run_lvis, seeded_lvis

CATS = [(1, "f"), (2, "c"), (3, "r")]
BOX = [10, 10, 40, 40]  # area 1600: medium


def _img(ev, img=1, cat=1, area=0):
    return ev.eval_imgs[img, cat, area]


# ---- one rule each ---------------------------------------------------------------------------------------------------------------------------
def test_the_image_cut_precedes_the_category_filter(osr):
    """max_dets 3: the two best detections are of category 2, which image 1 does not evaluate. They fill the cut and vanish; of
    category 1 only the third-best of the image is left. Filtering first would have listed both detections of category 1."""
    gt = lvis_json([1], CATS, [dict(image_id=1, category_id=1, bbox=BOX)])
    dets = [det(1, 2, BOX, .9), det(1, 2, BOX, .8), det(1, 1, BOX, .7), det(1, 1, BOX, .6)]
    ev = run_lvis(gt, dets, max_dets=3)
    assert _img(ev)["dt_ids"] == [3] and (1, 2, 0) not in ev.eval_imgs
    assert _img(run_lvis(gt, dets, max_dets=4))["dt_ids"] == [3, 4]


def test_a_tie_at_the_cut_keeps_the_earlier_row(osr):
    gt = lvis_json([1], CATS, [dict(image_id=1, category_id=1, bbox=BOX)])
    ev = run_lvis(gt, [det(1, 1, [200, 200, 40, 40], .5), det(1, 1, BOX, .9), det(1, 1, BOX, .5)], max_dets=2)
    assert _img(ev)["dt_ids"] == [2, 1]  # the matching box of the same score came later and is cut
    assert _img(ev)["dt_matched"][0].tolist() == [True, False]


def test_an_unevaluated_category_vanishes_and_a_negative_one_is_a_false_positive(osr):
    """Category 2 is neither positive nor negative in image 1: its detection does not exist. Category 3 is negative there: the same
    box is a false positive, which halves the precision category 3 reaches through its true positive in image 2."""
    gt = lvis_json([1, 2], CATS, [dict(image_id=1, category_id=1, bbox=BOX), dict(image_id=2, category_id=2, bbox=BOX), dict(image_id=2, category_id=3, bbox=BOX)],
                   neg={1: [3]})
    ev = run_lvis(gt, [det(1, 2, BOX, .9), det(1, 3, BOX, .9), det(2, 2, BOX, .5), det(2, 3, BOX, .5)])
    assert (1, 2, 0) not in ev.eval_imgs
    e = _img(ev, 1, 3)
    assert e["dt_ids"] == [2] and not e["dt_matched"].any() and not e["dt_ignore"][:, 0].any()
    pr = ev.eval["precision"]
    assert (pr[:, :, 1, 0] == pr[0, 0, 1, 0]).all() and pr[0, 0, 1, 0] > 0.999  # category 2: its lone detection is the true positive
    assert np.allclose(pr[:, :, 2, 0], 0.5)  # category 3: the false positive outranks the true positive


def test_not_exhaustive_ignores_the_unmatched_and_keeps_the_matched(osr):
    gt = lvis_json([1], CATS, [dict(image_id=1, category_id=1, bbox=BOX)], nex={1: [1]})
    e = _img(run_lvis(gt, [det(1, 1, BOX, .9), det(1, 1, [200, 200, 40, 40], .8)]))
    assert e["dt_matched"][:, 0].all() and not e["dt_ignore"][:, 0].any()  # a true positive
    assert not e["dt_matched"][:, 1].any() and e["dt_ignore"][:, 1].all()  # ignored, not a false positive
    e = _img(run_lvis(lvis_json([1], CATS, [dict(image_id=1, category_id=1, bbox=BOX)]), [det(1, 1, BOX, .9), det(1, 1, [200, 200, 40, 40], .8)]))
    assert not e["dt_ignore"].any()  # exhaustive: the second one is a false positive


def test_two_detections_on_one_ground_truth_give_one_tp_and_one_fp(osr):
    gt = lvis_json([1], CATS, [dict(image_id=1, category_id=1, bbox=BOX)])
    e = _img(run_lvis(gt, [det(1, 1, BOX, .6), det(1, 1, BOX, .9)]))
    assert e["dt_ids"] == [2, 1] and e["dt_matched"][:, 0].all() and not e["dt_matched"][:, 1].any() and not e["dt_ignore"].any()


def test_ignored_and_out_of_range_ground_truths_are_consulted_last(osr):
    """The detection equals the `ignore` ground truth (IoU 1) and overlaps the regular one with IoU 2/3 (32 of 48 columns). Up to 0.65
    the regular one wins although its IoU is lower; above, only the ignored one is left and the match is ignored. In the small range
    both are ignored (area 2000), the better one is taken, and the match is ignored at every threshold."""
    gt = lvis_json([1], CATS, [dict(image_id=1, category_id=1, bbox=[0, 0, 40, 50], ignore=1), dict(image_id=1, category_id=1, bbox=[8, 0, 40, 50])])
    e = _img(run_lvis(gt, [det(1, 1, [0, 0, 40, 50], .9)]))
    assert e["dt_matched"][:, 0].all()
    assert e["dt_gt"][:, 0].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0] and e["dt_ignore"][:, 0].tolist() == [False] * 4 + [True] * 6
    small = _img(run_lvis(gt, [det(1, 1, [0, 0, 40, 50], .9)]), area=1)
    assert small["dt_gt"][:, 0].tolist() == [0] * 10 and small["dt_ignore"][:, 0].all()


def test_equal_ious_go_to_the_later_ground_truth(osr):
    gt = lvis_json([1], CATS, [dict(image_id=1, category_id=1, bbox=BOX), dict(image_id=1, category_id=1, bbox=BOX)])
    e = _img(run_lvis(gt, [det(1, 1, BOX, .9), det(1, 1, BOX, .8)]))
    assert e["dt_gt"][:, 0].tolist() == [1] * 10 and e["dt_gt"][:, 1].tolist() == [0] * 10  # no re-use: the second takes what is left


def test_iou_exactly_at_a_threshold_matches(osr):
    gt = lvis_json([1], CATS, [dict(image_id=1, category_id=1, bbox=[0, 0, 1, 1]), dict(image_id=1, category_id=2, bbox=[0, 0, 3, 1])])
    ev = run_lvis(gt, [det(1, 1, [0, 0, 2, 1], .9), det(1, 2, [0, 0, 4, 1], .9)])
    assert _img(ev, 1, 1)["dt_matched"][:, 0].tolist() == [True] + [False] * 9  # IoU 0.5
    assert _img(ev, 1, 2)["dt_matched"][:, 0].tolist() == [True] * 6 + [False] * 4  # IoU 0.75


def test_one_ap_by_hand_and_a_frequency_group_without_a_category_is_nan(osr):
    """Category 1 (frequent): two ground truths in two images; detections 0.9 (TP), 0.8 (FP: a box off the ground truth) and 0.7 (TP).
    Recall 0.5, 0.5, 1; precision 1, 1/2, 2/3, envelope 1, 2/3, 2/3: the 51 recall thresholds up to 0.5 read
    1, the other 50 read 2/3. Every box pair has IoU 1, so all ten thresholds agree. There is no rare category: APr is NaN; category
    2 (common) has no ground truth: APc is NaN as well."""
    gt = lvis_json([1, 2], CATS[:2], [dict(image_id=1, category_id=1, bbox=BOX), dict(image_id=2, category_id=1, bbox=BOX)])
    res = run_lvis(gt, [det(1, 1, BOX, .9), det(1, 1, [200, 200, 40, 40], .8), det(2, 1, BOX, .7)]).results()
    want = (51 * 1.0 + 50 * 2.0 / 3.0) / 101 * 100
    assert list(res) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"]
    for k in ("AP", "AP50", "AP75", "APm", "APf"):
        assert res[k] == pytest.approx(want, abs=1e-9), k
    assert all(np.isnan(res[k]) for k in ("APs", "APl", "APr", "APc"))


# ---- against the numpy COCOeval ----------------------------------------------------------------------------------------------------------
def test_neutral_conditions_equal_the_numpy_cocoeval(osr):
    """No crowd, no ignore, nothing not exhaustive, every absent category negative, 40 detections per image (under COCO's 100 per
    category and LVIS's 300 per image): the federated rules change nothing and the six shared figures must be the same doubles."""
    from openset_rcnn_amd.host.coco_evaluation import COCOeval, derive_coco_results, detection_records
    gt, image_ids, dets = seeded_lvis(5, neutral=True)
    rev = {k: c["id"] for k, c in enumerate(gt["categories"])}
    records = [r for img, d in zip(image_ids, dets) for r in detection_records(img, d["boxes"], d["scores"], d["classes"], None, rev)]
    ours = run_lvis(gt, records).results()
    coco = COCOeval(gt, records, "bbox", max_dets=[1, 10, 100])
    coco.evaluate()
    coco.accumulate()
    theirs = derive_coco_results(coco.summarize(), coco.eval["precision"], "bbox", None)
    assert 5 < ours["AP"] < 95 and ours["APs"] > 0 and ours["APl"] > 0  # the set says something
    for k in ("AP", "AP50", "AP75", "APs", "APm", "APl"):
        assert ours[k] == theirs[k], k


# ---- loader, registration, dispatch ------------------------------------------------------------------------------------------------------
def _cfg(*opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_list(list(opts))
    return cfg


def test_loader_registration_and_dispatch(osr, tmp_path, monkeypatch, caplog):
    from openset_rcnn_amd.host import datasets as D
    from openset_rcnn_amd.host.lvis_evaluation import LVISEvaluator
    gt = lvis_json([7, 3], [(20, "f"), (5, "r")], [dict(image_id=3, category_id=20, bbox=[1, 2, 3, 4], segmentation=[[1, 2, 4, 2, 4, 6]]),
                                                  dict(image_id=3, category_id=5, bbox=[5, 6, 7, 8])], neg={7: [5]}, nex={3: [20]})
    gt["images"][0]["file_name"] = "own/name.jpg"
    name = register(tmp_path, gt, "load")
    dicts = D.DatasetCatalog[name]()
    meta = D.MetadataCatalog.get(name)
    assert meta.evaluator_type == "lvis" and meta.lvis_json is True and meta.thing_classes == ["c5", "c20"]
    assert meta.thing_dataset_id_to_contiguous_id == {5: 0, 20: 1}
    assert [d["image_id"] for d in dicts] == [3, 7]
    assert dicts[0]["file_name"] == os.path.join(str(tmp_path), "val2017", "000000000003.jpg") and dicts[1]["file_name"] == os.path.join(str(tmp_path), "own/name.jpg")
    assert dicts[0]["not_exhaustive_category_ids"] == [20] and dicts[1]["neg_category_ids"] == [5] and dicts[0]["neg_category_ids"] == []
    assert dicts[0]["annotations"] == [dict(bbox=[1, 2, 3, 4], bbox_mode="XYWH_ABS", category_id=1, segmentation=[[1, 2, 4, 2, 4, 6]]),
                                       dict(bbox=[5, 6, 7, 8], bbox_mode="XYWH_ABS", category_id=0)]
    ev = D.get_evaluator(_cfg("TEST.DETECTIONS_PER_IMAGE", 50), name, str(tmp_path / "o"))
    assert isinstance(ev, LVISEvaluator) and ev.max_dets == 300 and ev.tasks == ("bbox",)
    # a name that merely says "lvis" keeps the refusal
    D.MetadataCatalog.get(f"odd_{tmp_path.name}").evaluator_type = "lvis"
    with pytest.raises(NotImplementedError, match="no Evaluator for the dataset"):
        D.get_evaluator(_cfg(), f"odd_{tmp_path.name}")
    # segm: one warning from a config, a refusal by name; proposals only: a refusal
    with caplog.at_level(logging.WARNING):
        masked = LVISEvaluator(name, _cfg("MODEL.MASK_ON", True))
    assert masked.tasks == ("bbox",) and sum("segm" in r.getMessage() for r in caplog.records) == 1
    with pytest.raises(NotImplementedError, match="segm"):
        LVISEvaluator(name, tasks=("segm",))
    with pytest.raises(NotImplementedError, match="proposal"):
        ev.process([dict(image_id=3)], [dict(proposals=None)])
    # the built-in names appear when their files do
    import run_net
    os.makedirs(tmp_path / "datasets" / "lvis")
    json.dump(gt, open(tmp_path / "datasets" / "lvis" / "lvis_v1_val.json", "w"))
    monkeypatch.setenv("DETECTRON2_DATASETS", str(tmp_path / "datasets"))
    D2 = run_net.register_datasets(_cfg())
    assert "lvis_v1_val" in D2.DatasetCatalog and "lvis_v1_train" not in D2.DatasetCatalog and "lvis_v0.5_val" not in D2.DatasetCatalog
    assert isinstance(D2.get_evaluator(_cfg(), "lvis_v1_val", None), LVISEvaluator)
    assert D2.DatasetCatalog["lvis_v1_val"]()[0]["file_name"] == os.path.join(str(tmp_path / "datasets"), "coco", "val2017", "000000000003.jpg")


def test_the_evaluator_on_cpu_tensors_writes_the_file_and_resumes_from_it(osr, tmp_path):
    from openset_rcnn_amd.host.coco_evaluation import detection_records
    from openset_rcnn_amd.host.lvis_evaluation import LVISEvaluator
    gt, image_ids, dets = seeded_lvis(9)
    name = register(tmp_path, gt, "cpu")
    ev = LVISEvaluator(name, output_dir=str(tmp_path / "out"), max_dets_per_image=30)
    ev.process([dict(image_id=i) for i in image_ids[:-1]], [dict(instances=instances(d)) for d in dets[:-1]])  # (one image is never processed)
    res = ev.evaluate()
    rev = {k: c["id"] for k, c in enumerate(gt["categories"])}
    records = [r for img, d in zip(image_ids[:-1], dets[:-1]) for r in detection_records(img, d["boxes"], d["scores"], d["classes"], None, rev)]
    assert json.dumps(res) == json.dumps({"bbox": run_lvis(gt, records, max_dets=30).results()}) and 0 < res["bbox"]["AP"] < 100
    assert json.load(open(tmp_path / "out" / "lvis_instances_results.json")) == records  # every detection, dataset ids, cut or not
    assert json.dumps(LVISEvaluator(name, output_dir=str(tmp_path / "out"), max_dets_per_image=30).evaluate(resume=True)) == json.dumps(res)
    assert json.dumps(res) != json.dumps({"bbox": run_lvis(gt, records).results()})  # the cut at 30 of 40 is felt
    with pytest.raises(ValueError, match="1024"):  # the device path's limit is told on the host
        big = dict(boxes=np.zeros((1025, 4), dtype=np.float32), scores=np.zeros(1025, dtype=np.float32), classes=np.zeros(1025, dtype=np.int64))
        ev._process_device([image_ids[0]], [instances(big)])


# ---- osr_lvis_match refuses before it launches ---------------------------------------------------------------------------------------------
def test_lvis_match_refusals_need_no_gpu(osr):
    lib = osr._lib.load()
    L = osr._lib
    thr, rng = (ctypes.c_double * 17)(*([0.5] * 17)), (ctypes.c_double * 18)(*([0.0, 1e10] * 9))
    one = ctypes.c_void_p(8)  # a non-null, aligned address that is never read: every case below is refused before a launch

    def call(n=1, cap=8, K=1203, ne=4, ng=10, group=5, t=10, a=4, max_dets=300, ptr=None, thrs=thr, rngs=rng, ws=None, ws_bytes=1 << 30):
        return lib.osr_lvis_match(ptr, ptr, ptr, ptr, n, cap, K, ptr, ptr, ptr, ptr, ne, ptr, ptr, ptr, ng, group, thrs, t, rngs, a, max_dets, ptr, ptr, None, None,
                                  ws, ws_bytes, None)

    beyond = dict(cap=L.LVIS_MAX_CAP + 1, max_dets=L.LVIS_MAX_DET + 1, t=L.LVIS_MAX_THRS + 1, a=L.LVIS_MAX_AREAS + 1, group=L.LVIS_MAX_GROUP + 1)
    assert L.LVIS_MAX_DET >= 300
    for k, v in beyond.items():
        assert call(**{k: v}) == -2 and b"osr_lvis_match" in lib.osr_last_error(), k  # OSR_ERR_UNSUPPORTED
    for bad in (dict(n=-1), dict(cap=-1), dict(K=0), dict(ne=-1), dict(ng=-1), dict(group=-1), dict(t=0), dict(a=0), dict(max_dets=0), dict(thrs=None), dict(rngs=None)):
        assert call(**bad) == -1 and b"osr_lvis_match" in lib.osr_last_error(), bad
    # at the limits nothing is unsupported: the call gets as far as its pointers, each of which is refused when null
    at = dict(cap=L.LVIS_MAX_CAP, max_dets=L.LVIS_MAX_DET, t=L.LVIS_MAX_THRS, a=L.LVIS_MAX_AREAS, group=L.LVIS_MAX_GROUP, K=1 << 20)
    assert call(**at) == -1 and b"osr_lvis_match: null pointer" in lib.osr_last_error()
    assert call(ptr=one, ws=None) == -1 and b"null pointer" in lib.osr_last_error()  # the workspace is always needed
    need = lib.osr_lvis_match_workspace_bytes(1, 8, 300, 10)
    assert need == 8 * 10 * 8 + (1 + 4 * 8 + 1) * 4 and lib.osr_lvis_match_workspace_bytes(2, 400, 300, 7) == 300 * 7 * 8 + (2 + 4 * 600) * 4
    assert lib.osr_lvis_match_workspace_bytes(-1, 8, 300, 0) == -1
    assert call(ptr=one, ws=one, ws_bytes=need - 1) == -4 and b"workspace" in lib.osr_last_error()  # OSR_ERR_WORKSPACE
    assert call(ptr=one, ws=ctypes.c_void_p(12), ws_bytes=need) == -1 and b"misaligned" in lib.osr_last_error()
    assert call(n=0, ptr=None) == 0 and call(cap=0, ptr=None) == 0  # nothing to do is no error
    with pytest.raises(osr.ops.OsrError, match="must live on the GPU"):
        z = torch.zeros
        osr.ops.lvis_match(z(1, 2, 4), z(1, 2), z(1, 2, dtype=torch.int64), z(1, dtype=torch.int32), 3, z(2, dtype=torch.int32), z(0, dtype=torch.int32),
                           z(1, dtype=torch.int32), z(0, dtype=torch.uint8), z(0, 4, dtype=torch.float64), z(0, dtype=torch.float64), z(0, dtype=torch.uint8),
                           0, [0.5], [[0, 1e10]], 300)  # CPU tensors: refused, not computed on the host
