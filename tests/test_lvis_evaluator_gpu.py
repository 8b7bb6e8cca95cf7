"""LVISEvaluator end to end on a 6-image temporary dataset, one image never processed. The device path (osr_lvis_match per batch, one
copy, accumulation from the flags) must return a dict equal to the same evaluator on CPU copies of the predictions (the numpy
LVISEval), write the same results file, and `resume=True` on that file must return it again."""
import json

import pytest

from tests.lvis_eval_common import instances, register, seeded_lvis

DEV = "cuda:0"


@pytest.mark.gpu
def test_device_cpu_and_resume_return_equal_dicts_and_files(osr, tmp_path):
    from openset_rcnn_amd.host.lvis_evaluation import LVISEvaluator
    gt, image_ids, dets = seeded_lvis(3, n_images=6)
    dets[1] = {k: v[:0] for k, v in dets[1].items()}  # an image without a detection
    name = register(tmp_path, gt, "e2e")
    results = {}
    for where, device in (("dev", DEV), ("cpu", "cpu")):
        ev = LVISEvaluator(name, output_dir=str(tmp_path / where), max_dets_per_image=30)  # 40 detections per image: the cut is felt
        for lo, hi in ((0, 2), (2, 5)):  # two batches; image 5 is never processed
            ev.process([dict(image_id=i) for i in image_ids[lo:hi]], [dict(instances=instances(d, device)) for d in dets[lo:hi]])
        results[where] = ev.evaluate()
        if where == "dev":
            assert ev._chunks and not ev._cpu_records and ev._chunks[0]["flags"].is_cuda  # it did go through the kernel
    res = results["dev"]
    assert list(res) == ["bbox"] and list(res["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"]
    assert 0 < res["bbox"]["AP"] < 100 and all(v == v for v in res["bbox"].values())  # the set says something: no NaN, not all or nothing
    assert json.dumps(results["dev"]) == json.dumps(results["cpu"])
    files = [json.load(open(tmp_path / w / "lvis_instances_results.json")) for w in ("dev", "cpu")]
    assert files[0] == files[1] and len(files[0]) == 4 * 40
    again = LVISEvaluator(name, output_dir=str(tmp_path / "dev"), max_dets_per_image=30).evaluate(resume=True)
    assert json.dumps(again) == json.dumps(res)
    part = LVISEvaluator(name, output_dir=str(tmp_path / "dev"), max_dets_per_image=30)
    part.process([dict(image_id=i) for i in image_ids[:5]], [dict(instances=instances(d, DEV)) for d in dets[:5]])
    narrowed = part.evaluate(img_ids=image_ids[:3])  # narrowed to three images: the device and numpy paths still agree
    assert json.dumps(narrowed) == json.dumps(part.evaluate(img_ids=image_ids[:3], resume=True)) and json.dumps(narrowed) != json.dumps(res)
