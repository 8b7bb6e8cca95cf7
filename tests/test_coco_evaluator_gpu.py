"""COCOEvaluator end to end on the device: a temporary 6-image COCO JSON with seeded device Instances, with and without keypoints.
The device path (osr_coco_match per batch, one copy, accumulation from the flags) must return a dict equal to the same evaluator on
CPU copies (the numpy COCOeval), and `resume=True` on the file it wrote must equal both."""
import json
import math

import pytest
import torch

from tests.coco_eval_common import instances as _instances, register as _register, seeded_dataset

DEV = "cuda:0"


@pytest.mark.gpu
@pytest.mark.parametrize("keypoints", [0, 17])
def test_device_instances_score_like_cpu_copies_and_like_the_results_file(osr, tmp_path, keypoints):
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    gt, image_ids, dets = seeded_dataset(7, keypoints=keypoints)
    dets[2] = {k: v[:9] for k, v in dets[2].items()}  # batches of different caps
    dets[4] = {k: v[:0] for k, v in dets[4].items()}  # an image without a detection
    name = _register(osr, tmp_path, gt, f"gpu{keypoints}")
    results = {}
    for device in (DEV, "cpu"):
        ev = COCOEvaluator(name, output_dir=str(tmp_path / device.replace(":", "_")))
        for lo, hi in ((0, 2), (2, 5)):  # the sixth image is never processed: its ground truths still count
            ev.process([dict(image_id=i) for i in image_ids[lo:hi]], [dict(instances=_instances(osr, d, device)) for d in dets[lo:hi]])
        if device == DEV:
            assert len(ev._chunks) == 2 and all(t.is_cuda for c in ev._chunks for t in c.values() if isinstance(t, torch.Tensor)) and not ev._cpu_records
        results[device] = ev.evaluate()
    dev, cpu = results[DEV], results["cpu"]
    assert list(dev) == (["bbox", "keypoints"] if keypoints else ["bbox"])
    assert not any(math.isnan(v) for figures in cpu.values() for v in figures.values())  # (so that == compares every figure)
    assert 0 < cpu["bbox"]["AP"] < 100 and len(cpu["bbox"]) == 9
    assert dev == cpu
    assert json.load(open(tmp_path / "cuda_0" / "coco_instances_results.json")) == json.load(open(tmp_path / "cpu" / "coco_instances_results.json"))
    resumed = COCOEvaluator(name, tasks=tuple(dev), output_dir=str(tmp_path / "cuda_0")).evaluate(resume=True)
    assert resumed == dev and resumed == cpu
    narrowed = COCOEvaluator(name, output_dir=None)
    narrowed.process([dict(image_id=i) for i in image_ids[:3]], [dict(instances=_instances(osr, d, DEV)) for d in dets[:3]])
    cpu3 = COCOEvaluator(name, output_dir=None)
    cpu3.process([dict(image_id=i) for i in image_ids[:3]], [dict(instances=_instances(osr, d, "cpu")) for d in dets[:3]])
    assert json.dumps(narrowed.evaluate(img_ids=image_ids[:2])) == json.dumps(cpu3.evaluate(img_ids=image_ids[:2]))
