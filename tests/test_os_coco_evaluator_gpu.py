"""OpensetCOCOEvaluator end to end on the device: a seeded 6-image open-set JSON with device Instances in two batches of different
caps, one image never processed. The device path (osr_os_coco_match per batch, one copy, accumulation from the flags) must return
what the same evaluator returns for CPU copies (the numpy OpensetCOCOEval), write the same files, and agree with `resume=True`."""
import copy
import json

import pytest
import torch

from tests.os_coco_common import instances, names_of, seeded_openset

DEV = "cuda:0"
FILES = ("coco_instances_results.json", "known_precision_bbox.npy", "known_recall_bbox.npy", "unknown_precision_bbox.npy", "unknown_recall_bbox.npy")


def _data():
    gt, image_ids, known_ids, reverse_map, dets = seeded_openset(7)
    dets[0], dets[1] = {k: v[:12] for k, v in dets[0].items()}, {k: v[:14] for k, v in dets[1].items()}  # batches of different caps: 14 and 18
    dets[2] = {k: v[:9] for k, v in dets[2].items()}
    dets[4] = {k: v[:0] for k, v in dets[4].items()}  # an image without a detection
    return gt, image_ids, names_of(gt, known_ids), reverse_map, dets


def _run(osr, gt, names, reverse_map, image_ids, dets, devices, output_dir=None, batches=((0, 2), (2, 5)), **kw):
    from openset_rcnn_amd.host.os_coco_evaluation import OpensetCOCOEvaluator
    ev = OpensetCOCOEvaluator(gt, names, reverse_map, output_dir=output_dir)
    for (lo, hi), device in zip(batches, devices):
        ev.process([dict(image_id=i) for i in image_ids[lo:hi]], [dict(instances=instances(osr, d, device)) for d in dets[lo:hi]])
    return ev, (lambda: ev.evaluate(**kw))


@pytest.mark.gpu
def test_device_instances_score_like_cpu_copies_and_write_the_same_files(osr, tmp_path):
    from openset_rcnn_amd.host.os_coco_evaluation import OpensetCOCOEvaluator
    gt, image_ids, names, reverse_map, dets = _data()
    results = {}
    for device in (DEV, "cpu"):
        ev, evaluate = _run(osr, gt, names, reverse_map, image_ids, dets, (device, device), str(tmp_path / device.replace(":", "_")))
        if device == DEV:  # the chunks are device tensors and no per-detection record was built
            assert len(ev._chunks) == 2 and ev._chunks[0]["cap"] != ev._chunks[1]["cap"] and not ev._predictions
            assert all(t.is_cuda for c in ev._chunks for t in c.values() if isinstance(t, torch.Tensor))
            assert all(isinstance(c[k], torch.Tensor) for c in ev._chunks for k in ("boxes", "scores", "classes", "counts", "flags", "rank"))
        results[device] = evaluate()
    dev, cpu = results[DEV], results["cpu"]
    assert list(cpu) == ["bbox", "bbox_unknown"] and len(cpu["bbox"]) + len(cpu["bbox_unknown"]) == 30
    assert 0 < cpu["bbox"]["AP"] < 100 and 0 < cpu["bbox_unknown"]["AP"] < 100 and cpu["bbox"]["AOSE"] > 0 and cpu["bbox"]["WI"] > 0
    assert json.dumps(dev) == json.dumps(cpu)
    for name in FILES:
        assert (tmp_path / "cuda_0" / name).read_bytes() == (tmp_path / "cpu" / name).read_bytes(), name
    resumed = OpensetCOCOEvaluator(gt, names, reverse_map, output_dir=str(tmp_path / "cuda_0")).evaluate(resume=True)
    assert json.dumps(resumed) == json.dumps(dev) and json.dumps(resumed) == json.dumps(cpu)


@pytest.mark.gpu
def test_narrowed_images_mixed_input_and_a_zero_id(osr, caplog):
    gt, image_ids, names, reverse_map, dets = _data()
    narrow = [image_ids[0], image_ids[2], image_ids[5]]
    _, on_device = _run(osr, gt, names, reverse_map, image_ids, dets, (DEV, DEV), img_ids=narrow)
    _, on_cpu = _run(osr, gt, names, reverse_map, image_ids, dets, ("cpu", "cpu"), img_ids=narrow)
    cpu_narrow = on_cpu()
    assert json.dumps(on_device()) == json.dumps(cpu_narrow)
    _, all_cpu = _run(osr, gt, names, reverse_map, image_ids, dets, ("cpu", "cpu"))
    cpu = all_cpu()
    assert json.dumps(cpu) != json.dumps(cpu_narrow)
    mixed_ev, mixed = _run(osr, gt, names, reverse_map, image_ids, dets, ("cpu", DEV))
    with caplog.at_level("WARNING"):
        assert json.dumps(mixed()) == json.dumps(cpu)
    assert len(mixed_ev._chunks) == 1 and sum("numpy OpensetCOCOEval" in r.getMessage() for r in caplog.records) == 1
    zero = copy.deepcopy(gt)
    zero["annotations"][3]["id"] = 0  # the numpy class reads this ground truth's matches as "unmatched": the host path is the only one that agrees
    zero_ev, zero_dev = _run(osr, zero, names, reverse_map, image_ids, dets, (DEV, DEV))
    _, zero_cpu = _run(osr, zero, names, reverse_map, image_ids, dets, ("cpu", "cpu"))
    assert not zero_ev._chunks and json.dumps(zero_dev()) == json.dumps(zero_cpu())
    assert sum("take the host path" in r.getMessage() for r in caplog.records) == 1  # two batches, one line
