"""COCOEvaluator and OpensetCOCOEvaluator on outputs that carry "proposals": proposals alone and beside "instances", box_proposals
first and equal to the specification, the pickle; on the device 12 images in batches of 5 give exactly the CPU path's eight numbers."""
import json
import pickle

import numpy as np
import pytest
import torch

from tests.coco_eval_common import instances as _instances, register as _register, seeded_dataset
from tests.proposal_common import coco_gt, proposals as _proposals, seeded_image

DEV = "cuda:0"
NAMES = ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]


def _dataset(seed, n_images=12):
    """-> (COCO JSON with some crowd annotations, image ids, per image (boxes, logits)): 130 proposals on most images, so that the
    limit of 100 matters; one image without proposals, one without ground truth."""
    rng = np.random.default_rng(seed)
    image_ids = [5 + 2 * i for i in range(n_images)]
    props, gts = [], []
    for i in range(n_images):
        b, s, g, ar = seeded_image(rng, 0 if i == 3 else (130 if i % 2 == 0 else 20 + i), 0 if i == 7 else 3 + i)
        props.append((b, s))
        gts.append((g, ar, (rng.random(len(g)) < 0.2).astype(int)))
    return coco_gt(image_ids, gts), image_ids, props


def _specification(gt, image_ids, props):
    from openset_rcnn_amd.host import proposal_evaluation as PE
    from openset_rcnn_amd.host.coco_evaluation import _GroundTruthTables
    tb = _GroundTruthTables(gt)
    recs = [dict(image_id=i, boxes=b, objectness_logits=s) for i, (b, s) in zip(image_ids, props)]
    out = {}
    for limit in (100, 1000):
        for area, suffix in (("all", ""), ("small", "s"), ("medium", "m"), ("large", "l")):
            out[f"AR{suffix}@{limit}"] = float(PE.evaluate_box_proposals(recs, tb, area=area, limit=limit)["ar"].item() * 100)
    return out


def _run(ev, image_ids, props, device, batch=5, extra=None):
    for lo in range(0, len(image_ids), batch):
        outs = [dict(proposals=_proposals(b, s, device)) for b, s in props[lo:lo + batch]]
        if extra is not None:
            for o, d in zip(outs, extra[lo:lo + batch]):
                o["instances"] = d
        ev.process([dict(image_id=i) for i in image_ids[lo:lo + batch]], outs)
    return ev.evaluate()


def test_coco_evaluator_scores_proposals_alone(osr, tmp_path):
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    gt, image_ids, props = _dataset(21)
    want = _specification(gt, image_ids, props)
    assert list(want) == NAMES and 0 < want["AR@100"] < want["AR@1000"] < 100
    name = _register(osr, tmp_path, gt, "prop")
    res = _run(COCOEvaluator(name, output_dir=str(tmp_path / "out")), image_ids, props, "cpu")
    assert list(res) == ["box_proposals"] and list(res["box_proposals"]) == NAMES
    assert res["box_proposals"] == want
    assert not (tmp_path / "out" / "coco_instances_results.json").exists()
    with open(tmp_path / "out" / "box_proposals.pkl", "rb") as f:
        saved = pickle.load(f)
    assert sorted(saved) == ["bbox_mode", "boxes", "ids", "objectness_logits"] and saved["bbox_mode"] == 0 and saved["ids"] == image_ids
    for (b, s), sb, ss in zip(props, saved["boxes"], saved["objectness_logits"]):
        assert isinstance(sb, np.ndarray) and sb.dtype == np.float32 and np.array_equal(sb, b) and np.array_equal(ss, s)
    # reset() forgets them; an evaluator that saw nothing reports as before
    ev = COCOEvaluator(name)
    _run(ev, image_ids[:5], props[:5], "cpu")
    ev.reset()
    assert list(ev.evaluate()) == ["bbox"]


def test_coco_evaluator_scores_both_keys_and_puts_proposals_first(osr, tmp_path):
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    gt, image_ids, dets = seeded_dataset(7)
    rng = np.random.default_rng(3)
    props = [seeded_image(rng, 30, 4)[:2] for _ in image_ids]
    name = _register(osr, tmp_path, gt, "both")
    plain = COCOEvaluator(name)
    plain.process([dict(image_id=i) for i in image_ids], [dict(instances=_instances(osr, d)) for d in dets])
    plain = plain.evaluate()
    res = _run(COCOEvaluator(name, output_dir=str(tmp_path / "out")), image_ids, props, "cpu", batch=4, extra=[_instances(osr, d) for d in dets])
    assert list(res) == ["box_proposals", "bbox"] and res["bbox"] == plain["bbox"]
    assert res["box_proposals"] == _specification(gt, image_ids, props)
    assert (tmp_path / "out" / "coco_instances_results.json").exists() and (tmp_path / "out" / "box_proposals.pkl").exists()


def test_openset_evaluator_scores_proposals(osr, tmp_path):
    from openset_rcnn_amd.host.os_coco_evaluation import OpensetCOCOEvaluator
    gt, image_ids, dets = seeded_dataset(9)
    rng = np.random.default_rng(4)
    props = [seeded_image(rng, 25, 5)[:2] for _ in image_ids]
    known = [c["name"] for c in gt["categories"][:2]]
    id_map = {k: c["id"] for k, c in enumerate(gt["categories"])}
    want = _specification(gt, image_ids, props)
    res = _run(OpensetCOCOEvaluator(gt, known, id_map, output_dir=str(tmp_path / "p")), image_ids, props, "cpu")
    assert list(res) == ["box_proposals"] and res["box_proposals"] == want
    with open(tmp_path / "p" / "box_proposals.pkl", "rb") as f:
        assert pickle.load(f)["ids"] == image_ids
    plain = OpensetCOCOEvaluator(gt, known, id_map)
    plain.process([dict(image_id=i) for i in image_ids], [dict(instances=_instances(osr, d)) for d in dets])
    plain = plain.evaluate()
    both = _run(OpensetCOCOEvaluator(gt, known, id_map), image_ids, props, "cpu", extra=[_instances(osr, d) for d in dets])
    assert list(both)[0] == "box_proposals" and both["box_proposals"] == want
    assert json.dumps({k: v for k, v in both.items() if k != "box_proposals"}) == json.dumps(plain)


def test_limits_are_named(osr, tmp_path):
    from openset_rcnn_amd.host import proposal_evaluation as PE
    from openset_rcnn_amd.host.coco_evaluation import _GroundTruthTables
    from openset_rcnn_amd.host.structures import Boxes, Instances

    rng = np.random.default_rng(1)
    gt = coco_gt([1], [seeded_image(rng, 1, 1025)[2:]])
    pr = PE.ProposalRecall(_GroundTruthTables(gt))
    with pytest.raises(ValueError, match="at most 2048"):
        pr._process_device([1], [Instances((480, 640), proposal_boxes=Boxes(torch.zeros(2049, 4)), objectness_logits=torch.zeros(2049))], False)
    with pytest.raises(ValueError, match="at most 1024"):
        pr._process_device([1], [Instances((480, 640), proposal_boxes=Boxes(torch.zeros(8, 4)), objectness_logits=torch.zeros(8))], False)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["coco", "openset"])
def test_device_batches_give_exactly_the_cpu_paths_numbers(osr, tmp_path, which):
    from openset_rcnn_amd.host.coco_evaluation import COCOEvaluator
    from openset_rcnn_amd.host.os_coco_evaluation import OpensetCOCOEvaluator
    gt, image_ids, props = _dataset(21)
    name = _register(osr, tmp_path, gt, "dev")

    def make(sub):
        out = str(tmp_path / sub)
        return COCOEvaluator(name, output_dir=out) if which == "coco" else OpensetCOCOEvaluator(gt, ["thing"], {0: 1}, output_dir=out)
    ev = make("dev")
    dev = _run(ev, image_ids, props, DEV)  # 12 images in batches of 5: the last one has 2
    assert not ev.proposals._cpu_records and ev.proposals._dev_sums[0].is_cuda and tuple(ev.proposals._dev_sums[0].shape) == (4, 2, 10)
    cpu = _run(make("cpu"), image_ids, props, "cpu")
    assert list(dev) == ["box_proposals"] and list(dev["box_proposals"]) == NAMES
    assert dev == cpu and dev["box_proposals"] == _specification(gt, image_ids, props)
    a, b = (pickle.load(open(tmp_path / sub / "box_proposals.pkl", "rb")) for sub in ("dev", "cpu"))
    assert a["ids"] == b["ids"] and all(np.array_equal(x, y) for k in ("boxes", "objectness_logits") for x, y in zip(a[k], b[k]))
    # device and CPU batches in one evaluator: the sums add
    mixed = make("mixed")
    for lo, device in ((0, DEV), (5, "cpu"), (10, DEV)):
        mixed.process([dict(image_id=i) for i in image_ids[lo:lo + 5]], [dict(proposals=_proposals(b_, s_, device)) for b_, s_ in props[lo:lo + 5]])
    assert mixed.evaluate() == cpu
