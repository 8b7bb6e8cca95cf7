"""The dataset path of mask training (no GPU): a COCO-format json whose annotations carry uncompressed RLE goes through
datasets.load_coco_json -- what run_net.py's registered datasets are read with -- and DatasetMapper to the gt_masks the trainer pads;
a json without `segmentation` loads as before and is refused by the mapper by name. Also the self-check of the float64 RoIAlign
reference the GPU tests of osr_mask_targets use, against the oracle's fp32 loop."""
import json
import os

import numpy as np
import pytest

from oracle import osr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(*opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _rle(mask: np.ndarray) -> dict:
    flat = mask.T.reshape(-1).astype(np.uint8)
    change = np.flatnonzero(np.diff(flat)) + 1
    runs = np.diff(np.concatenate(([0], change, [flat.size]))).tolist()
    return {"size": list(mask.shape), "counts": ([0] if flat[0] else []) + runs}


def _toy_coco(tmp_path, with_masks=True):
    from PIL import Image
    h, w = 36, 48
    rng = np.random.RandomState(1)
    os.makedirs(os.path.join(str(tmp_path), "images"), exist_ok=True)
    masks = {}
    images, annos = [], []
    for i in range(2):
        Image.fromarray(rng.randint(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(str(tmp_path), "images", f"{i}.png"))
        images.append(dict(id=10 + i, file_name=f"{i}.png", height=h, width=w))
        for j, (x, y, bw, bh) in enumerate(((4, 5, 20, 12), (22, 14, 18, 16))):
            m = np.zeros((h, w), dtype=bool)
            m[y + 1:y + bh - 1, x + 2:x + bw - j] = True
            masks[(10 + i, j)] = m
            a = dict(id=len(annos), image_id=10 + i, category_id=(7, 3)[j], bbox=[x, y, bw, bh], iscrowd=0)
            if with_masks:
                a["segmentation"] = _rle(m)
            annos.append(a)
    path = os.path.join(str(tmp_path), "toy.json")
    with open(path, "w") as fh:
        json.dump(dict(images=images, annotations=annos, categories=[dict(id=3, name="a"), dict(id=7, name="b")]), fh)
    return path, os.path.join(str(tmp_path), "images"), masks


def test_coco_json_with_rle_reaches_gt_masks(osr, tmp_path):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.data import DatasetMapper
    from openset_rcnn_amd.host.datasets import load_coco_json
    path, root, masks = _toy_coco(tmp_path)
    dicts = load_coco_json(path, root)
    assert len(dicts) == 2 and all("segmentation" in a for d in dicts for a in d["annotations"])
    assert dicts[0]["annotations"][0]["bbox"] == [4, 5, 24, 17] and dicts[0]["annotations"][0]["category_id"] == 1
    cfg = _cfg("MODEL.MASK_ON", "True", "INPUT.MASK_FORMAT", "bitmask", "INPUT.RANDOM_FLIP", "none")
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = (36,), 400
    mapper = DatasetMapper(cfg, is_train=True)
    batch = [mapper(d) for d in dicts]
    for d, out in zip(dicts, batch):
        inst = out["instances"]
        assert len(inst) == 2 and inst.gt_classes.tolist() == [1, 0]
        for j in range(2):
            assert np.array_equal(inst.gt_masks.tensor[j].numpy(), masks[(d["image_id"], j)])
    # ... and the planes the trainer is handed
    model = M.build_model(cfg)
    tensors = model._train_tensors(batch)
    assert len(tensors) == 9 and tuple(tensors[8].shape) == (2, 2, 36, 48)
    assert np.array_equal(tensors[8][1, 1].numpy().astype(bool), masks[(11, 1)])


def test_coco_json_without_segmentation_loads_as_before_and_the_mapper_says_what_is_missing(osr, tmp_path):
    from openset_rcnn_amd.host.data import DatasetMapper
    from openset_rcnn_amd.host.datasets import load_coco_json
    path, root, _ = _toy_coco(tmp_path, with_masks=False)
    dicts = load_coco_json(path, root)
    assert all(set(a) == {"bbox", "bbox_mode", "category_id", "iscrowd"} for d in dicts for a in d["annotations"])
    assert len(DatasetMapper(_cfg(), is_train=True)(dicts[0])["instances"]) == 2
    with pytest.raises(ValueError, match="segmentation"):
        DatasetMapper(_cfg("MODEL.MASK_ON", "True", "INPUT.MASK_FORMAT", "bitmask"), is_train=True)(dicts[0])


def test_float64_roi_align_reference_agrees_with_the_oracle():
    """tests/test_mask_train_kernels.py's float64 loop is the oracle's fp32 roi_align_ref up to fp32 rounding, on the rows that exist."""
    from tests.test_mask_train_kernels import M as SIDE, _targets_case
    planes, boxes, gt_idx, _, ref = _targets_case()
    for r in range(3):
        rois = np.concatenate(([0.0], boxes[r])).astype(np.float32)[None]
        o = O.roi_align_ref(planes[0, gt_idx[r]].astype(np.float32)[None, None], rois, 1.0, SIDE, 0, True)[0, 0]
        assert np.abs(o - ref[r]).max() < 1e-5, f"row {r}"
