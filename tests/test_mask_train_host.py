"""Training the mask branch, host side (no GPU): INPUT.MASK_FORMAT, BitMasks, the dataset mapper's bitmask path and the padding of
the ground-truth planes. "polygon" (the [d2] default) keeps the refusal that names the mask loss; "bitmask" builds a model whose
trainer is refused only by the missing GPU."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(*opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _rle(mask: np.ndarray) -> dict:
    """Uncompressed COCO RLE of a 2-D bitmap: column-major runs, zeros first."""
    flat = mask.T.reshape(-1).astype(np.uint8)
    change = np.flatnonzero(np.diff(flat)) + 1
    runs = np.diff(np.concatenate(([0], change, [flat.size]))).tolist()
    if flat[0] == 1:
        runs = [0] + runs
    return {"size": list(mask.shape), "counts": runs}


def test_mask_format_default_and_the_two_modes(osr):
    from openset_rcnn_amd.host import modeling as M
    assert _cfg().INPUT.MASK_FORMAT == "polygon"
    poly = M.build_model(_cfg("MODEL.MASK_ON", "True"))
    with pytest.raises(NotImplementedError, match="mask loss") as ei:
        poly.make_trainer()
    assert "bitmask" in str(ei.value) and "polygon" in str(ei.value)
    with pytest.raises(NotImplementedError, match="mask loss"):
        poly.losses_forward([])
    bit = M.build_model(_cfg("MODEL.MASK_ON", "True", "INPUT.MASK_FORMAT", "bitmask"))
    assert bit.roi_heads.mask_format == "bitmask" and bit._mask_training() is True and poly._mask_training() is False
    assert M.build_model(_cfg())._mask_training() is None
    with pytest.raises(osr.OsrError):  # the refusal is gone: the trainer now stops at the device check (no GPU here)
        bit.make_trainer()
    with pytest.raises(ValueError, match="MASK_FORMAT"):
        M.build_model(_cfg("MODEL.MASK_ON", "True", "INPUT.MASK_FORMAT", "rle"))


def test_bitmask_batch_without_gt_masks_says_so(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.structures import Boxes, Instances
    bit = M.build_model(_cfg("MODEL.MASK_ON", "True", "INPUT.MASK_FORMAT", "bitmask"))
    gt = Instances((64, 64), gt_boxes=Boxes(torch.tensor([[4.0, 4.0, 40.0, 40.0]])), gt_classes=torch.tensor([1]))
    with pytest.raises(ValueError, match="gt_masks"):
        bit._train_tensors([{"image": torch.zeros(3, 64, 64), "instances": gt}])


def test_bitmasks_through_instances(osr):
    from openset_rcnn_amd.host.structures import BitMasks, Boxes, Instances
    m = torch.zeros(3, 8, 10, dtype=torch.uint8)
    m[0, 1:3, 2:5] = 1
    m[2, 4:, :] = 1
    bm = BitMasks(m)
    assert len(bm) == 3 and bm.tensor.dtype == torch.bool and bm.image_size == (8, 10)
    assert bm.nonempty().tolist() == [True, False, True]
    assert len(bm[1]) == 1 and tuple(bm[1].tensor.shape) == (1, 8, 10)
    inst = Instances((8, 10), gt_boxes=Boxes(torch.tensor([[2.0, 1, 5, 3], [0, 0, 0, 0], [0, 4, 10, 8]])), gt_classes=torch.tensor([0, 1, 2]),
                     gt_masks=bm)
    kept = inst[torch.tensor([True, False, True])]
    assert len(kept) == 2 and isinstance(kept.gt_masks, BitMasks) and torch.equal(kept.gt_masks.tensor, bm.tensor[[0, 2]])
    both = Instances.cat([kept, inst[1:2]])
    assert len(both) == 3 and torch.equal(both.gt_masks.tensor, bm.tensor[[0, 2, 1]])
    assert both.to("cpu").gt_masks.tensor.dtype == torch.bool
    assert len(BitMasks(torch.zeros(0, 8, 10))) == 0


def _write_image(tmp_path, h, w):
    from PIL import Image
    rng = np.random.RandomState(0)
    path = os.path.join(str(tmp_path), "img.png")
    Image.fromarray(rng.randint(0, 255, (h, w, 3), dtype=np.uint8)).save(path)
    return path


def _record(tmp_path, h=40, w=60):
    yy, xx = np.mgrid[0:h, 0:w]
    rect = np.zeros((h, w), dtype=np.uint8)
    rect[5:25, 10:40] = 1
    disc = ((yy - 20) ** 2 + (xx - 45) ** 2 <= 81)
    annos = [dict(bbox=[10.0, 5.0, 40.0, 25.0], category_id=1, segmentation=rect),
             dict(bbox=[36.0, 11.0, 55.0, 30.0], category_id=0, segmentation=_rle(disc)),
             dict(bbox=[7.0, 7.0, 7.0, 20.0], category_id=2, segmentation=np.zeros((h, w), dtype=bool)),  # empty box: dropped by `keep`
             dict(bbox=[0.0, 0.0, 9.0, 9.0], category_id=0, iscrowd=1, segmentation=rect)]               # crowd: dropped
    return dict(file_name=_write_image(tmp_path, h, w), image_id=3, annotations=annos), rect.astype(bool), disc


def test_mapper_maps_arrays_and_rle_flips_resizes_and_filters(osr, tmp_path):
    from PIL import Image
    from openset_rcnn_amd.host.data import DatasetMapper, decode_segmentation
    rec, rect, disc = _record(tmp_path)
    assert np.array_equal(decode_segmentation(_rle(disc), 40, 60), disc) and np.array_equal(decode_segmentation(_rle(rect), 40, 60), rect)
    ones = np.ones((3, 4), dtype=bool)
    assert np.array_equal(decode_segmentation(_rle(ones), 3, 4), ones)
    cfg = _cfg("MODEL.MASK_ON", "True", "INPUT.MASK_FORMAT", "bitmask")
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN = (80,), 400
    mapper = DatasetMapper(cfg, is_train=True, seed=0)
    seen = set()
    for seed in range(8):
        out = mapper(rec, sample_seed=seed)
        inst = out["instances"]
        nh, nw = inst.image_size
        assert (nh, nw) == (80, 120) and len(inst) == 2 and inst.gt_classes.tolist() == [1, 0]
        masks = inst.gt_masks.tensor.numpy()
        assert masks.shape == (2, 80, 120) and masks.dtype == np.bool_
        # the rectangle's box x range [10, 40] of 60 lands at [20, 80] of 120 or, flipped, at [40, 100]
        flipped = abs(float(inst.gt_boxes.tensor[0, 0]) - 40.0) < 1e-4
        seen.add(flipped)
        for got, src in zip(masks, (rect, disc)):
            src = src[:, ::-1] if flipped else src
            want = np.asarray(Image.fromarray(np.ascontiguousarray(src).astype(np.uint8)).resize((120, 80), Image.NEAREST)).astype(bool)
            assert np.array_equal(got, want)
        # a mask stays inside its (flipped, resized) box
        ys, xs = np.nonzero(masks[0])
        b = inst.gt_boxes.tensor[0].tolist()
        assert b[0] - 1 <= xs.min() and xs.max() <= b[2] + 1 and b[1] - 1 <= ys.min() and ys.max() <= b[3] + 1
    assert seen == {True, False}, "eight samples must show both the flipped and the unflipped image"
    # masks are mapped only when the model trains them
    assert not DatasetMapper(_cfg("MODEL.MASK_ON", "True"), is_train=True)(rec)["instances"].has("gt_masks")
    assert not DatasetMapper(_cfg("INPUT.MASK_FORMAT", "bitmask"), is_train=True)(rec)["instances"].has("gt_masks")


def test_mapper_refuses_polygons_and_compressed_rle(osr, tmp_path):
    from openset_rcnn_amd.host.data import DatasetMapper
    rec, _, _ = _record(tmp_path)
    cfg = _cfg("MODEL.MASK_ON", "True", "INPUT.MASK_FORMAT", "bitmask")
    mapper = DatasetMapper(cfg, is_train=True)
    poly = dict(rec, annotations=[dict(bbox=[1.0, 1, 20, 20], category_id=0, segmentation=[[1.0, 1.0, 20.0, 1.0, 20.0, 20.0]])])
    with pytest.raises(ValueError, match="INPUT.MASK_FORMAT"):
        mapper(poly)
    crle = dict(rec, annotations=[dict(bbox=[1.0, 1, 20, 20], category_id=0, segmentation={"size": [40, 60], "counts": "abc"})])
    with pytest.raises(ValueError, match="INPUT.MASK_FORMAT"):
        mapper(crle)
    with pytest.raises(ValueError, match="segmentation"):
        mapper(dict(rec, annotations=[dict(bbox=[1.0, 1, 20, 20], category_id=0)]))


def test_train_tensors_pad_the_masks_of_a_ragged_batch(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.structures import BitMasks, Boxes, Instances
    g = torch.Generator().manual_seed(0)

    def sample(h, w, k):
        masks = torch.rand(k, h, w, generator=g) < 0.3
        boxes = torch.tensor([[1.0, 1.0, 10.0, 12.0]] * k).reshape(k, 4)
        return {"image": torch.zeros(3, h, w, dtype=torch.uint8),
                "instances": Instances((h, w), gt_boxes=Boxes(boxes), gt_classes=torch.arange(k), gt_masks=BitMasks(masks))}
    batch = [sample(40, 64, 2), sample(48, 56, 0), sample(32, 32, 3)]
    gt, gcls, gcnt, planes = M.pad_ground_truth([b["instances"] for b in batch], (48, 64))
    assert tuple(planes.shape) == (3, 3, 48, 64) and planes.dtype == torch.uint8 and gcnt.tolist() == [2, 0, 3]
    for i, b in enumerate(batch):
        m = b["instances"].gt_masks.tensor
        k, h, w = m.shape if len(m) else (0, 0, 0)
        if k:
            assert torch.equal(planes[i, :k, :h, :w].bool(), m)
        rest = planes[i].clone()
        rest[:k, :h, :w] = 0
        assert int(rest.max()) == 0, "everything outside an image's own masks is zero"
    assert len(M.pad_ground_truth([b["instances"] for b in batch])) == 3, "without masks_hw the three tensors as before"
    bit = M.build_model(_cfg("MODEL.MASK_ON", "True", "INPUT.MASK_FORMAT", "bitmask"))
    tensors = bit._train_tensors(batch, torch.Generator().manual_seed(1))
    assert len(tensors) == 9 and torch.equal(tensors[8], planes) and tuple(tensors[0].shape[-2:]) == (48, 64)
    assert bit._mask_kwargs(tensors).keys() == {"gt_masks"}
    off = M.build_model(_cfg())
    assert len(off._train_tensors(batch, torch.Generator().manual_seed(1))) == 8 and off._mask_kwargs(tensors[:8]) == {}


def test_deconv_pack_round_trip(osr):
    from openset_rcnn_amd.host.weights import pack_deconv_weight, unpack_deconv_weight
    w = torch.randn(128, 64, 2, 2)
    for dt, e in ((torch.float32, 0), (torch.float32, 8), (torch.float16, 0)):
        p = pack_deconv_weight(w, dt, frag_elems=e)
        assert torch.equal(unpack_deconv_weight(p), w.to(dt))
    assert torch.equal(pack_deconv_weight(w, torch.float32, frag_elems=8).half(), pack_deconv_weight(w, torch.float16))
