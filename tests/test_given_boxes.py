"""GeneralizedRCNN.inference(detected_instances=...) / StandardROIHeads.forward_with_given_boxes: the mask branch on boxes the
caller supplies. Feeding a pass's own detections back returns the same boxes, scores and classes and pred_masks bit-equal to that
pass's (the given lists are padded to the engine's capacity, so they go through the very launches that made the masks); a model
without a mask head returns the instances unchanged. Model: tests/tta_common.py (the recipe of tests/test_mask_rcnn_e2e.py), images
96 x 128 and 80 x 112."""
import pytest
import torch

from tests import tta_common as T

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]


def _inputs():
    return [T.inputs()[0], T.inputs()[2]]  # 96 x 128 (pasted at 120 x 160) and 80 x 112: a ragged batch


def _given(outs):
    from openset_rcnn_amd.host.structures import Boxes, Instances
    return [Instances(o["instances"].image_size, pred_boxes=Boxes(o["instances"].pred_boxes.tensor.clone()), scores=o["instances"].scores.clone(),
                      pred_classes=o["instances"].pred_classes.clone()) for o in outs]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("agnostic", [True, False], ids=["agnostic", "per-class"])
def test_own_detections_fed_back(osr, dtype, agnostic):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    _, model = T.build(True, agnostic, dtype)
    first = model.inference(_inputs(), do_postprocess=False)
    counts = [len(o["instances"]) for o in first]
    assert all(c >= 1 for c in counts), f"precondition: detections in every image, got {counts}"
    again = model.inference(_inputs(), detected_instances=_given(first), do_postprocess=False)
    for a, b in zip(first, again):
        a, b = a["instances"], b["instances"]
        assert b.image_size == a.image_size
        assert torch.equal(b.pred_boxes.tensor, a.pred_boxes.tensor) and torch.equal(b.scores, a.scores) and torch.equal(b.pred_classes, a.pred_classes)
        assert b.pred_masks.shape == (len(a), 1, 28, 28) and b.pred_masks.dtype == torch.float32
        assert torch.equal(b.pred_masks, a.pred_masks)
        assert float(a.pred_masks.max()) > 0.0
    # with the postprocess: the same Instances as the plain call's
    plain = model.inference(_inputs())
    post = model.inference(_inputs(), detected_instances=_given(first))
    for a, b in zip(plain, post):
        a, b = a["instances"], b["instances"]
        assert b.image_size == a.image_size and torch.equal(b.pred_boxes.tensor, a.pred_boxes.tensor) and torch.equal(b.pred_masks, a.pred_masks)
    # StandardROIHeads.forward_with_given_boxes on the NCHW pyramid
    eng = model.engine()
    batch, sizes = model._stack_images([x["image"] for x in _inputs()])
    pyr = eng._backbone(batch, 96, 128)
    feats = {k: pyr[k].permute(0, 3, 1, 2) for k in ("p2", "p3", "p4", "p5")}
    for a, b in zip(first, model.roi_heads.forward_with_given_boxes(feats, _given(first))):
        assert torch.equal(b.pred_masks, a["instances"].pred_masks) and torch.equal(b.scores, a["instances"].scores)
    # a subset in another order: each row's mask follows its box
    sub = _given(first)
    sub[0] = sub[0][torch.arange(len(sub[0]) - 1, -1, -1)]
    rev = model.inference(_inputs(), detected_instances=sub, do_postprocess=False)[0]["instances"]
    assert torch.equal(rev.pred_masks, first[0]["instances"].pred_masks.flip(0))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
def test_without_a_mask_head_the_instances_come_back_unchanged(osr, dtype):
    _, model = T.build(False, False, dtype)
    first = model.inference(_inputs(), do_postprocess=False)
    assert sum(len(o["instances"]) for o in first) >= 1
    given = _given(first)
    again = model.inference(_inputs(), detected_instances=given, do_postprocess=False)
    for g, b in zip(given, again):
        b = b["instances"]
        assert not b.has("pred_masks") and set(b.get_fields()) == {"pred_boxes", "scores", "pred_classes"}
        assert torch.equal(b.pred_boxes.tensor, g.pred_boxes.tensor) and torch.equal(b.scores, g.scores) and torch.equal(b.pred_classes, g.pred_classes)
    pyr = model.engine()._backbone(*_stacked(model))
    feats = {k: pyr[k].permute(0, 3, 1, 2) for k in ("p2", "p3", "p4", "p5")}
    assert model.roi_heads.forward_with_given_boxes(feats, given) is given
    with pytest.raises(ValueError, match="Instances for"):
        model.inference(_inputs(), detected_instances=given[:1])


def _stacked(model):
    batch, _ = model._stack_images([x["image"] for x in _inputs()])
    return batch, 96, 128
