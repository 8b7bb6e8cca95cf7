"""CascadeROIHeads without a GPU: MODEL.ROI_BOX_CASCADE_HEAD's defaults, configs/cascade_rcnn_fpn.yaml and detectron2's own cascade
yaml keys, the model mirror's modules and parameter names, the refusals detectron2 asserts (each a ValueError naming its key), the
mask variant and the TEST.AUG refusal."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# detectron2's configs/Misc/cascade_mask_rcnn_R_50_FPN_1x.yaml, the keys it sets on top of Base-RCNN-FPN.yaml (restated, with the
# base file replaced by this repository's)
D2_CASCADE_YAML = """
_BASE_: "{base}"
MODEL:
  MASK_ON: True
  RESNETS:
    DEPTH: 50
  ROI_HEADS:
    NAME: CascadeROIHeads
  ROI_BOX_HEAD:
    CLS_AGNOSTIC_BBOX_REG: True
  RPN:
    POST_NMS_TOPK_TRAIN: 2000
"""


def _cfg(osr, *opts, yaml="cascade_rcnn_fpn.yaml"):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    cfg.merge_from_file(yaml if os.path.isabs(yaml) else os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _d2_names(stages, mask=False):
    names = []
    for s in range(stages):
        names += [f"roi_heads.box_head.{s}.{fc}.{p}" for fc in ("fc1", "fc2") for p in ("weight", "bias")]
        names += [f"roi_heads.box_predictor.{s}.{l}.{p}" for l in ("cls_score", "bbox_pred") for p in ("weight", "bias")]
    if mask:
        names += [f"roi_heads.mask_head.{l}.{p}" for l in ("mask_fcn1", "mask_fcn2", "mask_fcn3", "mask_fcn4", "deconv", "predictor")
                  for p in ("weight", "bias")]
    return sorted(names)


def test_defaults(osr):
    from openset_rcnn_amd.host.config import get_cfg
    ch = get_cfg().MODEL.ROI_BOX_CASCADE_HEAD
    assert tuple(tuple(w) for w in ch.BBOX_REG_WEIGHTS) == ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))
    assert tuple(ch.IOUS) == (0.5, 0.6, 0.7)
    from openset_rcnn_amd.host import ops
    assert ops.CASCADE_MAX_STAGES == 4


def test_the_shipped_yaml(osr):
    cfg = _cfg(osr)
    assert cfg.MODEL.ROI_HEADS.NAME == "CascadeROIHeads" and cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG is True
    assert cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN == 2000 and cfg.MODEL.MASK_ON is False
    # the rest is base_rcnn_fpn.yaml's
    assert cfg.MODEL.ROI_BOX_HEAD.NUM_FC == 2 and cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION == 7 and cfg.MODEL.RPN.POST_NMS_TOPK_TEST == 1000


def test_detectron2_cascade_yaml_keys_load(osr, tmp_path):
    path = tmp_path / "cascade_mask_rcnn_R_50_FPN_1x.yaml"
    path.write_text(D2_CASCADE_YAML.format(base=os.path.join(ROOT, "configs", "base_rcnn_fpn.yaml")))
    cfg = _cfg(osr, "MODEL.ROI_BOX_CASCADE_HEAD.IOUS", "(0.5, 0.6)", "MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS", "((10, 10, 5, 5), (20, 20, 10, 10))",
               yaml=str(path))
    assert cfg.MODEL.MASK_ON is True and cfg.MODEL.ROI_HEADS.NAME == "CascadeROIHeads"
    assert tuple(cfg.MODEL.ROI_BOX_CASCADE_HEAD.IOUS) == (0.5, 0.6) and len(cfg.MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS) == 2


def test_build_model_gives_the_cascade_with_detectron2_names(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.engine_cascade import CascadeRCNNEngine
    assert "CascadeROIHeads" in M.ROI_HEADS_REGISTRY
    model = M.build_model(_cfg(osr))
    rh = model.roi_heads
    assert type(rh) is M.CascadeROIHeads and isinstance(rh, M.StandardROIHeads)
    assert isinstance(rh.box_head, torch.nn.ModuleList) and isinstance(rh.box_predictor, torch.nn.ModuleList)
    assert len(rh.box_head) == 3 and len(rh.box_predictor) == 3 and rh.num_cascade_stages == 3
    sd = model.state_dict()
    assert sorted(k for k in sd if k.startswith("roi_heads.")) == _d2_names(3)
    for s in range(3):
        assert sd[f"roi_heads.box_head.{s}.fc1.weight"].shape == (1024, 256 * 49)
        assert sd[f"roi_heads.box_predictor.{s}.cls_score.weight"].shape == (81, 1024)
        assert sd[f"roi_heads.box_predictor.{s}.bbox_pred.weight"].shape == (4, 1024)
    assert model._engine_cls is CascadeRCNNEngine and rh._engine_cls is CascadeRCNNEngine
    assert not hasattr(rh, "mask_head")


def test_state_dict_round_trips(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.weights import random_cascade_params
    cfg = _cfg(osr)
    a, b = M.build_model(cfg), M.build_model(cfg)
    sd = a.state_dict()
    params = random_cascade_params(0, stages=3)
    heads = [k for k in params if k.startswith("roi_heads.")]
    assert sorted(heads) == _d2_names(3)
    for k in heads:
        assert sd[k].shape == params[k].shape, k
        sd[k] = params[k]
    b.load_state_dict(sd)
    got = b.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    # the stages are separate parameters
    assert not torch.equal(got["roi_heads.box_head.0.fc1.weight"], got["roi_heads.box_head.1.fc1.weight"])


@pytest.mark.parametrize("opts, key", [
    (("MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", "False"), "CLS_AGNOSTIC_BBOX_REG"),
    (("MODEL.ROI_BOX_CASCADE_HEAD.IOUS", "(0.5, 0.6)"), "ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS"),
    (("MODEL.ROI_BOX_CASCADE_HEAD.IOUS", "(0.6, 0.6, 0.7)"), "ROI_HEADS.IOU_THRESHOLDS"),
    (("MODEL.ROI_BOX_CASCADE_HEAD.IOUS", "()", "MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS", "()"), "ROI_BOX_CASCADE_HEAD.IOUS"),
    (("MODEL.ROI_BOX_CASCADE_HEAD.IOUS", "(0.5, 0.55, 0.6, 0.65, 0.7)",
      "MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS", repr(((10, 10, 5, 5),) * 5)), "ROI_BOX_CASCADE_HEAD.IOUS"),
    (("MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS", "((10, 10, 5, 5), (20, 20, 10), (30, 30, 15, 15))"), "ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS"),
    (("MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS", "((10, 10, 5, 5), (20, 20, 10, 0), (30, 30, 15, 15))"), "ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS"),
    (("MODEL.KEYPOINT_ON", "True"), "KEYPOINT_ON"),
], ids=["class-specific", "lengths", "first-iou", "no-stage", "five-stages", "three-weights", "zero-weight", "keypoints"])
def test_refusals_name_their_key(osr, opts, key):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match=key):
        M.build_model(_cfg(osr, *opts))


@pytest.mark.parametrize("stages", [1, 2, 4])
def test_one_to_four_stages_build(osr, stages):
    from openset_rcnn_amd.host import modeling as M
    ious = (0.5, 0.6, 0.7, 0.75)[:stages]
    model = M.build_model(_cfg(osr, "MODEL.ROI_BOX_CASCADE_HEAD.IOUS", repr(ious), "MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS",
                               repr(((10.0, 10.0, 5.0, 5.0),) * stages)))
    assert len(model.roi_heads.box_head) == stages
    assert sorted(k for k in model.state_dict() if k.startswith("roi_heads.")) == _d2_names(stages)


def test_mask_on_builds_the_mask_head_and_polygon_training_stays_refused(osr):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(_cfg(osr, "MODEL.MASK_ON", "True"))
    assert isinstance(model.roi_heads.mask_head, M.MaskRCNNConvUpsampleHead) and model.roi_heads.mask_on
    assert sorted(k for k in model.state_dict() if k.startswith("roi_heads.")) == _d2_names(3, mask=True)
    with pytest.raises(NotImplementedError, match="bitmask"):  # (INPUT.MASK_FORMAT "polygon": as for StandardROIHeads)
        model.make_trainer()


def test_tta_refuses_the_cascade_by_name(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    cfg = _cfg(osr, "TEST.AUG.ENABLED", "True")
    with pytest.raises(ValueError, match="CascadeROIHeads"):
        GeneralizedRCNNWithTTA(cfg, M.build_model(cfg).eval())


def test_engine_options_check(osr):
    from openset_rcnn_amd.host.engine_cascade import check_cascade_options
    assert check_cascade_options((0.5, 0.6, 0.7), ((10, 10, 5, 5),) * 3, first_iou=0.5) == 3
    assert check_cascade_options((0.5,), ((10.0, 10.0, 5.0, 5.0),)) == 1
    with pytest.raises(ValueError, match="BBOX_REG_WEIGHTS"):
        check_cascade_options((0.5,), ((10, 10, 5, True),))
