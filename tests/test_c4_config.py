"""Faster R-CNN R50-C4 on the host side, without a GPU: configs/faster_rcnn_R_50_C4.yaml and detectron2's own Base-RCNN-C4.yaml keys,
the two registered names, the model mirror's parameter names and shapes (detectron2's, so faster_rcnn_R_50_C4 checkpoints load), the
checkpoint round trips, every refusal by its key, the training refusals, and that the FPN model is built as before."""
import os
import pickle

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# detectron2's configs/Base-RCNN-C4.yaml and configs/COCO-Detection/faster_rcnn_R_50_C4_1x.yaml (restated): everything else of the
# model is detectron2's defaults, which host/config.py carries
D2_BASE_C4_YAML = """
MODEL:
  META_ARCHITECTURE: "GeneralizedRCNN"
  RPN:
    PRE_NMS_TOPK_TEST: 6000
    POST_NMS_TOPK_TEST: 1000
  ROI_HEADS:
    NAME: "Res5ROIHeads"
DATASETS:
  TRAIN: ("coco_2017_train",)
  TEST: ("coco_2017_val",)
SOLVER:
  IMS_PER_BATCH: 16
  BASE_LR: 0.02
  STEPS: (60000, 80000)
  MAX_ITER: 90000
INPUT:
  MIN_SIZE_TRAIN: (640, 672, 704, 736, 768, 800)
VERSION: 2
"""
D2_R50_C4_1X_YAML = """
_BASE_: "Base-RCNN-C4.yaml"
MODEL:
  WEIGHTS: "detectron2://ImageNetPretrained/MSRA/R-50.pkl"
  MASK_ON: False
  RESNETS:
    DEPTH: 50
"""
BN = ("weight", "bias", "running_mean", "running_var")


def _cfg(*opts, yaml="faster_rcnn_R_50_C4.yaml"):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    if yaml:
        cfg.merge_from_file(yaml if os.path.isabs(yaml) else os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _conv_bn(pre):
    return [pre + ".weight"] + [f"{pre}.norm.{s}" for s in BN]


def _block(pre, first):
    names = []
    for conv in (["shortcut"] if first else []) + ["conv1", "conv2", "conv3"]:
        names += _conv_bn(f"{pre}.{conv}")
    return names


def d2_c4_names():
    """The state_dict keys of detectron2's faster_rcnn_R_50_C4: no `bottom_up`, res5 under roi_heads."""
    names = _conv_bn("backbone.stem.conv1")
    for stage, nb in ((2, 3), (3, 4), (4, 6)):
        for b in range(nb):
            names += _block(f"backbone.res{stage}.{b}", b == 0)
    for b in range(3):
        names += _block(f"roi_heads.res5.{b}", b == 0)
    names += [f"proposal_generator.rpn_head.{l}.{p}" for l in ("conv", "objectness_logits", "anchor_deltas") for p in ("weight", "bias")]
    names += [f"roi_heads.box_predictor.{l}.{p}" for l in ("cls_score", "bbox_pred") for p in ("weight", "bias")]
    return sorted(names)


def test_the_shipped_yaml(osr):
    m = _cfg().MODEL
    assert m.META_ARCHITECTURE == "GeneralizedRCNN" and m.BACKBONE.NAME == "build_resnet_backbone"
    assert list(m.RESNETS.OUT_FEATURES) == ["res4"] and m.RESNETS.DEPTH == 50 and m.RESNETS.RES5_DILATION == 1
    assert list(m.RPN.IN_FEATURES) == ["res4"] and m.RPN.PRE_NMS_TOPK_TEST == 6000 and m.RPN.POST_NMS_TOPK_TEST == 1000
    assert [list(s) for s in m.ANCHOR_GENERATOR.SIZES] == [[32, 64, 128, 256, 512]]
    assert m.ROI_HEADS.NAME == "Res5ROIHeads" and list(m.ROI_HEADS.IN_FEATURES) == ["res4"]
    assert m.ROI_BOX_HEAD.POOLER_RESOLUTION == 14 and m.ROI_BOX_HEAD.POOLER_TYPE == "ROIAlignV2"
    assert m.MASK_ON is False and m.KEYPOINT_ON is False


def test_detectron2_base_rcnn_c4_yaml_merges_to_the_same_model(osr, tmp_path):
    (tmp_path / "Base-RCNN-C4.yaml").write_text(D2_BASE_C4_YAML)
    (tmp_path / "faster_rcnn_R_50_C4_1x.yaml").write_text(D2_R50_C4_1X_YAML)
    d2 = _cfg(yaml=str(tmp_path / "faster_rcnn_R_50_C4_1x.yaml"))
    ours = _cfg()
    assert d2.MODEL.WEIGHTS == "detectron2://ImageNetPretrained/MSRA/R-50.pkl"
    d2.MODEL.WEIGHTS = ours.MODEL.WEIGHTS
    assert d2.MODEL == ours.MODEL, "the shipped yaml spells out detectron2's defaults: the two configurations are one model"
    from openset_rcnn_amd.host import modeling as M
    assert sorted(M.build_model(d2).state_dict()) == d2_c4_names()


def test_both_names_are_registered(osr):
    from openset_rcnn_amd.host import modeling as M
    assert "build_resnet_backbone" in M.BACKBONE_REGISTRY and "Res5ROIHeads" in M.ROI_HEADS_REGISTRY
    assert not issubclass(M.Res5ROIHeads, M.StandardROIHeads)  # (what the TTA check and forward_with_given_boxes go by)


@pytest.mark.parametrize("k,agnostic", [(80, False), (7, True)])
def test_state_dict_is_detectron2s(osr, k, agnostic):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.engine_c4 import C4RCNNEngine
    model = M.build_model(_cfg("MODEL.ROI_HEADS.NUM_CLASSES", str(k), "MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", str(agnostic)))
    assert type(model).__name__ == "GeneralizedRCNN" and type(model.backbone).__name__ == "ResNetC4" and type(model.roi_heads) is M.Res5ROIHeads
    assert model._engine_cls is C4RCNNEngine and model.proposal_generator.rpn_head._engine_cls is C4RCNNEngine
    sd = model.state_dict()
    assert sorted(sd) == d2_c4_names()
    assert not [n for n in sd if "bottom_up" in n or "fpn" in n or "box_head" in n]
    shape = lambda n: tuple(sd[n].shape)  # noqa: E731
    assert shape("proposal_generator.rpn_head.conv.weight") == (1024, 1024, 3, 3)
    assert shape("proposal_generator.rpn_head.objectness_logits.weight") == (15, 1024, 1, 1)
    assert shape("proposal_generator.rpn_head.anchor_deltas.weight") == (60, 1024, 1, 1)
    assert shape("backbone.stem.conv1.weight") == (64, 3, 7, 7) and shape("backbone.res4.5.conv3.weight") == (1024, 256, 1, 1)
    assert shape("backbone.res4.0.shortcut.weight") == (1024, 512, 1, 1)
    assert shape("roi_heads.res5.0.shortcut.weight") == (2048, 1024, 1, 1) and shape("roi_heads.res5.0.conv1.weight") == (512, 1024, 1, 1)
    assert shape("roi_heads.res5.0.conv2.weight") == (512, 512, 3, 3) and shape("roi_heads.res5.2.conv3.weight") == (2048, 512, 1, 1)
    assert shape("roi_heads.res5.1.conv1.weight") == (512, 2048, 1, 1) and shape("roi_heads.res5.0.conv3.norm.running_var") == (2048,)
    assert shape("roi_heads.box_predictor.cls_score.weight") == (k + 1, 2048)
    assert shape("roi_heads.box_predictor.bbox_pred.weight") == ((4 if agnostic else 4 * k), 2048)
    ec = model._eng_cfg
    assert ec["anchor_sizes"] == ((32.0, 64.0, 128.0, 256.0, 512.0),) and ec["pooler_scales"] == (1.0 / 16,)
    assert ec["pre_nms_topk_test"] == 6000 and ec["post_nms_topk_test"] == 1000 and ec["pooler_resolution"] == 14 and ec["std_num_classes"] == k
    assert model.backbone.output_shape()["res4"].channels == 1024 and model.backbone.output_shape()["res4"].stride == 16


def test_deformable_res3_res4_come_with_the_trunk(osr):
    from openset_rcnn_amd.host import modeling as M
    sd = M.build_model(_cfg("MODEL.RESNETS.DEFORM_ON_PER_STAGE", "[False, True, True, False]", "MODEL.RESNETS.DEFORM_MODULATED", "True")).state_dict()
    extra = sorted(set(sd) - set(d2_c4_names()))
    assert extra == sorted(f"backbone.res{s}.{b}.conv2_offset.{p}" for s, nb in ((3, 4), (4, 6)) for b in range(nb) for p in ("weight", "bias"))
    assert tuple(sd["backbone.res4.0.conv2_offset.weight"].shape) == (27, 256, 3, 3)


def test_state_dict_round_trips_through_pth_and_pkl(osr, tmp_path):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.checkpoint import load_checkpoint, load_into
    torch.manual_seed(3)
    src = M.build_model(_cfg("MODEL.ROI_HEADS.NUM_CLASSES", "5"))
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    pth, pkl = str(tmp_path / "faster_rcnn_R_50_C4.pth"), str(tmp_path / "faster_rcnn_R_50_C4.pkl")
    torch.save({"model": sd, "iteration": 7}, pth)
    with open(pkl, "wb") as f:  # detectron2's model-zoo form
        pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "test"}, f)
    for path in (pth, pkl):
        torch.manual_seed(4)
        dst = M.build_model(_cfg("MODEL.ROI_HEADS.NUM_CLASSES", "5"))
        state = load_checkpoint(path)
        assert state.origin == "d2"
        missing, unexpected = load_into(dst, state, strict=True)
        assert not missing and not unexpected
        got = dst.state_dict()
        assert all(torch.equal(got[k], sd[k]) for k in sd)


def test_a_backbone_only_checkpoint_fills_the_trunk_and_res5(osr, tmp_path):
    """MSRA R-50.pkl (what faster_rcnn_R_50_C4_1x.yaml starts from): res2..res4 go to backbone.*, res5 to roi_heads.res5.*."""
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.checkpoint import load_checkpoint, load_into, msra_names_for
    torch.manual_seed(5)
    fpn = M.build_model(_cfg(yaml="base_rcnn_fpn.yaml")).state_dict()
    trunk = {k: v for k, v in fpn.items() if k.startswith("backbone.bottom_up.")}
    blobs = {msra: trunk[d2].numpy() for d2, msra in msra_names_for(trunk).items() if not d2.endswith(("running_mean", "running_var"))}
    path = str(tmp_path / "R-50.pkl")
    with open(path, "wb") as f:
        pickle.dump(blobs, f)
    model = M.build_model(_cfg())
    missing, unexpected = load_into(model, load_checkpoint(path))
    assert not unexpected
    assert sorted(missing) == sorted(n for n in d2_c4_names() if n.startswith(("proposal_generator.", "roi_heads.box_predictor.")))
    got = model.state_dict()
    assert torch.equal(got["backbone.res3.1.conv2.weight"], trunk["backbone.bottom_up.res3.1.conv2.weight"])
    assert torch.equal(got["backbone.stem.conv1.norm.weight"], trunk["backbone.bottom_up.stem.conv1.norm.weight"])
    assert torch.equal(got["roi_heads.res5.0.shortcut.weight"], trunk["backbone.bottom_up.res5.0.shortcut.weight"])
    assert torch.equal(got["roi_heads.res5.2.conv3.norm.bias"], trunk["backbone.bottom_up.res5.2.conv3.norm.bias"])


REFUSALS = [
    (["MODEL.MASK_ON", "True"], "MODEL.MASK_ON"),
    (["MODEL.KEYPOINT_ON", "True", "MODEL.ROI_HEADS.NUM_CLASSES", "1"], "MODEL.KEYPOINT_ON"),
    (["TEST.AUG.ENABLED", "True"], "TEST.AUG"),
    (["MODEL.RESNETS.RES5_DILATION", "2"], "MODEL.RESNETS.RES5_DILATION"),
    (["MODEL.RESNETS.DEFORM_ON_PER_STAGE", "[False, False, False, True]"], r"MODEL.RESNETS.DEFORM_ON_PER_STAGE\[3\]"),
    (["MODEL.RESNETS.OUT_FEATURES", "['res4', 'res5']"], "MODEL.RESNETS.OUT_FEATURES"),
    (["MODEL.RESNETS.OUT_FEATURES", "['res5']"], "MODEL.RESNETS.OUT_FEATURES"),
    (["MODEL.ROI_HEADS.NAME", "StandardROIHeads"], "MODEL.ROI_HEADS.NAME"),
    (["MODEL.BACKBONE.NAME", "build_resnet_fpn_backbone"], "MODEL.BACKBONE.NAME"),
    (["MODEL.RPN.PRE_NMS_TOPK_TEST", "8193"], "MODEL.RPN.PRE_NMS_TOPK_TEST"),
    (["MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", "15"], "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION"),
    (["MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIPool"], "MODEL.ROI_BOX_HEAD.POOLER_TYPE"),
]


@pytest.mark.parametrize("opts,key", REFUSALS, ids=[r[1].replace("\\", "") + "-" + r[0][1][:12] for r in REFUSALS])
def test_refusals_name_their_key(osr, opts, key):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match=key):
        M.build_model(_cfg(*opts))


def test_res5_heads_on_the_fpn_yaml_and_standard_heads_on_c4_are_refused(osr):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match="Res5ROIHeads"):
        M.build_model(_cfg("MODEL.ROI_HEADS.NAME", "Res5ROIHeads", yaml="base_rcnn_fpn.yaml"))
    with pytest.raises(ValueError, match="build_resnet_backbone"):
        M.build_model(_cfg("MODEL.ROI_HEADS.NAME", "CascadeROIHeads"))


def test_depth_keeps_its_message(osr):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(AssertionError, match="only R-50 is on the hot path"):
        M.build_model(_cfg("MODEL.RESNETS.DEPTH", "101"))


def test_training_is_refused_by_name(osr):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(_cfg())
    for call in (model.make_trainer, model.trainer, lambda: model.losses_forward([])):
        with pytest.raises(NotImplementedError, match='MODEL.ROI_HEADS.NAME "Res5ROIHeads"'):
            call()
    model.train()
    with pytest.raises(NotImplementedError, match='MODEL.ROI_HEADS.NAME "Res5ROIHeads"'):
        model([])
    with pytest.raises(NotImplementedError, match='MODEL.ROI_HEADS.NAME "Res5ROIHeads"'):
        model.roi_heads(None, {}, [], [])


def test_tta_wrapper_refuses_the_head(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    model = M.build_model(_cfg()).eval()
    with pytest.raises(ValueError, match="TEST.AUG"):
        GeneralizedRCNNWithTTA(_cfg(), model)


def test_no_engine_without_a_gpu(osr):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(_cfg()).eval()
    with pytest.raises(osr.OsrError):
        model([{"image": torch.zeros(3, 64, 64, dtype=torch.uint8)}])


def test_the_fpn_model_builds_with_identical_keys(osr):
    """base_rcnn_fpn.yaml as before this head existed: the stock modules, the stock engine, the same parameter names."""
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.engine_std import StandardRCNNEngine
    model = M.build_model(_cfg(yaml="base_rcnn_fpn.yaml"))
    assert type(model.backbone).__name__ == "ResNetFPN" and type(model.roi_heads) is M.StandardROIHeads and model._engine_cls is StandardRCNNEngine
    assert model.proposal_generator.rpn_head._engine_cls is StandardRCNNEngine and model._c4 is False
    sd = model.state_dict()
    trunk = [n.replace("backbone.", "backbone.bottom_up.", 1) for n in d2_c4_names() if n.startswith("backbone.")]
    trunk += [n.replace("roi_heads.", "backbone.bottom_up.", 1) for n in d2_c4_names() if n.startswith("roi_heads.res5.")]
    want = set(trunk)
    want |= {f"backbone.fpn_{kind}{l}.{p}" for kind in ("lateral", "output") for l in (2, 3, 4, 5) for p in ("weight", "bias")}
    want |= {f"proposal_generator.rpn_head.{l}.{p}" for l in ("conv", "objectness_logits", "anchor_deltas") for p in ("weight", "bias")}
    want |= {f"roi_heads.{l}.{p}" for l in ("box_head.fc1", "box_head.fc2", "box_predictor.cls_score", "box_predictor.bbox_pred") for p in ("weight", "bias")}
    assert set(sd) == want
    assert tuple(sd["proposal_generator.rpn_head.conv.weight"].shape) == (256, 256, 3, 3)
    assert tuple(sd["proposal_generator.rpn_head.objectness_logits.weight"].shape) == (3, 256, 1, 1)
    assert model._eng_cfg["anchor_sizes"] == (32.0, 64.0, 128.0, 256.0, 512.0) and model._eng_cfg["pooler_scales"] == (0.25, 0.125, 0.0625, 0.03125)
