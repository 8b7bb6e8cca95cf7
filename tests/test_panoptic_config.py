"""META_ARCHITECTURE "PanopticFPN" / "SemanticSegmentor" on the host side, without a GPU: the MODEL.SEM_SEG_HEAD and MODEL.PANOPTIC_FPN
defaults (detectron2 v0.6), configs/panoptic_fpn.yaml, the model mirror's parameter names and shapes for NORM "GN" and "", checkpoint
round trips, every refusal by its key, the training refusals by the meta architecture's name, and the table -> segments_info conversion."""
import os
import pickle

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVS = ("p2.0", "p3.0", "p4.0", "p4.2", "p5.0", "p5.2", "p5.4")


def _cfg(yaml="panoptic_fpn.yaml", *opts):
    from openset_rcnn_amd.host.config import add_openset_rcnn_config, get_cfg
    cfg = get_cfg()
    add_openset_rcnn_config(cfg)
    if yaml:
        cfg.merge_from_file(os.path.join(ROOT, "configs", yaml))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def test_defaults_are_detectron2s(osr):
    m = _cfg(None).MODEL
    assert dict(m.SEM_SEG_HEAD) == dict(NAME="SemSegFPNHead", IN_FEATURES=["p2", "p3", "p4", "p5"], IGNORE_VALUE=255, NUM_CLASSES=54, CONVS_DIM=128,
                                        COMMON_STRIDE=4, NORM="GN", LOSS_WEIGHT=1.0)
    assert m.PANOPTIC_FPN.INSTANCE_LOSS_WEIGHT == 1.0
    assert dict(m.PANOPTIC_FPN.COMBINE) == dict(ENABLED=True, OVERLAP_THRESH=0.5, STUFF_AREA_LIMIT=4096, INSTANCES_CONFIDENCE_THRESH=0.5)
    assert m.META_ARCHITECTURE == "GeneralizedRCNN"


def test_yaml_loads_and_restates_base_panoptic_fpn(osr):
    m = _cfg().MODEL
    assert m.META_ARCHITECTURE == "PanopticFPN" and m.MASK_ON is True and m.SEM_SEG_HEAD.LOSS_WEIGHT == 0.5
    assert m.BACKBONE.NAME == "build_resnet_fpn_backbone" and m.ROI_HEADS.NAME == "StandardROIHeads"  # (from base_rcnn_fpn.yaml)
    assert m.SEM_SEG_HEAD.NUM_CLASSES == 54 and m.PANOPTIC_FPN.COMBINE.ENABLED is True


@pytest.mark.parametrize("norm", ["GN", ""], ids=["GN", "none"])
@pytest.mark.parametrize("arch", ["PanopticFPN", "SemanticSegmentor"])
def test_parameter_names_and_shapes(osr, arch, norm):
    from openset_rcnn_amd.host import modeling as M
    torch.manual_seed(0)
    model = M.build_model(_cfg("panoptic_fpn.yaml", "MODEL.META_ARCHITECTURE", arch, "MODEL.SEM_SEG_HEAD.NORM", norm))
    assert type(model).__name__ == arch
    sd = model.state_dict()
    head = {k[len("sem_seg_head."):]: tuple(v.shape) for k, v in sd.items() if k.startswith("sem_seg_head.")}
    want = {"predictor.weight": (54, 128, 1, 1), "predictor.bias": (54,)}
    for c in CONVS:
        want[c + ".weight"] = (128, 256 if c.endswith(".0") else 128, 3, 3)
        if norm == "GN":
            want[c + ".norm.weight"] = want[c + ".norm.bias"] = (128,)
        else:
            want[c + ".bias"] = (128,)
    assert head == want
    # c2_msra_fill (fan_out, relu: std = sqrt(2 / (128 * 9))), GroupNorm weight 1 / bias 0, zero predictor bias
    assert 0.9 < float(sd["sem_seg_head.p5.2.weight"].std()) / (2.0 / (128 * 9)) ** 0.5 < 1.1
    assert float(sd["sem_seg_head.predictor.bias"].abs().max()) == 0.0
    if norm == "GN":
        assert bool((sd["sem_seg_head.p4.2.norm.weight"] == 1).all()) and bool((sd["sem_seg_head.p4.2.norm.bias"] == 0).all())
    stock = set(M.build_model(_cfg("base_rcnn_fpn.yaml", "MODEL.MASK_ON", "True")).state_dict())
    rest = {k for k in sd if not k.startswith("sem_seg_head.")}
    assert rest == (stock if arch == "PanopticFPN" else {k for k in stock if k.startswith("backbone.")})


def test_other_widths_and_class_counts(osr):
    from openset_rcnn_amd.host import modeling as M
    sd = M.build_model(_cfg("panoptic_fpn.yaml", "MODEL.SEM_SEG_HEAD.CONVS_DIM", "64", "MODEL.SEM_SEG_HEAD.NUM_CLASSES", "7")).state_dict()
    assert tuple(sd["sem_seg_head.p5.4.weight"].shape) == (64, 64, 3, 3) and tuple(sd["sem_seg_head.predictor.weight"].shape) == (7, 64, 1, 1)


def test_state_dict_round_trips_through_pth_and_pkl(osr, tmp_path):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.checkpoint import load_checkpoint, load_into
    torch.manual_seed(3)
    src = M.build_model(_cfg())
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    pth, pkl = str(tmp_path / "panoptic_fpn_R_50_1x.pth"), str(tmp_path / "panoptic_fpn_R_50_1x.pkl")
    torch.save({"model": sd, "iteration": 7}, pth)
    with open(pkl, "wb") as f:  # detectron2's model-zoo form
        pickle.dump({"model": {k: v.numpy() for k, v in sd.items()}, "__author__": "Detectron2 Model Zoo"}, f)
    for path in (pth, pkl):
        torch.manual_seed(4)
        dst = M.build_model(_cfg())
        state = load_checkpoint(path)
        assert state.origin == "d2"
        missing, unexpected = load_into(dst, state)
        assert not missing and not unexpected
        got = dst.state_dict()
        assert all(torch.equal(got[k], sd[k]) for k in sd)


@pytest.mark.parametrize("opts,key", [
    (("MODEL.SEM_SEG_HEAD.NORM", "BN"), "MODEL.SEM_SEG_HEAD.NORM"),
    (("MODEL.SEM_SEG_HEAD.CONVS_DIM", "96"), "MODEL.SEM_SEG_HEAD.CONVS_DIM"),
    (("MODEL.SEM_SEG_HEAD.COMMON_STRIDE", "8"), "MODEL.SEM_SEG_HEAD.COMMON_STRIDE"),
    (("MODEL.SEM_SEG_HEAD.IN_FEATURES", "['p3', 'p4', 'p5']"), "MODEL.SEM_SEG_HEAD.IN_FEATURES"),
    (("MODEL.SEM_SEG_HEAD.NUM_CLASSES", "256"), "MODEL.SEM_SEG_HEAD.NUM_CLASSES"),
    (("MODEL.SEM_SEG_HEAD.NUM_CLASSES", "0"), "MODEL.SEM_SEG_HEAD.NUM_CLASSES"),
    (("MODEL.SEM_SEG_HEAD.NAME", "DeepLabV3Head"), "MODEL.SEM_SEG_HEAD.NAME"),
    (("MODEL.KEYPOINT_ON", "True"), "KEYPOINT_ON"),
    (("TEST.AUG.ENABLED", "True"), "TEST.AUG"),
])
@pytest.mark.parametrize("arch", ["PanopticFPN", "SemanticSegmentor"])
def test_refusals_name_their_keys(osr, arch, opts, key):
    from openset_rcnn_amd.host import modeling as M
    with pytest.raises(ValueError, match=key):
        M.build_model(_cfg("panoptic_fpn.yaml", "MODEL.META_ARCHITECTURE", arch, *opts))


def test_panoptic_refusals(osr):
    from openset_rcnn_amd.host import modeling as M
    from openset_rcnn_amd.host.tta import GeneralizedRCNNWithTTA
    with pytest.raises(ValueError, match="MASK_ON"):
        M.build_model(_cfg("panoptic_fpn.yaml", "MODEL.MASK_ON", "False"))
    with pytest.raises(ValueError, match="MODEL.ROI_HEADS.NAME"):
        M.build_model(_cfg("panoptic_fpn.yaml", "MODEL.ROI_HEADS.NAME", "CascadeROIHeads"))
    # without the combine step the masks are not needed
    model = M.build_model(_cfg("panoptic_fpn.yaml", "MODEL.MASK_ON", "False", "MODEL.PANOPTIC_FPN.COMBINE.ENABLED", "False"))
    assert not model.combine_enabled and not [k for k in model.state_dict() if "mask_head" in k]
    for arch in ("PanopticFPN", "SemanticSegmentor"):
        model = M.build_model(_cfg("panoptic_fpn.yaml", "MODEL.META_ARCHITECTURE", arch)).eval()
        with pytest.raises(ValueError, match=f'META_ARCHITECTURE "{arch}"'):
            GeneralizedRCNNWithTTA(_cfg(), model)


@pytest.mark.parametrize("arch", ["PanopticFPN", "SemanticSegmentor"])
def test_training_is_refused_by_the_meta_architectures_name(osr, arch):
    from openset_rcnn_amd.host import modeling as M
    model = M.build_model(_cfg("panoptic_fpn.yaml", "MODEL.META_ARCHITECTURE", arch))
    model.train()
    want = f'MODEL.META_ARCHITECTURE "{arch}".*semantic loss.*GroupNorm backward'
    inputs = [{"image": torch.zeros(3, 32, 32, dtype=torch.uint8)}]
    with pytest.raises(NotImplementedError, match=want):
        model(inputs)
    with pytest.raises(NotImplementedError, match=want):
        model.make_trainer()
    with pytest.raises(NotImplementedError, match=want):
        model.trainer()
    with pytest.raises(NotImplementedError, match=want):
        model.losses_forward(inputs)


def test_engine_options_are_checked_without_a_model(osr):
    from openset_rcnn_amd.host.engine_panoptic import PanopticFPNEngine
    with pytest.raises(ValueError, match="MODEL.SEM_SEG_HEAD.CONVS_DIM"):
        PanopticFPNEngine({}, dict(sem_seg_convs_dim=100), torch.float32, "cpu")
    with pytest.raises(ValueError, match="conv"):
        PanopticFPNEngine({}, None, torch.float32, "cpu", conv="split")


def test_segment_table_to_segments_info(osr):
    ops = osr.ops
    table = torch.zeros(6, 4, dtype=torch.int32)
    table[0] = torch.tensor([1, 2, 0, 400])
    table[1] = torch.tensor([1, 0, 4, 360])
    table[2] = torch.tensor([0, 3, -1, 500])
    table[3] = torch.tensor([0, 9, -1, 77])  # beyond the count: not reported
    scores = torch.tensor([0.95, 0.7, 0.0, 0.0, 0.0, 0.0])
    info = ops.segments_info_from_table(table, scores, torch.tensor([3], dtype=torch.int32))
    assert info == [{"id": 1, "isthing": True, "score": float(torch.tensor(0.95)), "category_id": 2, "instance_id": 0},
                    {"id": 2, "isthing": True, "score": float(torch.tensor(0.7)), "category_id": 0, "instance_id": 4},
                    {"id": 3, "isthing": False, "category_id": 3, "area": 500}]
    assert all(type(v) in (int, float, bool) for d in info for v in d.values())
    assert ops.segments_info_from_table(table, scores, torch.tensor([0], dtype=torch.int32)) == []
